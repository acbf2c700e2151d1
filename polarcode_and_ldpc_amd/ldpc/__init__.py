"""LDPC codes: drop-in BP / Min-Sum decoders (HIP) + parity-check matrices."""
from .decoder import (BPDecoder, LayeredMSDecoder, MSDecoder, QCFixedMSDecoder, QCLayeredBPDecoder, QCLayeredMSDecoder,
                      quantize_host)
from .encoder import LDPCEncoder, QCLDPCEncoder, valid_generator
from .matrix import (calculate_girth, check_matrix_rank, create_systematic_generator, csr_to_dense, dense_to_csr,
                     generate_ldpc_matrix, gf2_systematic_pair, layer_schedule, mackay_construction, peg_construction,
                     qc_block_layers, qc_encodable_base, qc_encoding_structure, qc_expand, qc_random_base, qc_to_csr,
                     regular_construction)
from .ratematch import QCRateMatcher
from .utils import calculate_syndrome, check_syndrome, count_errors, create_tanner_graph, hamming_distance

__all__ = ["BPDecoder", "MSDecoder", "LayeredMSDecoder", "QCLayeredMSDecoder", "QCFixedMSDecoder", "QCLayeredBPDecoder", "quantize_host", "LDPCEncoder", "QCLDPCEncoder", "QCRateMatcher", "dense_to_csr", "csr_to_dense",
           "generate_ldpc_matrix", "mackay_construction", "regular_construction", "peg_construction",
           "layer_schedule", "create_systematic_generator", "check_matrix_rank", "calculate_girth",
           "gf2_systematic_pair", "create_tanner_graph", "check_syndrome", "calculate_syndrome", "count_errors",
           "hamming_distance", "qc_expand", "qc_to_csr", "qc_block_layers", "qc_random_base",
           "qc_encodable_base", "qc_encoding_structure"]

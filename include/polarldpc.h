/*
 * polarldpc.h -- C-ABI of libpolarldpc.so, the MI355X (gfx950) batched
 * channel decoder.  Plain pointers and sizes only; device pointers are
 * hipMalloc'd (e.g. torch tensors' data_ptr()); `stream` is a hipStream_t
 * passed as void* (NULL = legacy default stream).
 *
 * The reference (B1ear/PolarCode_and_LDPC) is pure Python/NumPy and has no FFI;
 * each entry point below replaces the body of a reference Python method.  The
 * Python drop-in classes (polarcode_and_ldpc_amd.polar.SCDecoder, ...) bind
 * these with ctypes; INTEGRATION.md shows the binding.
 *
 * Return codes: 0 ok, <0 error (PL_E*); pl_last_error() gives a thread-local
 * message for the last failing call on the calling thread.
 */
#ifndef POLARLDPC_H
#define POLARLDPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PL_OK 0
#define PL_EINVAL (-1)       /* bad argument (reference: AssertionError)        */
#define PL_ENOMEM (-2)       /* device allocation failed                         */
#define PL_EHIP (-3)         /* HIP runtime error (launch, copy)                 */
#define PL_EUNSUPPORTED (-4) /* valid for the reference but not for this build,  */
                             /* or MS on a degree-1 check (reference ValueError) */

#define PL_LDPC_BP 0 /* BPDecoder: sum-product, tanh rule   (src/ldpc/decoder.py:11-205)  */
#define PL_LDPC_MS 1 /* MSDecoder: (normalised) min-sum     (src/ldpc/decoder.py:208-355) */
#define PL_LDPC_LMS 2 /* layered (row-serial) normalised min-sum, build-defined
                         (pl_ldpc_layered_plan_create; no reference counterpart)   */

typedef struct pl_plan pl_plan;

typedef struct {
    int32_t kind;       /* 0 polar, 1 ldpc                                         */
    int32_t n_in;       /* LLRs per frame (N or n)                                 */
    int32_t n_out;      /* output bits per frame: K (polar) or n (ldpc)            */
    int32_t list_size;  /* polar: 0 = SC, >=1 = SCL list size                      */
    int32_t lds_bytes;  /* dynamic LDS per workgroup of the decode kernel          */
    int32_t fused_top;  /* polar: tree depths fused into the channel read (>=1)    */
    int32_t frames_per_block; /* frames one workgroup decodes: polar, frames per
                           wavefront; flooding LDPC, 2 on the degree-grouped BP
                           kernel's two-frame instance, else 1; layered LDPC,
                           frames per workgroup (one wavefront each), 1 when a
                           workgroup decodes one frame; quasi-cyclic layered LDPC,
                           frames per workgroup (64 / Z per wavefront for Z <= 64) */
    int32_t reserved;   /* polar: kernel (4 tree, 3 lane, 6 single-workgroup exact);
                           LDPC: 2 register-cached, 7 register-cached BP with
                           degree-grouped check products, 1 generic,
                           3 thread-per-check, 5 min-sum with compressed check state,
                           8 (3,6)-regular min-sum with rebuild-ready check state,
                           9 layered min-sum with its state in LDS,
                           10 layered min-sum with its state in the workspace,
                           11 quasi-cyclic layered min-sum with its state in LDS,
                           12 quasi-cyclic layered min-sum with its state in the
                           workspace,
                           13 / 14 the same two with the state in single precision
                           (PL_LDPC_QC_F32),
                           15 int8 fixed-point quasi-cyclic layered min-sum with its
                           state in LDS, 16 with its state in the workspace (such a
                           plan reports in fused_top the kernel instance: 8, 16 or 32
                           inputs of a check kept in registers, 0 the two-pass form),
                           17 fp64 quasi-cyclic layered sum-product with its state in
                           LDS, 18 with its state in the workspace */
} pl_plan_info;

/* Polar SC / SCL plan.
 *   Replaces SCDecoder.__init__ (src/polar/decoder.py:16-36) when list_size == 0
 *   and SCLDecoder.__init__ (src/polar/decoder.py:191-223) when list_size >= 1.
 *   frozen_mask: host array [N], nonzero = frozen (the reference's frozen_bits
 *   index set as a mask; info bits = the complement, ascending).
 *   N power of two (2..32768); K = number of unfrozen positions, 1 <= K <= N
 *   (the reference's 0 < K < N assertion, decoder.py:17-18, is made by the
 *   Python layer on its K argument, exactly as the reference does).
 *   list_size: lists above 64 run one frame per workgroup of list_size/64
 *   wavefronts (16-bit path slots above 256); lists above 1024 run every frame
 *   through the exact single-workgroup decoder of polar_nan.hip (milliseconds
 *   per frame; its per-frame list state in LDS up to 2048 paths, in the
 *   workspace above).  list_size > 65536 or list_size * N > 2^30 returns
 *   PL_EUNSUPPORTED (the reference accepts any L, its scripts use <= 32).
 *   Cost of the largest lists: one frame's list state takes about
 *   list_size * N * 11 bytes of workspace (path LLR + bit arrays; 11 GB at
 *   list_size * N = 2^30, refused when larger than the device's memory), and
 *   one thread sorts the 2 * list_size candidates of every information bit,
 *   so such a frame takes seconds to minutes.  Tested up to list_size 4096.
 *   flags: 0 = fastest kernel built for (N, list size).  Diagnostics: bits 0-3
 *   force the lane kernel (polar_lane.hip) with that fused-top depth, 0x10 or
 *   0x20 the lane kernel with its default depth.
 *   The plan owns device constants only; decode workspace is per stream (grown
 *   lazily to the batch, see pl_decode) or caller-supplied (pl_decode_ws). */
int pl_polar_plan_create(int32_t N, int32_t K, const uint8_t* frozen_mask, int32_t list_size,
                         int32_t flags, pl_plan** out);

/* CRC-aided list selection (build-defined extension: the reference stores
 *   SCLDecoder's use_crc / crc_polynomial but never reads them, decoder.py:202-203,
 *   259).  With crc_len > 0 the decoded path is the first one, in descending
 *   final-metric order (ties: lower list index), whose u_hat[info bits] passes
 *   crc_check of src/polar/utils.py:128-163 (bit-serial, MSB first, zero initial
 *   register, generator `poly` without its x^crc_len term, e.g. CRC-8 0x1D,
 *   CRC-16 0x1021, CRC-24 0x1864CFB); if none passes, the argmax path.
 *   crc_len == 0 restores plain SCL.  List plans only (list_size >= 1). */
int pl_polar_plan_set_crc(pl_plan* plan, int32_t crc_len, uint32_t poly);

/* LDPC plan.  Replaces BPDecoder.__init__/_build_tanner_graph
 *   (src/ldpc/decoder.py:18-60) for algo PL_LDPC_BP and MSDecoder.__init__
 *   (:215-255) for PL_LDPC_MS.  H given as CSR over its m rows with ascending
 *   column indices: row_ptr[m+1], col_idx[row_ptr[m]] (host arrays).
 *   normalization is MSDecoder's factor (ignored for BP). */
int pl_ldpc_plan_create(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                        int32_t algo, int32_t max_iter, int32_t early_stop, double normalization,
                        int32_t flags, pl_plan** out);

/* Layered (row-serial) normalised min-sum plan.  Build-defined extension: the
 *   reference has flooding decoders only.  H as for pl_ldpc_plan_create.  The
 *   rows are visited layer by layer: layer l holds rows
 *   layer_rows[layer_ptr[l] .. layer_ptr[l+1]) (host arrays, layer_ptr[n_layers+1],
 *   layer_rows[m]).  All fp64:
 *     P[v] = llr[v]; R[c][j] = 0
 *     for it < max_iter: for each layer in order, for each row c of it (deg > 0):
 *         q[j] = P[v_j] - R[c][j]
 *         R[c][j] = (prod_{k != j} sign(q[k]) * min_{k != j} |q[k]|) * normalization
 *                   (MSDecoder._check_node_update_ms on q, NumPy special values)
 *         P[v_j] = q[j] + R[c][j]
 *       decoded = P <= 0; with early_stop, stop once H decoded = 0 (iterations = it + 1)
 *   max_iter == 0 returns the decisions of the channel LLRs, iterations 0.
 *   PL_EINVAL unless the layers list every row exactly once and no two rows of a
 *   layer share a column; PL_EUNSUPPORTED for a degree-1 row when max_iter > 0
 *   (empty minimum; with max_iter == 0 no check is evaluated, as in MSDecoder)
 *   or a row degree >= 2048.  Every argument check runs before the first device call.
 *   One thread updates one check; a code whose largest layer has <= 64 rows runs
 *   one wavefront per frame (several frames per workgroup), others one workgroup
 *   per frame.  The per-frame state (P and the compressed check state, about
 *   8 n + 20 m bytes) lives in LDS when it fits 160 KB (pl_plan_info.reserved
 *   9), else in the workspace (10); PL_LMS_GLOBAL=1 at plan creation forces the
 *   workspace (diagnostic).  pl_decode, pl_decode_ws, pl_plan_workspace_bytes,
 *   pl_plan_reserve and pl_plan_release work as for any plan. */
int pl_ldpc_layered_plan_create(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_rows,
                                int32_t max_iter, int32_t early_stop, double normalization, int32_t flags,
                                pl_plan** out);

/* Quasi-cyclic layered normalised min-sum plan.  Build-defined, as the layered
 *   plan.  H is mb x nb blocks of z x z: shift[i * nb + j] (host array, row-major)
 *   is -1 for a zero block, else s in 0 .. z-1 for the cyclically shifted identity
 *   H[i z + r, j z + (r + s) % z] = 1, r = 0 .. z-1 (one circulant per block).
 *   The decoder is by definition pl_ldpc_layered_plan_create's on that H with
 *   the block rows as layers, layer l = rows [i z, (i+1) z) for i = layer_order[l]
 *   (host array [mb], a permutation of 0 .. mb-1; NULL: 0 .. mb-1): same bits,
 *   iteration counts and posteriors, bit for bit.  H is never expanded.
 *   PL_EINVAL for mb, nb or z < 1, nb z or mb z beyond int32, a shift outside
 *   -1 .. z-1, a layer_order that is no permutation, max_iter < 0;
 *   PL_EUNSUPPORTED for a block row with exactly one non-zero block when
 *   max_iter > 0 (as the layered plan's degree-1 row), a block row with >= 2048
 *   non-zero blocks, z > 1024.  A block row without blocks is skipped.  Every
 *   argument check runs before the first device call.
 *   One thread updates one check of the current block row; for z <= 64, 64 / z
 *   frames share a wavefront (each stops on its own zero syndrome), otherwise
 *   one workgroup of z threads (rounded up to 64) decodes a frame.  The state
 *   (as the layered plan's) lives in LDS when it fits 160 KB
 *   (pl_plan_info.reserved 11), else in the workspace (12); PL_LMS_GLOBAL=1
 *   forces the workspace.  pl_decode, pl_decode_ws, pl_ldpc_decode_soft,
 *   pl_plan_workspace_bytes, pl_plan_reserve and pl_plan_release work as for a
 *   layered plan.
 *   flags: bit 0 is PL_LDPC_QC_F32, the other bits are ignored.
 *   PL_LDPC_QC_F32: the same decoder with every value and every operation in
 *   IEEE binary32 -- the layered definition printed at
 *   pl_ldpc_layered_plan_create, read in single precision:
 *     P[v] = (float)llr[v]   round to nearest even for an fp64 input (beyond
 *                            FLT_MAX: +-inf; 5e-324: 0), an fp32 input as it is
 *     norm32 = (float)normalization, rounded once on the host
 *     q[j] = P[v_j] - R[c][j]
 *     R[c][j] = (prod_{k != j} sign(q[k]) * min_{k != j} |q[k]|) * norm32
 *     P[v_j] = q[j] + R[c][j]
 *   each step one rounding (no FMA contraction, no double intermediate),
 *   subnormals kept (not flushed); NaN, zero and sign rules as in fp64;
 *   decisions P <= 0 and the early stop as in fp64.  Bits, iteration counts and
 *   posteriors equal a NumPy float32 restatement bit for bit; they are not the
 *   fp64 decoder's rounded.  State per frame 4 n + 8 m + 4 mw m bytes (mw meta
 *   words per check) against 8 n + 16 m + 4 mw m, under the same LDS rules
 *   (pl_plan_info.reserved 13 in LDS, 14 in the workspace; the workspace unit
 *   is the single-precision state).  Such a plan takes fp32 LLRs through
 *   pl_ldpc_decode_f32, and fp64 LLRs through pl_decode, pl_decode_ws and
 *   pl_ldpc_decode_soft, which round each LLR on load and widen the posteriors
 *   on store (exact), with no conversion pass. */
#define PL_LDPC_QC_F32 1
int pl_ldpc_qc_plan_create(int32_t mb, int32_t nb, int32_t z, const int32_t* shift /* [mb*nb] row-major */,
                           const int32_t* layer_order /* [mb] or NULL */, int32_t max_iter, int32_t early_stop,
                           double normalization, int32_t flags, pl_plan** out);

/* int8 fixed-point quasi-cyclic layered normalised min-sum plan.  Build-defined.
 *   The code (mb, nb, z, shift), the layers (layer_order), the position j of an
 *   input in its check (the rank of its block column among the row's non-zero
 *   blocks), the skipping of block rows without blocks and max_iter == 0 are
 *   exactly pl_ldpc_qc_plan_create's.  Parameters: norm16 in 1 .. 16 (the
 *   normalisation is norm16 / 16), llr_max in 1 .. 127, msg_max in 1 .. 127.
 *   All arithmetic is on integers and no intermediate overflows (|values| <= 254):
 *     P[v] = clamp(L[v], -llr_max, llr_max)      L int8, any of its 256 values
 *                                                (so -128 -> -llr_max)
 *     R[c][j] = 0
 *     for it < max_iter: for each block row in layer_order (d >= 2 blocks), for
 *                        each of its z checks c:
 *         q[j]    = clamp(P[v_j] - R[c][j], -127, 127)
 *         mag_j   = min(msg_max, (min_{k != j} |q[k]| * norm16) >> 4)
 *         R[c][j] = (odd number of k != j with q[k] < 0) ? -mag_j : mag_j
 *         P[v_j]  = clamp(q[j] + R[c][j], -127, 127)
 *       decoded = P <= 0; with early_stop, stop once every parity is even
 *       (iterations = it + 1)
 *   A zero q[k] counts as non-negative; its sign never shows, because it makes
 *   the minimum 0.  No NaN, no signed zero, no rounding: bits, iteration counts
 *   and posteriors equal a NumPy integer restatement exactly.  With norm16 = 16,
 *   msg_max = 127 and inputs for which no clamp ever acts this is the fp64
 *   decoder of pl_ldpc_qc_plan_create at normalisation 1.0 on the same integers.
 *   Checks: pl_ldpc_qc_plan_create's in its order, with norm16, llr_max and msg_max
 *   (PL_EINVAL, in this order, the message names the first one violated) behind
 *   the layer_order check and in front of the PL_EUNSUPPORTED ones (a one-block
 *   row when max_iter > 0, >= 2048 blocks in a row, z > 1024).  Every argument
 *   check runs before the first device call.
 *   Mapping as pl_ldpc_qc_plan_create's.  State per frame, mw u32 words per check
 *   and then the posteriors.  With min1 <= min2 the two smallest |q| of a check,
 *   s1 = min(msg_max, min1 norm16 >> 4), s2 the same of min2, idx1 the position
 *   of min1 (the first on a tie), maxdc the largest row degree of the code:
 *     at 0         [m][mw] u32.
 *                  maxdc <= 14, mw = 1: s1 in bits 0-6, s2 in bits 7-13, idx1 in
 *                  bits 14-17, the negative flags in bits 18-31 (position j at bit
 *                  18 + j); the parity of the negative inputs is their popcount.
 *                  maxdc > 14, mw = 1 + ceil(maxdc / 32): word 0 = s1 in bits 0-7,
 *                  s2 in bits 8-15, idx1 in bits 16-26, the parity in bit 27;
 *                  words 1 ..: the negative flags, position j at bit j % 32 of
 *                  word 1 + j / 32.
 *                  R[c][j] = +- (j == idx1 ? s2 : s1), negative iff parity != flag j.
 *     at 4 m mw    P[n] int8
 *   4 m mw + n bytes rounded up to 16 (n + 4 m for degrees <= 14, n + 8 m up to 32), in LDS
 *   under pl_ldpc_qc_plan_create's rules (pl_plan_info.reserved 15), else in the
 *   workspace (16); PL_LMS_GLOBAL=1 forces the workspace.
 *   Such a plan decodes through pl_ldpc_decode_i8 only: pl_decode, pl_decode_ws,
 *   pl_ldpc_decode_soft and pl_ldpc_decode_f32 return PL_EUNSUPPORTED.
 *   pl_plan_workspace_bytes, pl_plan_reserve and pl_plan_release work as for any plan. */
int pl_ldpc_qc_fixed_plan_create(int32_t mb, int32_t nb, int32_t z, const int32_t* shift /* [mb*nb] row-major */,
                                 const int32_t* layer_order /* [mb] or NULL */, int32_t max_iter, int32_t early_stop,
                                 int32_t norm16, int32_t llr_max, int32_t msg_max, pl_plan** out);

/* fp64 quasi-cyclic layered sum-product (belief propagation) plan.  Build-defined.
 *   The code (mb, nb, z, shift), the layers (layer_order), the position j of an
 *   input in its check (the rank of its block column among the row's non-zero
 *   blocks), the skipping of block rows without blocks, max_iter == 0, the
 *   stop rule and the hard decision are exactly pl_ldpc_qc_plan_create's; the
 *   check rule and the state differ.  Every operation below is one IEEE
 *   binary64 operation (no FMA contraction).
 *   clampq(x) = +0.0 if x is NaN; clip if x > clip; -clip if x < -clip; else x.
 *   boxplus(a, b), in this order:
 *     m  = |b| < |a| ? |b| : |a|
 *     s  = ((a < 0) != (b < 0)) ? -m : m
 *     cp = log1p(expm1(-|a + b|) + 1.0)
 *     cm = log1p(expm1(-|a - b|) + 1.0)
 *     boxplus = s + (cp - cm)
 *   with expm1 and log1p those of glibc 2.35 (dbl-64), bit for bit; their
 *   arguments here are <= 0 and in [0, 1].
 *     P[v] = clampq(L[v]);  every R = +0.0
 *     for it < max_iter: for each block row in layer_order (d >= 2 blocks), for
 *                        each of its z checks, inputs j = 0 .. d-1 by ascending
 *                        block column:
 *         q_j      = clampq(P[v_j] - R_j)
 *         F_0      = q_0;      F_j = boxplus(F_(j-1), q_j)   j = 1 .. d-2
 *         B_(d-1)  = q_(d-1);  B_j = boxplus(q_j, B_(j+1))   j = d-2 .. 1
 *         R'_0     = B_1;      R'_(d-1) = F_(d-2)
 *         R'_j     = boxplus(F_(j-1), B_(j+1))               0 < j < d-1
 *         P[v_j]   = q_j + R'_j;  R_j = R'_j
 *       (d == 2: the two inputs swap)
 *       decoded = P <= 0; with early_stop, a frame whose every parity is even
 *       after an iteration stops updating (iterations = it + 1)
 *   The posterior output is P.  With the clamp every value stays finite,
 *   |P| <= 2 clip + ln 2, so NaN and +-inf are ordinary inputs: a NaN LLR is an
 *   erasure (+0.0), +-inf is +-clip.  Bits, iteration counts and posteriors
 *   equal a NumPy restatement bit for bit.
 *   Checks: pl_ldpc_qc_plan_create's in its order, with clip (finite,
 *   0 < clip <= 2^20, else PL_EINVAL) behind the layer_order check and in front
 *   of the PL_EUNSUPPORTED ones (a one-block row when max_iter > 0, with a
 *   message of its own; >= 2048 blocks in a row; z > 1024).  Every argument
 *   check runs before the first device call.
 *   Mapping as pl_ldpc_qc_plan_create's.  State per frame: P[n] f64 at 0; at
 *   off_r = 8 n rounded up to 16, R as [blocks][z] f64, where edge j of a layer
 *   is slot (blocks of the earlier layers in stream order) + j and check r of
 *   the layer is element slot z + r; state_bytes = off_r + 8 z blocks rounded
 *   up to 16, in LDS under pl_ldpc_qc_plan_create's rules
 *   (pl_plan_info.reserved 17), else in the workspace (18); PL_LMS_GLOBAL=1
 *   forces the workspace.  Such a plan decodes fp64 LLRs through pl_decode,
 *   pl_decode_ws and pl_ldpc_decode_soft, as the fp64 plan of
 *   pl_ldpc_qc_plan_create; pl_ldpc_decode_f32 and pl_ldpc_decode_i8 return
 *   PL_EUNSUPPORTED.  pl_plan_workspace_bytes, pl_plan_reserve and
 *   pl_plan_release work as for any plan. */
int pl_ldpc_qc_bp_plan_create(int32_t mb, int32_t nb, int32_t z, const int32_t* shift /* [mb*nb] row-major */,
                              const int32_t* layer_order /* [mb] or NULL */, int32_t max_iter, int32_t early_stop,
                              double clip, pl_plan** out);

/* Batched decode: replaces SCDecoder.decode (decoder.py:38-71),
 *   SCLDecoder.decode (:225-262), BPDecoder.decode (src/ldpc/decoder.py:124-202)
 *   and MSDecoder.decode (:289-352) applied to `batch` frames.
 *   llr_dev : fp64 [batch][ld] device, row b = channel LLRs of frame b (n_in used)
 *   bits_dev: uint8 [batch][n_out] device, rows contiguous (pitch n_out).
 *             Polar: u_hat[info_bits] ascending; LDPC: the full hard-decision
 *             word (decoded = total <= 0).
 *   iters_dev: int32 [batch] device or NULL; LDPC: iterations run (BPDecoder's
 *             return_iterations); polar: ignored.
 *   Asynchronous on `stream`.  Deterministic bits: the decode path's atomics
 *   (the polar list kernels' frame-group counter and NaN mask ORs, LDPC
 *   syndrome XORs in LDS) decide which wavefront decodes which frames, never
 *   what a frame decodes to.
 *   Workspace: the plan keeps one device buffer per stream, sized on first use
 *   to this batch (polar: one slice per resident wavefront, at most the
 *   persistent grid; LDPC codes whose messages exceed LDS: one per frame of a
 *   chunk) and grown when a larger batch arrives (after draining that stream).
 *   Host threads may share a plan when each uses its own stream; calls on one
 *   stream are serialised by the plan. */
int pl_decode(pl_plan* plan, const double* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
              int32_t* iters_dev, void* stream);

/* Workspace bytes pl_decode_ws needs to decode `batch` frames at full speed
 * (0: the kernel needs none).  Any size >= one unit works: a smaller
 * workspace runs fewer resident wavefronts / smaller LDPC chunks. */
int pl_plan_workspace_bytes(const pl_plan* plan, int64_t batch, int64_t* bytes);

/* pl_decode with a caller-supplied device workspace (the caller owns it and
 * must not use it concurrently elsewhere); no allocation, so safe inside
 * hipGraph capture. */
int pl_decode_ws(pl_plan* plan, const double* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                 int32_t* iters_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* pl_decode of a layered (or quasi-cyclic layered) min-sum plan that also writes the final posteriors
 * P (the state the decisions are taken from: bits = P <= 0) to post_dev, fp64
 * [batch][ld_post] device, ld_post >= n.  Bits, iteration counts and posteriors
 * are reproducible bit for bit (no transcendental is involved; NaN payloads
 * and the sign of a zero are unspecified).  PL_EUNSUPPORTED for every other
 * plan kind.  Workspace as pl_decode. */
int pl_ldpc_decode_soft(pl_plan* plan, const double* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                        int32_t* iters_dev, double* post_dev, int64_t ld_post, void* stream);

/* Decode of a quasi-cyclic plan created with PL_LDPC_QC_F32 from fp32 LLRs:
 * llr_dev fp32 [batch][ld]; post_dev fp32 [batch][ld_post], ld_post >= n, or
 * NULL for no posterior output; workspace_dev NULL: the plan's per-stream
 * workspace as pl_decode, else a caller-owned one of workspace_bytes as
 * pl_decode_ws (no allocation).  The other arguments as pl_decode.
 * PL_EUNSUPPORTED for every plan without the flag. */
int pl_ldpc_decode_f32(pl_plan* plan, const float* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                       int32_t* iters_dev, float* post_dev /* may be NULL */, int64_t ld_post,
                       void* workspace_dev /* NULL: the plan's per-stream workspace */, int64_t workspace_bytes,
                       void* stream);

/* Decode of a fixed-point plan (pl_ldpc_qc_fixed_plan_create): llr_dev int8
 * [batch][ld]; post_dev int8 [batch][ld_post], ld_post >= n, the final P, or NULL;
 * workspace_dev NULL: the plan's per-stream workspace as pl_decode, else a
 * caller-owned one of workspace_bytes, aligned to 16 bytes, as pl_decode_ws (no
 * allocation, so safe inside hipGraph capture).  The other arguments as pl_decode.
 * PL_EUNSUPPORTED for every other plan. */
int pl_ldpc_decode_i8(pl_plan* plan, const int8_t* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                      int32_t* iters_dev, int8_t* post_dev /* may be NULL */, int64_t ld_post,
                      void* workspace_dev /* NULL: the plan's per-stream workspace */, int64_t workspace_bytes,
                      void* stream);

/* The LLR quantiser in front of pl_ldpc_decode_i8:
 *     out[b][v] = clamp(rint((double)llr[b][v] * scale), -llr_max, llr_max)   as int8
 * rint rounds half to even; the input is fp64, or fp32 (PL_QUANT_LLR_F32) widened
 * exactly; the product is one fp64 multiplication; NaN -> 0, +-inf -> +-llr_max.
 * llr_dev [batch][ld], out_dev int8 [batch][ld_out], pitches in elements, any
 * pitch >= n and any out_dev address (16-byte stores where the addresses allow).
 * PL_EINVAL: unknown flag bits, batch < 0, n < 1, a scale that is not a finite
 * double > 0, llr_max outside 1 .. 127, a pitch < n, and for batch > 0 a NULL
 * pointer or an llr_dev not aligned to its element type.  batch == 0 does nothing. */
#define PL_QUANT_LLR_F32 1
int pl_llr_quantize(const void* llr_dev, int32_t flags, int64_t ld, int64_t batch, int32_t n, double scale,
                    int32_t llr_max, int8_t* out_dev, int64_t ld_out, void* stream);

/* Pre-allocate `stream`'s workspace for batches up to max_batch, so that
 * pl_decode on that stream never allocates (max_batch == 0: pl_plan_release).
 * If the device cannot hold the full-speed size, the largest halving of at
 * least one unit is kept (fewer resident wavefronts, same results) and later
 * decodes of up to max_batch frames run on it without retrying the allocation;
 * only another pl_plan_reserve (or a larger batch) retries. */
int pl_plan_reserve(pl_plan* plan, int64_t max_batch, void* stream);

/* Free `stream`'s workspace (after draining that stream).  A finished stream's
 * buffer is otherwise kept until pl_plan_destroy, invisible to torch's
 * caching allocator.  No-op for a stream the plan has not decoded on. */
int pl_plan_release(pl_plan* plan, void* stream);

/* Number of per-stream workspaces the plan holds and their total bytes. */
int pl_plan_workspace_stats(const pl_plan* plan, int64_t* streams, int64_t* bytes);

int pl_plan_get_info(const pl_plan* plan, pl_plan_info* info);
/* Build-defined extension (no reference counterpart): the largest batch a
 * pl_decode of this polar plan runs on its small-batch tree instance (one more
 * LDS depth and a 2-wave register budget, polar_tree.hip tree_table_small;
 * bits identical to the product instance), 0 if it has none.  Such batches fit
 * the device at 8 wavefronts per CU, where that instance is 6-15 % faster;
 * larger ones run the product instance (16 per CU).  PL_TREE_SMALL=0 at plan
 * creation turns it off. */
int pl_polar_plan_small_batch(const pl_plan* plan, int64_t* max_frames);
int pl_plan_destroy(pl_plan* plan);
const char* pl_last_error(void);

/* Calls that touch a plan's device memory -- pl_decode, pl_decode_ws,
 * pl_ldpc_decode_soft, pl_ldpc_decode_f32, pl_ldpc_decode_i8, pl_plan_reserve, pl_plan_release, pl_polar_plan_set_crc, pl_polar_encode,
 * pl_debug_polar_stamps -- must run with the plan's device current (the device
 * current at plan creation); otherwise they return PL_EINVAL and do nothing.
 * pl_plan_get_info, pl_plan_workspace_bytes and pl_plan_workspace_stats read
 * host state only; pl_plan_destroy may run on any device. */

/* Diagnostic build only (make DIAG=1; the product library returns
 * PL_EUNSUPPORTED): pl_decode of a polar plan through an instrumented kernel that adds
 * per-phase s_memtime cycle totals (summed over all frames) into stamps_dev[16]:
 * tree kernel (pl_plan_info.reserved == 4): [0] fused top, [1] workspace chains,
 * [2] LDS chain, [3] path metrics, [4] pruning/cloning, [5] partial-sum walk,
 * [6] final selection/output, [7] workspace fences; then counts of the
 * path-metric evaluations: [8] per-wave calls, [9] calls with a lane that
 * evaluates log1p(e^-x), [10] such lanes, [11] active lanes.  Timing differs
 * from pl_decode; read shares. */
int pl_debug_polar_stamps(pl_plan* plan, const double* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                          unsigned long long* stamps_dev, void* stream);

/* Diagnostic build only (the product library returns PL_EUNSUPPORTED): the
 * frame-per-wavefront SCL prototype (one wavefront per frame, eight lanes per
 * list path, every LLR pool in LDS) on a polar N=1024 L=8
 * plan, for timing against pl_decode.  stamps_dev[5] (may be NULL) receives
 * per-phase s_memtime cycle totals: descent, metric, pruning, partial sums,
 * output.  grid <= 0: one wavefront per LDS slot of the device. */
int pl_debug_polar_fpw(pl_plan* plan, const double* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                       unsigned long long* stamps_dev, int32_t grid, void* stream);

/* Diagnostic build only (the product library returns PL_EUNSUPPORTED): the
 * dead-store bound of the SCL N=1024 L=8 tree kernel.  mode 1
 * decodes recording, per frame group of 8 frames, which workspace pool arrays
 * (depths F..DL-1, one bit per node and lane plane) a right child's g reads and
 * which were stored: mask_dev u32 [ceil(batch/8)][2][words], zeroed by the
 * caller; mode 2 decodes the same frames again with every store of an array
 * not read in mode 1 skipped.  Bits equal pl_decode's by construction. */
int pl_debug_polar_deadstore(pl_plan* plan, const double* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                             uint32_t* mask_dev, int32_t mode, void* stream);

/* Diagnostic build only (the product library returns PL_EUNSUPPORTED): BP
 * decode of a (504,252)-class LDPC plan on the degree-grouped kernel with
 * per-phase s_memtime cycle totals added into stamps_dev[4][8] (per wavefront
 * index of the workgroup = per SIMD): [0] init, [1] early-stop vote, [2] check
 * pass, [3] its barrier, [4] variable pass, [5] tanh list, [6] closing
 * barrier, [7] output.  Timing differs from pl_decode; read shares. */
int pl_debug_ldpc_stamps(pl_plan* plan, const double* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                         int32_t* iters_dev, unsigned long long* stamps_dev, void* stream);

/* Test hook, diagnostic build only (the product library returns
 * PL_EUNSUPPORTED): pl_decode of a list plan that also reports which frames the
 * list kernel flagged for the exact NaN-order redo decoder (frames with a NaN
 * input or two inputs of magnitude >= 2^1000 / inf; polar_tree.hip).
 * flagged_host: `batch` host bytes, 1 = flagged.  Bits are the product path's. */
int pl_debug_polar_flagged(pl_plan* plan, const double* llr_dev, int64_t batch, int64_t ld, uint8_t* bits_dev,
                           uint8_t* flagged_host, void* stream);

/* Test hook, diagnostic build only (the product library returns
 * PL_EUNSUPPORTED): overwrite the device id a plan is bound to, so the
 * wrong-device check can be exercised on a one-GPU machine.  UNSAFE: it turns
 * the wrong-device protection off for that plan. */
int pl_debug_set_plan_device(pl_plan* plan, int32_t device);

/* What the host-side LDPC planner (csrc/ldpc_plan.cpp) decides for a code,
 * without creating a plan: no device call, so it runs on a machine without a
 * GPU.  Product and diagnostic builds.  Arguments as pl_ldpc_plan_create (same
 * checks, codes and messages), with the planning switches given explicitly
 * instead of read from the environment: kernel_override one of
 * PL_LDPC_KERNEL_* (PL_LDPC_KERNEL; CHECK counts in the diagnostic build only),
 * bp_fpg the PL_BP_FPG value (0: the kernel's default, 1, anything else 2),
 * lms_global the PL_LMS_GLOBAL flag (layered plans only). */
#define PL_LDPC_KERNEL_DEFAULT 0
#define PL_LDPC_KERNEL_GENERIC 1
#define PL_LDPC_KERNEL_REG 2
#define PL_LDPC_KERNEL_COMPACT 3
#define PL_LDPC_KERNEL_CHECK 4
typedef struct {
    int32_t kernel;      /* the pl_plan_info.reserved code the plan would report */
    int32_t threads, lds_bytes, use_global, reg_variant, grp, fpg, tl, npad, compact, ms36;
    int64_t work_bytes_per_frame;
    int64_t table_len;   /* int32 elements of the plan's one device table buffer   */
    int64_t grp_at, ms_vw_at; /* element offsets of the degree-grouped BP tables and
                            of the (3,6) min-sum address words in it             */
    uint64_t digest;     /* 64-bit FNV-1a over the buffer's bytes                  */
} pl_ldpc_plan_probe;
int pl_debug_ldpc_plan_probe(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx, int32_t algo,
                             int32_t max_iter, int32_t early_stop, double normalization, int32_t kernel_override,
                             int32_t bp_fpg, int32_t lms_global, pl_ldpc_plan_probe* out);
/* The same for pl_ldpc_layered_plan_create: the layered kernel's geometry. */
typedef struct {
    int32_t kernel;      /* 9 or 10, as pl_plan_info.reserved */
    int32_t maxdc, n_layers, max_layer, mw, wave, use_global, fpb, threads, lds_bytes;
    int64_t state_bytes, off_mm, off_meta;
    int64_t table_len;
    uint64_t digest;
} pl_ldpc_layered_plan_probe;
int pl_debug_ldpc_layered_plan_probe(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                     int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_rows,
                                     int32_t max_iter, int32_t early_stop, double normalization,
                                     int32_t kernel_override, int32_t bp_fpg, int32_t lms_global,
                                     pl_ldpc_layered_plan_probe* out);

/* The same for pl_ldpc_qc_plan_create (no kernel_override / bp_fpg: they do not
 * apply).  fpw: frames per wavefront; fpb: wavefronts per workgroup when z <= 64,
 * else 1, so a workgroup decodes fpw * fpb frames; dcap: the inputs of a check
 * the kernel instance keeps in registers (8, 16, 32; 0: the two-pass instance);
 * table_len / digest: the layer stream (per layer the block row, its degree and
 * its (block column, shift) pairs). */
typedef struct {
    int32_t kernel;      /* 11 or 12 (13 or 14 with PL_LDPC_QC_F32), as pl_plan_info.reserved */
    int32_t z, mb, nb, maxdc, dcap, mw, fpw, fpb, threads, lds_bytes, use_global;
    int64_t state_bytes;
    int64_t table_len;
    uint64_t digest;
} pl_ldpc_qc_plan_probe;
int pl_debug_ldpc_qc_plan_probe(int32_t mb, int32_t nb, int32_t z, const int32_t* shift, const int32_t* layer_order,
                                int32_t max_iter, int32_t early_stop, double normalization, int32_t lms_global,
                                pl_ldpc_qc_plan_probe* out);
/* The same with pl_ldpc_qc_plan_create's flags (PL_LDPC_QC_F32: kernel 13 or 14,
 * state_bytes and lds_bytes of the single-precision layout; the layer stream,
 * table_len and digest do not depend on the flags).  flags 0: the call above. */
int pl_debug_ldpc_qc_plan_probe_flags(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                      const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                      double normalization, int32_t lms_global, int32_t flags,
                                      pl_ldpc_qc_plan_probe* out);

/* The same for pl_ldpc_qc_fixed_plan_create: the fields of pl_ldpc_qc_plan_probe
 * with the plan's three parameters, and off_p, the byte offset of P behind the
 * check words (state_bytes = off_p + n rounded up to 16). */
typedef struct {
    int32_t kernel;      /* 15 or 16, as pl_plan_info.reserved */
    int32_t z, mb, nb, maxdc, dcap, mw, fpw, fpb, threads, lds_bytes, use_global;
    int32_t norm16, llr_max, msg_max, pad;
    int64_t state_bytes, off_p;
    int64_t table_len;
    uint64_t digest;
} pl_ldpc_qc_fixed_plan_probe;
int pl_debug_ldpc_qc_fixed_plan_probe(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                      const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                      int32_t norm16, int32_t llr_max, int32_t msg_max, int32_t lms_global,
                                      pl_ldpc_qc_fixed_plan_probe* out);

/* The same for pl_ldpc_qc_bp_plan_create: the fields of pl_ldpc_qc_plan_probe
 * (dcap and mw are 0: the rule keeps no input in registers and no check words)
 * with clip, and off_r, the byte offset of R behind P. */
typedef struct {
    int32_t kernel;      /* 17 or 18, as pl_plan_info.reserved */
    int32_t z, mb, nb, maxdc, dcap, mw, fpw, fpb, threads, lds_bytes, use_global;
    double clip;
    int64_t state_bytes, off_r;
    int64_t table_len;
    uint64_t digest;
} pl_ldpc_qc_bp_plan_probe;
int pl_debug_ldpc_qc_bp_plan_probe(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                   const int32_t* layer_order, int32_t max_iter, int32_t early_stop, double clip,
                                   int32_t lms_global, pl_ldpc_qc_bp_plan_probe* out);

/* ---- Monte-Carlo frame source (replaces src/channel/awgn.py:91-112 and the
 *      message/encode loop of benchmarks/ber_simulation.py:167-177) ---------- */

/* Random message bits, uint8 [batch][k], Philox4x32-10 keyed by (seed, global
 * frame index = frame_offset + b): identical for any sharding of the frames.
 * Counter, key and bit order: DESIGN.md section 4.4, "Stream contract". */
int pl_random_bits(uint64_t seed, int64_t frame_offset, int64_t batch, int32_t k, uint8_t* bits_dev,
                   void* stream);

/* Polar encoder (src/polar/encoder.py:63-95 without CRC): u[info] = msg,
 * u[frozen] = 0, x = u * F^{(x)n} (src/polar/utils.py:193-229).
 * msg_dev uint8 [batch][K] (bit 0 of each byte); codeword_dev uint8 [batch][N].
 * Index order: DESIGN.md section 4.4, "Stream contract".  Any polar plan encodes,
 * also one whose decoder geometry needs more LDS than the device has (list_size
 * 0 or 1 at N = 32768): such a plan is created for encoding only, and every
 * decode call on it returns PL_EUNSUPPORTED. */
int pl_polar_encode(const pl_plan* plan, const uint8_t* msg_dev, int64_t batch, uint8_t* codeword_dev,
                    void* stream);

/* BPSK (0 -> +1, 1 -> -1) + AWGN with sigma = sqrt(1/(2*10^(snr_db/10)))
 * (awgn.py:27-32, :47, :88), LLR = 2*y/sigma^2 (:75).  codeword_dev uint8 (bit 0 of each byte)
 * [batch][n] or NULL for the all-zero codeword.  Noise: Philox4x32-10 keyed by
 * (seed, frame_offset + b) + Box-Muller; statistically equivalent to the
 * reference's np.random.normal, not stream-identical.  Counter, key, uniforms
 * and the tested error bound: DESIGN.md section 4.4, "Stream contract". */
int pl_awgn_llr(const uint8_t* codeword_dev, int32_t n, int64_t batch, double snr_db, uint64_t seed,
                int64_t frame_offset, double* llr_dev, int64_t ld, void* stream);

/* Rayleigh fading + BPSK + AWGN (src/channel/fading.py:31-63): per bit
 * |h| (h complex Gaussian, E|h|^2 = 1), y = |h| s + N(0, sigma), LLR =
 * 2 y |h| / sigma^2, sigma = sqrt(1/(2*10^(snr_db/10))).  Philox keyed by (seed,
 * frame_offset + b, bit); statistically equivalent, not stream-identical.
 * Counters, salts and the tested error bound: DESIGN.md section 4.4, "Stream
 * contract". */
int pl_rayleigh_llr(const uint8_t* codeword_dev, int32_t n, int64_t batch, double snr_db, uint64_t seed,
                    int64_t frame_offset, double* llr_dev, int64_t ld, void* stream);

/* Binary symmetric channel (src/channel/bsc.py:33-49): out[b][j] = cw[b][j] ^
 * (u < crossover_prob), u uniform per bit; codeword_dev NULL = all-zero word.
 * Counter, key and u: DESIGN.md section 4.4, "Stream contract". */
int pl_bsc(const uint8_t* codeword_dev, int32_t n, int64_t batch, double crossover_prob, uint64_t seed,
           int64_t frame_offset, uint8_t* out_dev, int64_t ld, void* stream);

/* CRC append (src/polar/utils.py:86-125 crc_encode, the message layout of
 * PolarEncoder(use_crc=True), src/polar/encoder.py:74-78): for each row b of the
 * uint8 device matrix msg [batch][ld], writes the crc_len CRC bits of
 * msg[b][0:k_data] (MSB first) to msg[b][k_data : k_data+crc_len]. */
int pl_crc_append(uint8_t* msg_dev, int64_t ld, int64_t batch, int32_t k_data, int32_t crc_len, uint32_t poly,
                  void* stream);

/* GF(2) block encoding (LDPC valid codewords; replaces LDPCEncoder.encode,
 * src/ldpc/encoder.py:56-95, whose direct-solving fallback :97-187 emits
 * non-codewords for rank-deficient H): cw[b][j] = XOR_i msg[b][i] & G[i][j] for
 * a k x n generator G given bit-packed column-wise in device memory,
 * g_dev[w * n + j] bit i = G[32 w + i][j], w < ceil(k / 32).  msg [batch][ld_msg]
 * and cw [batch][ld_cw] are uint8 0/1 device matrices. */
int pl_gf2_encode(const uint32_t* g_dev, int32_t k, int32_t n, const uint8_t* msg_dev, int64_t ld_msg,
                  int64_t batch, uint8_t* cw_dev, int64_t ld_cw, void* stream);

/* ---- Quasi-cyclic LDPC encoder from the base matrix ------------------------------
 * Valid codewords of the code pl_ldpc_qc_plan_create decodes, computed from the
 * base matrix by cyclic shifts and XORs: no generator, H is never expanded.
 *   shift[i * nb + j] as for pl_ldpc_qc_plan_create: H[i z + r, j z + (r + s) % z]
 *   = 1, so check r of block row i reads sum_j c_j[(r + s_ij) % z] = 0, c_j the z
 *   bits of block column j.  kb = nb - mb >= 1; k = kb z, n = nb z.  The message
 *   occupies block columns 0 .. kb-1 and the code is systematic: cw[0:k] = msg.
 * Supported structure of the parity part Hp = shift[:, kb:]: a core of g block rows
 * followed by a lower-triangular extension, g == 0 or 3 <= g <= mb.
 *   core rows (i < g):
 *     - parity column kb has exactly three non-zero blocks, in rows 0, x and g-1
 *       with 0 < x < g-1, of shifts (a, b, a): the first and the last are equal;
 *     - parity column kb + t, t = 1 .. g-1, has exactly two non-zero blocks, in rows
 *       t-1 and t, both of shift 0;
 *     - core rows have no block in parity columns >= kb + g.
 *   extension rows (g <= i < mb):
 *     - shift[i][kb + i] >= 0 (any shift d_i), and no block to the right of it;
 *     - any blocks in earlier columns, message or parity.
 *   g == 0: a purely lower-triangular parity part; g == mb: the shape of IEEE
 *   802.11n / 802.16e; g == 4 with degree-1 extension columns: the 5G NR shape.
 *   g is unique: scanning the rows from the bottom while they satisfy the extension
 *   condition, g = 0 if all do, else the last failing row is g - 2.  Hp is then
 *   invertible: every message has exactly one codeword.
 * Encoding (sums over GF(2); thread r handles check r of the current block row):
 *   1. lambda_t[r] = sum_{j < kb} c_j[(r + s_tj) % z]        for each core row t
 *   2. p_0[(r + b) % z] = sum_{t < g} lambda_t[r]
 *   3. p_1[r] = lambda_0[r] + p_0[(r + a) % z]
 *   4. p_{t+1}[r] = lambda_t[r] + p_t[r] + [t == x] p_0[(r + b) % z],  1 <= t <= g-2
 *   5. p_i[(r + d_i) % z] = sum_{j < kb + i} c_j[(r + s_ij) % z]  for each extension
 *      row i, in order (p_i: the bits of block column kb + i)
 * PL_EINVAL for mb, nb or z < 1, kb < 1, nb z beyond int32, a shift outside
 * -1 .. z-1; PL_EUNSUPPORTED for z > 1024, a parity part outside the structure (the
 * message names the first rule violated) and a workgroup's LDS need above 160 KB.
 * Every argument check runs before the first device call.  The encoder belongs
 * to the device current at creation, as a plan does.
 * One thread per check of the current block row; for z <= 64, 64 / z frames share
 * a wavefront and up to four wavefronts a workgroup, else one workgroup of z
 * threads (rounded up to 64) encodes a frame.  The codeword and the lambda_t live
 * in LDS, one byte per bit, (nb + g) z bytes a frame (rounded up to 16). */
typedef struct pl_qc_encoder pl_qc_encoder;
int pl_ldpc_qc_encoder_create(int32_t mb, int32_t nb, int32_t z, const int32_t* shift /* [mb*nb] row-major */,
                              pl_qc_encoder** out);
/* msg_dev uint8 [batch][ld_msg] device, ld_msg >= k, bit 0 of each byte is the
 * message bit; cw_dev uint8 [batch][ld_cw] device, ld_cw >= n: the n codeword
 * bytes (0 / 1) of each row are written, bytes beyond n are left alone.
 * Asynchronous on `stream`; batch == 0 launches nothing.  PL_EINVAL for a NULL
 * pointer, ld_msg < k, ld_cw < n, batch < 0, or a current device other than the
 * encoder's. */
int pl_ldpc_qc_encode(const pl_qc_encoder* enc, const uint8_t* msg_dev, int64_t ld_msg, int64_t batch,
                      uint8_t* cw_dev, int64_t ld_cw, void* stream);
int pl_ldpc_qc_encoder_destroy(pl_qc_encoder* enc);
/* What the planner decides for an encoder, with no device call (pl_ldpc_qc_encoder_create's checks,
 * codes and messages).  The stream the kernel walks, int32 words:
 *   g, x, a, b                       (x, a, b are 0 when g == 0)
 *   per core row t = 0 .. g-1:       d, then d (block column, shift) pairs: its message blocks, ascending
 *   per extension row i = g .. mb-1: d_i, the sync flag, d, then d (block column, shift) pairs: its blocks
 *                                    left of the diagonal, ascending block column
 * sync flag: 1 iff the row reads a parity block column written since the last synchronisation point.
 * n_sync: the synchronisation points the stream asks for, the one behind p_0 (g > 0) plus the flagged
 * extension rows (those around loading the message and storing the codeword are not counted). */
typedef struct {
    int32_t g, x, a, b;
    int32_t subwave;     /* 1: z <= 64, frames share wavefronts                         */
    int32_t fpw, fpb;    /* frames per wavefront, wavefronts per workgroup              */
    int32_t threads, lds_bytes, n_sync;
    int64_t table_len;   /* int32 words of the stream                                   */
    uint64_t digest;     /* 64-bit FNV-1a over the stream's bytes                       */
} pl_qc_encoder_probe;
int pl_debug_ldpc_qc_encoder_probe(int32_t mb, int32_t nb, int32_t z, const int32_t* shift, pl_qc_encoder_probe* out);
/* Test hook, diagnostic build only (the product library returns PL_EUNSUPPORTED):
 * pl_debug_set_plan_device for an encoder. */
int pl_debug_set_qc_encoder_device(pl_qc_encoder* enc, int32_t device);

/* ---- Rate matching for quasi-cyclic LDPC codes: puncture, shorten, repeat ---------
 * Which bits of a codeword of the code (mb, nb, z) are transmitted, and how their
 * LLRs come back to codeword positions.  This comment is the definition; the
 * kernels (ldpc_qc_ratematch.hip), ldpc.QCRateMatcher and the harness cite it.
 * Parameters and conditions (n = nb z, kb = nb - mb >= 1, k = kb z):
 *   punctured  leading block columns never transmitted; P = punctured z,
 *              0 <= punctured < kb
 *   fillers    F: the last F message bits (codeword positions k-F .. k-1) are
 *              known zeros and never transmitted; 0 <= F <= k - P
 *   ncb        the circular buffer is codeword positions P .. P+ncb-1;
 *              k - P <= ncb <= n - P; a negative ncb asks for the default n - P
 *   start      where reading begins in the buffer, 0 <= start < ncb; any value,
 *              not only multiples of z
 *   E >= 1     transmitted bits per frame
 *   M = ncb - F >= 1   the buffer without its fillers
 * Selection: t = 0, j = 0; while t < E: b = (start + j) mod ncb; if buffer
 *   position b is no filler (not k-P-F <= b < k-P): e[t] = c[P + b], t += 1;
 *   j += 1.
 * Closed form (what the kernels compute; there is no table):
 *   compact index of a non-filler buffer position b: c(b) = b for b < k-P-F,
 *   else b - F; c0 = c(start) if start is no filler, else (k-P-F) mod M;
 *   transmitted bit t is compact index (c0 + t) mod M; the position of compact
 *   index c receives t = r, r+M, r+2M, ... < E with r = (c - c0) mod M.
 *   hi: the highest transmitted codeword position; max_reps = ceil(E / M).
 * Recovery of out[b][0:n_out], element type T (fp64 or fp32), from llr[b][0:E]
 * (fp64 or fp32); hi < n_out <= n:
 *   a transmitted position gets its terms, each converted to T, summed left to
 *   right in ascending t starting from the first term (a single term is a copy:
 *   -0.0 stays -0.0); a filler gets +filler_llr (the sign that decodes to bit 0:
 *   pl_awgn_llr maps 0 -> +1), converted to T; every other position +0.0.
 *   PL_RM_ACCUMULATE (soft combining of retransmissions): out holds an earlier
 *   recovery; transmitted positions become out[pos] + s, s the sum above, and
 *   every other position keeps its value.
 * pl_ldpc_rate_match_check fills the derived fields from the parameters;
 * PL_EINVAL naming the first condition violated, in the order above.  It makes no
 * device call.  The two kernels take the struct by value: there is no device
 * object.  pl_ldpc_rate_match and pl_ldpc_rate_recover derive the fields again
 * themselves, so a caller's derived fields are never trusted. */
typedef struct {
    int32_t mb, nb, z;                           /* the code                                   */
    int32_t punctured, fillers, ncb, start, E;   /* ncb < 0 on input: n - P                    */
    int32_t n, k, P, M, c0, hi, max_reps;        /* derived by pl_ldpc_rate_match_check        */
} pl_rate_match;
int pl_ldpc_rate_match_check(pl_rate_match* rm);
/* The same from plain arguments (the planner's window for tests, as pl_debug_ldpc_qc_encoder_probe). */
int pl_debug_rate_match_probe(int32_t mb, int32_t nb, int32_t z, int32_t punctured, int32_t fillers, int32_t ncb,
                              int32_t start, int32_t E, pl_rate_match* out);
/* e[b][t] = cw[b][position of t], t < E: cw_dev uint8 [batch][ld_cw], ld_cw >= n,
 * bytes copied as they are; e_dev uint8 [batch][ld_e], ld_e >= E, bytes beyond E
 * are left alone.  Asynchronous on `stream`; batch == 0 launches nothing.
 * PL_EINVAL for what pl_ldpc_rate_match_check refuses, a NULL pointer, batch < 0
 * and a short pitch; every check runs before the first device call. */
int pl_ldpc_rate_match(const pl_rate_match* rm, const uint8_t* cw_dev, int64_t ld_cw, int64_t batch, uint8_t* e_dev,
                       int64_t ld_e, void* stream);
#define PL_RM_LLR_F32 1    /* llr_dev is float (else double)                           */
#define PL_RM_OUT_F32 2    /* out_dev is float (else double)                           */
#define PL_RM_ACCUMULATE 4 /* add to the recovery out_dev already holds                */
/* Recovery as defined above: llr_dev [batch][ld_llr], ld_llr >= E; out_dev
 * [batch][ld_out], ld_out >= n_out, elements beyond n_out are left alone; pitches
 * in elements.  Asynchronous on `stream`; batch == 0 launches nothing.  PL_EINVAL
 * as pl_ldpc_rate_match, and for n_out <= hi, n_out > n, unknown flag bits and a
 * pointer that is not aligned to its element type.
 * Both kernels cut each row at the 16-byte boundaries of its output addresses and
 * store whole pieces 16 bytes wide, whatever the pointer and the pitch. */
int pl_ldpc_rate_recover(const pl_rate_match* rm, const void* llr_dev, int64_t ld_llr, int64_t batch, void* out_dev,
                         int64_t ld_out, int32_t n_out, double filler_llr, int32_t flags, void* stream);

/* ---- Rate matching for polar codes: puncture, shorten, repeat -----------------------
 * Which of the N bits of a codeword x = u F^(x)n (natural order, pl_polar_encode) are
 * transmitted, and how E received LLRs come back to the N decoder inputs.  This
 * comment is the definition; the kernels (polar_ratematch.hip),
 * polar.PolarRateMatcher and the harness cite it.
 * Parameters and conditions; a violation is PL_EINVAL naming the first one violated,
 * in this order:
 *   1. N is a power of two in 2 .. 32768
 *   2. 1 <= E <= 2^30
 *   3. mode is PL_PRM_PUNCTURE or PL_PRM_SHORTEN (checked always, used when E < N)
 *   4. nsub is a power of two in 1 .. 32, and nsub <= N
 *   5. perm[0:nsub] is a permutation of 0 .. nsub-1
 * Derived: S = N / nsub, U = max(N - E, 0), max_reps = ceil(E / N), inv the inverse
 * of perm (entries nsub .. 31 of inv are 0), pad = 0.
 * Interleaved sequence: y[m] = x[J(m)], J(m) = perm[m / S] S + m mod S, m = 0 .. N-1:
 *   the N positions in nsub sub-blocks of S, the sub-blocks permuted.  The caller
 *   supplies perm; no standard's table is reproduced.  nsub = 1 (identity) is
 *   plain block puncturing and shortening.
 * Selection e[t], t = 0 .. E-1:
 *   E >= N           e[t] = y[t mod N]      (repetition)
 *   E < N, puncture  e[t] = y[t + N - E]    (the first U of y are not sent)
 *   E < N, shorten   e[t] = y[t]            (the last U of y are not sent; they are 0)
 * Recovery of out[b][0:N] (fp64) from llr[b][0:E] (fp64, or fp32 with
 * PL_PRM_LLR_F32).  Position i has interleaved index m = inv[i / S] S + i mod S.
 *   E >= N    the terms t = m, m+N, ... < E, each converted to fp64, summed left to
 *             right in ascending t starting from the first term (a single term is a
 *             copy: -0.0 stays -0.0)
 *   puncture  m < N - E: +0.0; else llr[m - (N - E)]
 *   shorten   m < E: llr[m]; else +known_llr (the sign that decodes to bit 0:
 *             pl_awgn_llr maps 0 -> +1); finite, so that the frame stays on the
 *             decoders' fast path
 *   PL_PRM_ACCUMULATE (Chase combining of retransmissions, possibly through another
 *             matcher of the same N): a transmitted position becomes out + s, s the
 *             value above; every other position keeps its value.
 * The output is fp64 only: no polar decoder reads fp32.
 * Frozen set: a shortened code is one only if the untransmitted x_i are zero for
 * every message.  x_i = XOR of u_j over j & i == i, so that holds exactly when every
 * u_j with j a superset of an untransmitted position is frozen:
 * pl_polar_rate_match_forced gives that minimal set (all zero unless shorten and
 * E < N).  THE CALLER'S OBLIGATION: the frozen mask of the plan that encodes and
 * decodes must contain it.  polar.construct_rate_matched builds such a set.
 * A superset of i is >= i, so when the last U of y are the U highest positions the set
 * is those U indices alone; every lower position a permutation moves into that tail
 * adds its supersets (the reversal at E = N/2 + 1 forces all N).  With shortening,
 * choose perm so that the highest sub-blocks stay last.
 * pl_polar_rate_match_check fills the derived fields and makes no device call.  The
 * kernels take the parameters by value: there is no device object.
 * pl_polar_rate_match and pl_polar_rate_recover derive the fields again themselves,
 * so a caller's derived fields are never trusted. */
#define PL_PRM_PUNCTURE 0
#define PL_PRM_SHORTEN 1
typedef struct {
    int32_t N, E, mode, nsub;    /* parameters                                             */
    uint8_t perm[32];            /* sub-block permutation, entries 0 .. nsub-1 used        */
    int32_t S, U, max_reps, pad; /* derived: S = N / nsub, U = max(N - E, 0), ceil(E / N)  */
    uint8_t inv[32];             /* derived: inverse permutation                           */
} pl_polar_rm;
int pl_polar_rate_match_check(pl_polar_rm* rm);
/* The same from plain arguments (the check's window for tests, as pl_debug_rate_match_probe);
 * perm: nsub bytes (may be NULL when nsub == 1: the identity). */
int pl_debug_polar_rate_match_probe(int32_t N, int32_t E, int32_t mode, int32_t nsub, const uint8_t* perm,
                                    pl_polar_rm* out);
/* mask_host uint8 [N], host memory: 1 where u_j must be frozen (see "Frozen set" above), else 0.
 * OR-zeta transform over supersets, N log N; no device call. */
int pl_polar_rate_match_forced(const pl_polar_rm* rm, uint8_t* mask_host);
/* e[b][t] as defined above, t < E: cw_dev uint8 [batch][ld_cw], ld_cw >= N, bytes copied as
 * they are; e_dev uint8 [batch][ld_e], ld_e >= E, bytes beyond E are left alone.
 * Asynchronous on `stream`; batch == 0 launches nothing.  PL_EINVAL for what
 * pl_polar_rate_match_check refuses, a NULL pointer, batch < 0 and a short pitch; every
 * check runs before the first device call. */
int pl_polar_rate_match(const pl_polar_rm* rm, const uint8_t* cw_dev, int64_t ld_cw, int64_t batch, uint8_t* e_dev,
                        int64_t ld_e, void* stream);
#define PL_PRM_LLR_F32 1    /* llr_dev is float (else double)                          */
#define PL_PRM_ACCUMULATE 4 /* add to the recovery out_dev already holds               */
/* Recovery as defined above: llr_dev [batch][ld_llr], ld_llr >= E; out_dev double
 * [batch][ld_out], ld_out >= N, elements beyond N are left alone; pitches in elements.
 * known_llr must be finite and > 0.  Asynchronous on `stream`; batch == 0 launches
 * nothing.  PL_EINVAL as pl_polar_rate_match, and for unknown flag bits, a known_llr
 * that is not finite and positive, and a pointer not aligned to its element type.
 * Both kernels cut each row at the 16-byte boundaries of its output addresses and store
 * whole pieces 16 bytes wide, whatever the pointer and the pitch. */
int pl_polar_rate_recover(const pl_polar_rm* rm, const void* llr_dev, int64_t ld_llr, int64_t batch, double* out_dev,
                          int64_t ld_out, double known_llr, int32_t flags, void* stream);

/* ---- Gray-mapped square QAM: modulator, complex AWGN, max-log soft demapper ----------
 * What crosses the channel between a rate matcher's E transmitted bits and the E LLRs it
 * takes back, when it is not one BPSK symbol per bit (pl_awgn_llr).  This comment is the
 * definition; the kernels (qam.hip), channel.QAMModem and the harness cite it.  The
 * mapping is built here from the binary-reflected Gray code; no standard's table is
 * reproduced.
 * Parameters and conditions; a violation is PL_EINVAL naming the first one violated, in
 * this order:
 *   1. m, bits per symbol, is 2, 4, 6 or 8 (QPSK, 16-, 64-, 256-QAM)
 *   2. 1 <= E <= 2^30, transmitted bits per frame
 * Derived: h = m / 2 bits per axis; S = ceil(E / m) symbols per frame; bits E .. S m - 1
 * of the last symbol are zeros at the modulator and get no LLR.
 * Bit to axis: bit i (0 .. m-1) of symbol s is e[s m + i] & 1.  Even i go to the I axis,
 *   odd i to the Q axis; the bit's position on its axis is p = i / 2, p = 0 first.
 * Axis mapping (Gray): from the axis bits b_0 .. b_(h-1): c_0 = b_0, c_p = c_(p-1) ^ b_p,
 *   idx = sum c_p 2^(h-1-p), integer level a = (2^h - 1) - 2 idx.  All-zero bits give the
 *   largest positive level (consistent with BPSK's 0 -> +1); neighbouring levels differ in
 *   exactly one bit.
 * Scale: D = 2 (4^h - 1) / 3, an exact integer (2, 10, 42, 170); scale = 1.0 / sqrt((double)D);
 *   the axis value is x = (double)a * scale, one multiplication.  The constellation has unit
 *   mean energy.
 * Symbol layout: fp64, I and Q interleaved, [batch][ld] with ld >= 2 S: element 2 s is I
 *   and element 2 s + 1 is Q of symbol s.
 * Channel: y = x + sigma z per axis, sigma = sqrt(1 / (2 10^(snr_db / 10))) computed as
 *   pl_awgn_llr computes it; snr_db is Es/N0 per QAM symbol.  The normals are the
 *   Box-Muller pair of the stream contract (pl_awgn_llr's: two 53-bit uniforms of one
 *   Philox4x32-10 call) at counter (s, f_lo, f_hi, 0x9A3A9A3A), f = frame_offset + b, key
 *   as the AWGN source (seed_lo ^ 0x5bd1e995, seed_hi): z0 -> I, z1 -> Q of symbol s.  A
 *   frame's values depend on (seed, frame_offset + b, s) only.
 * Demapper (max-log), exact fp64, every step one IEEE operation, no contraction.  For an
 *   axis value r and axis bit p: t = r - x_a, d_a = t * t for each of the 2^h levels; d0 =
 *   min d_a over the levels whose bit p is 0, d1 over those whose bit p is 1; s2 = sigma *
 *   sigma, w = 1.0 / (2.0 * s2) (on the host); llr = (d1 - d0) * w.  Positive decides 0.
 *   PL_QAM_LLR_F32: the fp64 result rounded once to fp32, to nearest even.  A NaN r, or
 *   an r so large that every d_a overflows, gives NaN (payload unspecified).
 * pl_qam_check makes no device call; S_out and scale_out may be NULL.  There is no device
 * object: the kernels take the parameters by value, and each entry point checks them
 * again itself. */
int pl_qam_check(int32_t m, int64_t E, int64_t* S_out, double* scale_out);
/* x[b][2 s], x[b][2 s + 1] = the clean symbol s of e[b][0:E]: e_dev uint8 [batch][ld_e], ld_e >= E
 * (bit 0 of each byte); x_dev double [batch][ld_x], ld_x >= 2 S, elements beyond 2 S are left
 * alone.  Asynchronous on `stream`; batch == 0 launches nothing.  PL_EINVAL for what
 * pl_qam_check refuses, batch < 0, a NULL pointer with batch > 0, a pointer that is not
 * aligned to its element type and a short pitch; every check runs before the first device
 * call. */
int pl_qam_modulate(int32_t m, int64_t E, int64_t batch, const uint8_t* e_dev, int64_t ld_e, double* x_dev,
                    int64_t ld_x, void* stream);
/* y = x + sigma z as defined above, mapped and disturbed in one pass: y_dev double
 * [batch][ld_y], ld_y >= 2 S.  e_dev == NULL: all-zero bits (ld_e is then not used).
 * PL_EINVAL as pl_qam_modulate (y_dev NULL with batch > 0), and for a snr_db that is not
 * finite. */
int pl_qam_awgn(int32_t m, int64_t E, int64_t batch, const uint8_t* e_dev, int64_t ld_e, double snr_db, uint64_t seed,
                int64_t frame_offset, double* y_dev, int64_t ld_y, void* stream);
#define PL_QAM_LLR_F32 1 /* llr_dev is float (else double) */
/* llr[b][t], t < E, of the received y_dev double [batch][ld_y], ld_y >= 2 S: llr_dev
 * [batch][ld_llr], ld_llr >= E, elements beyond E are left alone; pitches in elements.
 * PL_EINVAL as pl_qam_awgn, and for unknown flag bits.  The kernel cuts each row at the
 * 16-byte boundaries of its output addresses and stores whole pieces 16 bytes wide,
 * whatever the pointer and the pitch. */
int pl_qam_demap(int32_t m, int64_t E, int64_t batch, const double* y_dev, int64_t ld_y, double snr_db, void* llr_dev,
                 int64_t ld_llr, int32_t flags, void* stream);

/* ---- Block Rayleigh fading for the QAM symbols, and the demapper with channel state ----
 * A channel whose gain is correlated over neighbouring symbols, which is what the bit
 * interleaver is for, with perfect channel state at the receiver.  This comment is the
 * definition; the kernels (qam.hip), channel.QAMModem and the harness cite it.  It builds on
 * the block at pl_qam_check: its m, E, h bits per axis, S, scale, symbol layout, sigma and
 * noise stream.
 * Parameters and conditions; a violation is PL_EINVAL naming the first one violated, in
 * this order:
 *   1., 2. pl_qam_check's two, in its order
 *   3. 1 <= coherence <= 2^30: the coherence length Lc, in symbols
 * Derived: the fading block of symbol s is q = s / Lc (integer division); Q = ceil(S / Lc)
 * blocks per frame.  Lc >= S: one coefficient per frame (quasi-static); Lc = 1: one per
 * symbol (fast fading).
 * Coefficients: fp64, real and imaginary part interleaved, [batch][ld_h], ld_h >= 2 Q:
 *   element 2 q is Re and element 2 q + 1 is Im of block q.  hr = g0 * C, hi = g1 * C with
 *   C = 0x1.6a09e667f3bcdp-1 (the double nearest 1 / sqrt(2)) and (g0, g1) the Box-Muller
 *   pair of the stream contract at counter (q, f_lo, f_hi, 0xFADE9A3A), f = frame_offset + b,
 *   key as the AWGN source.  A coefficient depends on (seed, f, q) only: not on Lc, m, E or
 *   the batch.  E |h|^2 = 1.
 * Channel: with the clean symbol (xI, xQ), each step one IEEE operation, in this order, no
 *   contraction:
 *     yI = (hr * xI - hi * xQ) + sigma * z0
 *     yQ = (hr * xQ + hi * xI) + sigma * z1
 *   (z0, z1) is exactly pl_qam_awgn's pair of symbol s (salt 0x9A3A9A3A): with equal seeds
 *   the noise is pl_qam_awgn's noise.
 * Demapper with channel state (max-log), exact fp64, every step one IEEE operation.  Per
 *   symbol, with its block's (hr, hi):
 *     g  = hr * hr + hi * hi
 *     uI = hr * yI + hi * yQ          uQ = hr * yQ - hi * yI
 *     rI = uI / g                     rQ = uQ / g
 *     wg = w * g                      (w as pl_qam_demap: 1.0 / (2.0 * (sigma * sigma)), on the host)
 *   and the LLR of axis bit p is (d1 - d0) * wg with d_a = (r - x_a) * (r - x_a) and the
 *   minima as in pl_qam_demap.  The matched filter u = conj(h) y leaves r = y / h with noise
 *   of variance sigma^2 / g per axis: the thresholds stay where they are and the weight
 *   scales by g.  g == 0.0 (a zero or underflowing coefficient; u1 = 1 makes the Box-Muller
 *   radius exactly 0, so the channel can produce it): every LLR of the symbol is +0.0, an
 *   erased symbol.  Every other special (NaN, inf, a g so small that u / g overflows) gives
 *   what the operations give; a NaN's payload is unspecified.  PL_QAM_LLR_F32: the fp64
 *   result rounded once to fp32.
 *   Property: with h = (1.0, 0.0) and finite y the result equals pl_qam_demap's bit for bit
 *   (g = 1, u = y up to the sign of a zero, r = u, wg = w).
 * pl_qam_fading_check makes no device call; S_out and Q_out may be NULL. */
int pl_qam_fading_check(int32_t m, int64_t E, int64_t coherence, int64_t* S_out, int64_t* Q_out);
/* y = h x + sigma z as defined above, mapped, faded and disturbed in one pass: y_dev double
 * [batch][ld_y], ld_y >= 2 S; h_dev double [batch][ld_h], ld_h >= 2 Q, receives the
 * coefficients; elements beyond 2 S and 2 Q of a row are left alone; y_dev and h_dev must not
 * overlap.  e_dev == NULL: all-zero bits (ld_e is then not used).  Asynchronous on `stream`;
 * batch == 0 launches nothing.  PL_EINVAL as pl_qam_awgn, and for what pl_qam_fading_check
 * refuses, h_dev NULL with batch > 0, h_dev not 8-byte aligned and ld_h < 2 Q; every check
 * runs before the first device call. */
int pl_qam_rayleigh(int32_t m, int64_t E, int64_t coherence, int64_t batch, const uint8_t* e_dev, int64_t ld_e,
                    double snr_db, uint64_t seed, int64_t frame_offset, double* y_dev, int64_t ld_y,
                    double* h_dev, int64_t ld_h, void* stream);
/* llr[b][t], t < E, of the received y_dev and the coefficients h_dev (layouts as above):
 * llr_dev [batch][ld_llr], ld_llr >= E, float with PL_QAM_LLR_F32, else double; elements
 * beyond E are left alone.  PL_EINVAL as pl_qam_demap and as pl_qam_rayleigh for coherence
 * and h_dev.  The kernel stores whole 16-byte pieces as pl_qam_demap's does, whatever the
 * pointer and the pitch. */
int pl_qam_demap_csi(int32_t m, int64_t E, int64_t coherence, int64_t batch, const double* y_dev, int64_t ld_y,
                     const double* h_dev, int64_t ld_h, double snr_db, void* llr_dev, int64_t ld_llr,
                     int32_t flags, void* stream);

/* ---- The exact log-MAP soft demapper ---------------------------------------------------
 * Max-log keeps one nearest level per bit hypothesis; the a-posteriori LLR of a bit sums
 * over all levels: log sum_{bit = 0} e^(-W d_a) - log sum_{bit = 1} e^(-W d_a).  An LLR of
 * this kind predicts its own hard-decision error probability, 1 / (1 + e^|L|), which the
 * magnitude-consuming stages behind the demapper (normalised and fixed-point min-sum, soft
 * combining) rely on.  This comment is the definition; the kernel (qam.hip), channel.QAMModem
 * and the harness cite it.  It builds on the blocks at pl_qam_check and pl_qam_fading_check:
 * their m, E, h, S, scale, levels x_a, symbol layout, sigma, w, g, r, wg.
 * For an axis value r, a weight W and an axis bit p, exact fp64, every step one IEEE
 * operation, no contraction:
 *   W is w in pl_qam_demap_logmap and wg in pl_qam_demap_csi_logmap, where r = u / g exactly
 *   as in pl_qam_demap_csi.
 *   d_a = (r - x_a) * (r - x_a) for each of the 2^h levels, as in max-log.
 *   For each hypothesis v in {0, 1}: D_v = min d_a over the levels whose bit p is v (max-log's
 *   d0 and d1).  T_v starts at 0.0; over the levels of that set in ascending level index
 *   (index 0 is the largest level: idx of the axis mapping):
 *     q = (D_v - d_a) * W
 *     e = expm1(q) + 1.0
 *     T_v = T_v + e
 *   c_v = log1p(T_v - 1.0)
 *   llr = ((D_1 - D_0) * W) + (c_0 - c_1).  Positive decides 0.
 * expm1 and log1p are the functions as glibc 2.35's dbl-64 libm computes them (the fdlibm
 * algorithms with glibc's evaluation order; csrc/libm_exact.hpp restates them in plain IEEE
 * operations), extended to expm1(-inf) = -1.0, expm1(NaN) = NaN and log1p(NaN) = NaN.  The sum
 * is written around the minimum, so every exponent is <= 0 and nothing overflows; the
 * form expm1 + 1 and log1p(T - 1) is chosen because those two functions are the ones whose
 * bit-exact restatement the library already carries.
 * Consequences:
 *   T_v >= 1.0 always: the minimum itself contributes expm1(+-0) + 1.0 = 1.0, and every other
 *     term is in [0, 1].  The log1p argument is therefore in [0, 2^(h-1) - 1].
 *   g == 0.0 in pl_qam_demap_csi_logmap: every LLR of the symbol is +0.0, as in max-log.
 *   An LLR that max-log gives as NaN (a NaN r, every d_a overflowing) is NaN here.  Every other
 *     special value gives what the operations give: a d_a that alone overflows has q = -inf
 *     and contributes e = 0.0.  A NaN's payload is unspecified.
 *   QPSK, and any r, W for which every q of a non-minimal level is <= -56 ln 2 (glibc's expm1
 *     returns -1.0 from the double 0x1.3687ap+5 on, in magnitude): T_v = 1.0, c_v = +0.0 and
 *     the result equals max-log's as a number.  It is bit for bit equal, except that max-log's
 *     -0.0 becomes +0.0 (-0.0 + (+0.0)).
 *   With h = (1.0, 0.0) and finite y, pl_qam_demap_csi_logmap equals pl_qam_demap_logmap bit
 *     for bit, as the max-log pair does.
 *   PL_QAM_LLR_F32: the fp64 result rounded once to fp32.
 * A kernel may skip a level whose q is <= -0x1.3687ap+5: its e is 0.0 and T_v + 0.0 is T_v. */
/* pl_qam_demap with the exact log-MAP LLR defined above: its arguments, its refusals, its
 * stores.  Asynchronous on `stream`; batch == 0 launches nothing; every check runs before
 * the first device call. */
int pl_qam_demap_logmap(int32_t m, int64_t E, int64_t batch, const double* y_dev, int64_t ld_y, double snr_db,
                        void* llr_dev, int64_t ld_llr, int32_t flags, void* stream);
/* pl_qam_demap_csi likewise. */
int pl_qam_demap_csi_logmap(int32_t m, int64_t E, int64_t coherence, int64_t batch, const double* y_dev, int64_t ld_y,
                            const double* h_dev, int64_t ld_h, double snr_db, void* llr_dev, int64_t ld_llr,
                            int32_t flags, void* stream);

/* ---- Bit interleaver between rate matching and the QAM modem ---------------------------
 * The m bit positions of a QAM symbol are unequally reliable and a rate matcher hands over
 * runs of consecutive code bits; the interleaver spreads such a run over the positions.
 * This comment is the definition; the kernels (interleave.hip), channel.BitInterleaver and
 * the harness cite it.  It is build-defined and given as a procedure; no standard's text
 * or table is reproduced.
 * An interleaver is (kind, rows, E).  It maps e[0:E) to f[0:E); its inverse acts on LLRs.
 * Conditions; a violation is PL_EINVAL naming the first one violated, in this order:
 *   1. kind is PL_ILV_RECT or PL_ILV_TRI
 *   2. 1 <= E <= 2^30
 *   3. PL_ILV_RECT: 1 <= rows <= 64.  PL_ILV_TRI: rows == 0.
 * PL_ILV_RECT: C = ceil(E / rows).  Write e row by row into a rows x C array: cell (r, c)
 *   holds index k = r C + c; cells with k >= E are empty.  Read column by column, c outer
 *   and r inner, skipping empty cells.  With rows = m and E a multiple of m, bit r of
 *   symbol s is e[r C + s].  E need not be a multiple of rows; E < rows is legal.
 * PL_ILV_TRI: T is the smallest integer with T (T + 1) / 2 >= E.  Row i (0 .. T-1) has
 *   T - i cells and starts at index st(i) = i T - i (i - 1) / 2.  Write e row by row; cells
 *   with index >= E are empty (always at the tail; several trailing rows may be empty).
 *   Read column by column: column j has rows 0 .. T-1-j; skip empty cells.
 * pos(k) is the output position of input k: f[pos(k)] = e[k].  The deinterleaver is
 *   e_llr[k] = f_llr[pos(k)].
 * The device computes pos in closed form (csrc/interleave_check.hpp): no table and no device
 * object; the kernels take the parameters by value, and each entry point checks them again
 * itself.  pl_interleave_check and pl_interleave_index make no device call. */
#define PL_ILV_RECT 0
#define PL_ILV_TRI 1
/* *dim_out (may be NULL) receives C (PL_ILV_RECT) or T (PL_ILV_TRI). */
int pl_interleave_check(int32_t kind, int32_t rows, int64_t E, int64_t* dim_out);
/* *pos_out = pos(k), by the code the kernels run.  PL_EINVAL for what pl_interleave_check
 * refuses, for k outside 0 .. E-1 and for a NULL pos_out. */
int pl_interleave_index(int32_t kind, int32_t rows, int64_t E, int64_t k, int64_t* pos_out);
/* The largest E whose frames of elem_size bytes (1, 4, 8) the kernels permute in LDS; longer
 * frames are permuted directly in global memory.  0 for another elem_size. */
int64_t pl_interleave_lds_max_e(int32_t elem_size);
/* f[b][pos(k)] = e[b][k], bytes copied whole: e_dev uint8 [batch][ld_e], f_dev uint8
 * [batch][ld_f], pitches >= E; bytes beyond E are left alone.  Asynchronous on `stream`;
 * batch == 0 launches nothing.  PL_EINVAL for what pl_interleave_check refuses, batch < 0, a
 * NULL pointer with batch > 0, a short pitch, and e_dev and f_dev overlapping; every check
 * runs before the first device call. */
int pl_bit_interleave(int32_t kind, int32_t rows, int64_t E, int64_t batch, const uint8_t* e_dev, int64_t ld_e,
                      uint8_t* f_dev, int64_t ld_f, void* stream);
#define PL_ILV_LLR_F32 1 /* f_dev and e_dev are float (else double) */
/* e[b][k] = f[b][pos(k)]: f_dev [batch][ld_f], e_dev [batch][ld_e], both double, or both
 * float with PL_ILV_LLR_F32; pitches in elements, >= E; elements beyond E are left alone.
 * Values are copied bit for bit (NaN payloads, -0.0).  PL_EINVAL as pl_bit_interleave, and for
 * unknown flag bits and a pointer that is not aligned to its element type. */
int pl_llr_deinterleave(int32_t kind, int32_t rows, int64_t E, int64_t batch, const void* f_dev, int64_t ld_f,
                        void* e_dev, int64_t ld_e, int32_t flags, void* stream);

/* Error counting (benchmarks/ber_simulation.py:180-189):
 * counts_dev[0] += bit errors, [1] += frame errors, [2] += frames, over the
 * first `width` entries of each row.  counts_dev int64[3], device. */
int pl_count_errors(const uint8_t* ref_dev, int64_t ld_ref, const uint8_t* dec_dev, int64_t ld_dec,
                    int32_t width, int64_t batch, int64_t* counts_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POLARLDPC_H */

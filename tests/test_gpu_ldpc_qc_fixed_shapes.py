"""QCFixedMSDecoder (ldpc_qc_fixed.hip on ldpc_qc_frame.hpp) against the NumPy
integer restatement (tests/qc_fixed_ref.py) at the lifting sizes, planner edges,
check-word packing edges and rate-matched frames of tests/qc_fixed_shapes.py.
Bar: hard decisions, iteration counts and int8 posteriors array_equal.  The
builders of qc_fixed_shapes.py assert every condition on the inputs on the
restatement before the device is asked; tests/test_ldpc_qc_fixed_shapes_host.py
holds the geometry tables against the planner and states what they reach."""
import numpy as np
import pytest
import torch

import qc_fixed_shapes as S

pytestmark = pytest.mark.gpu


def _dec(base, Z, p, max_iter, early_stop=True, layer_order=None):
    return S.L().QCFixedMSDecoder(np.array(base), Z, max_iter=max_iter, normalization=p["norm16"] / 16.0,
                                  early_stop=early_stop, layer_order=layer_order, llr_scale=p["llr_scale"],
                                  llr_max=p["llr_max"], msg_max=p["msg_max"])


def _same(got, want, B=None):
    bits, its, post = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    want = [w[:B] for w in want]
    assert np.array_equal(bits, want[0])
    assert np.array_equal(its, want[1])
    assert post.dtype == np.int8 and want[2].dtype == np.int8 and np.array_equal(post, want[2])


def _soft(dec, llr):
    return dec.decode_batch(torch.from_numpy(np.array(llr)).cuda(), return_iterations=True, return_llr=True)


def _holds(dec, g):
    """The plan made is the row of the table (the host file holds the rest of the row against the planner)."""
    info = dec.plan.info
    assert info.reserved == g["kernel"] and info.fused_top == g["dcap"]
    assert info.frames_per_block == g["fpw"] * g["fpb"] and info.lds_bytes == g["lds"]
    assert dec.plan.workspace_bytes(1) == (g["state"] if g["use_global"] else 0)


# ---- a. lifting sizes ------------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("Z", sorted(S.LIFT))
def test_lifting_sizes(gpu, Z, early_stop):
    """Z = 2, 3: 32 and 21 frames per wavefront, the stop mask shifted by up to 62 bits; 32: the second
    frame's mask in bits 32..63; 33, 63: fpw == 1 with idle lanes of lane / z == 1; 65: a second wavefront
    with one working lane; 128: two full wavefronts; 384: six; 1000, 1024: all 16 vote words.  B = 1,
    fpg - 1, fpg + 1 and all frames from one plan."""
    want = S.z_want(Z, early_stop)
    dec = _dec(S.z_base(Z), Z, S.STD, S.Z_ITER, early_stop)
    _holds(dec, S.LIFT[Z])
    for B in S.z_batches(Z):
        _same(_soft(dec, S.z_pool(Z)[:B]), want, B)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("Z", sorted(S.STUCK_R))
def test_stuck_frame_votes_in_a_late_wavefront(gpu, Z, early_stop):
    """The same pools at llr_max = 127: the last frame (every LLR +8, one of -127) never stops, and after
    iteration 1 only checks at index r or above of their block rows say so: r = 51, 124 (the second
    wavefront's vote word), 329, 700, 790 (past the fourth wavefront)."""
    want = S.stuck_want(Z, early_stop)
    dec = _dec(S.z_base(Z), Z, S.STUCK, S.Z_ITER, early_stop)
    _holds(dec, S.LIFT[Z])
    _same(_soft(dec, S.z_pool(Z)), want)
    _same(_soft(dec, S.z_pool(Z)[-1:]), [w[-1:] for w in want])


def test_z1024_dcap32(gpu):
    """Row degrees [12, 24, 3, 32] at Z = 1024: the 32-register instance at 1024 threads, two words a check,
    8 m + n = 64 KiB of state in LDS."""
    base, llr = S.d32_case()
    dec = _dec(base, S.D32["Z"], S.STD, S.D32["max_iter"])
    _holds(dec, S.D32_GEOM)
    _same(_soft(dec, llr), S.d32_want())


# ---- b. planner edges ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.EDGES))
def test_planner_edges(gpu, name):
    """The largest LDS-resident plans (163 808 bytes in a block with one and with two words a check, P behind
    4 m mw bytes of check words; 163 840 in a sub-wave workgroup at Z = 32 and at Z = 1) and their neighbours
    on the workspace by the planner's own choice; fpb = 4, 3, 3, 2, 2, 1 wavefronts per workgroup at Z = 32
    with fpg + 1 frames, so every wavefront's LDS slots hold live frames."""
    deg, mb, nb, Z, frames, g = S.EDGES[name]
    base, llr = S.edge_case(name)
    want = S.edge_want(name)
    dec = _dec(base, Z, S.STD, S.EDGE_ITER)
    _holds(dec, g)
    _same(_soft(dec, llr), want)
    if frames > 3:  # a workgroup not full
        _same(_soft(dec, llr[:frames - 2]), want, frames - 2)


# ---- c. check-word packing edges ---------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name", sorted(S.PACK))
def test_packing_edges(gpu, name, early_stop):
    """The widest row's checks read, frame by frame: the minimum at the last input (idx1 = 13 in 4 bits, 2046
    in 11 beside the parity bit), every input negative, only the last one (bit 31 of word 0 at degree 14, of
    a flag word at 32 and 64; the first bit of a new flag word at 33 and 65), one zero, two zeros, and
    |L| = 127 throughout (both stored minima 127)."""
    degrees, nb, Z, max_iter, noisy, g = S.PACK[name]
    base, llr = S.pack_case(name)
    want = S.pack_want(name, early_stop)
    dec = _dec(base, Z, S.FULL, max_iter, early_stop)
    _holds(dec, g)
    _same(_soft(dec, llr), want)


# ---- d. rate-matched frames ------------------------------------------------------------
@pytest.mark.parametrize("reordered", [True, False])
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name", sorted(S.RATE))
def test_rate_matched_frames(gpu, name, early_stop, reordered):
    """Codewords of QCLDPCEncoder, the first two block columns punctured (0) and the fillers at +llr_max;
    with the block rows that read both punctured columns first in the layer order (every such check has
    minimum 0 in iteration 1), and in the natural order."""
    base, Z, llr, cw, fillers = S.rate_case(name)
    want = S.rate_want(name, early_stop, reordered)
    dec = _dec(base, Z, S.STD, S.RATE_ITER, early_stop,
               layer_order=S.rate_layer_order(base)[0] if reordered else None)
    _holds(dec, S.RATE[name][3])
    _same(_soft(dec, llr), want)

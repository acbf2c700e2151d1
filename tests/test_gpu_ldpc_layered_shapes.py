"""LayeredMSDecoder (ldpc_layered.hip) against the restatements at the layer
widths, planner edges, packing edges and layer shapes of tests/layered_shapes.py,
and the posteriors of every layered decoder across lms_decode_impl's chunks.
Bar: hard decisions and iteration counts array_equal, posteriors array_equal with
equal_nan.  The builders of layered_shapes.py assert every condition on the inputs
on the restatement before the device is asked; tests/test_ldpc_layered_shapes_host.py
holds the geometry tables against the planner and states what they reach."""
import numpy as np
import pytest
import torch

import layered_shapes as S

pytestmark = pytest.mark.gpu


def _same(got, want, B=None):
    bits, its, post = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    want = [w[:B] for w in want]
    assert np.array_equal(bits, want[0])
    assert np.array_equal(its, want[1])
    assert post.dtype == want[2].dtype and np.array_equal(post, want[2], equal_nan=want[2].dtype.kind == "f")


def _soft(dec, llr):
    return dec.decode_batch(np.array(llr), return_iterations=True, return_llr=True)


def _qc_dec(base, Z, max_iter, early_stop):
    """The generic decoder on the expanded H, the block rows as layers."""
    Lib = S.L()
    return Lib.LayeredMSDecoder(Lib.qc_expand(base, Z), max_iter=max_iter, normalization=S.NORM, early_stop=early_stop,
                                layers=Lib.qc_block_layers(np.asarray(base).shape[0], Z))


def _holds(dec, g):
    """The plan made is the row of the table (the host file holds the rest of the row against the planner)."""
    info = dec.plan.info
    assert info.reserved == (10 if g["use_global"] else 9) and info.frames_per_block == g["fpb"]
    assert info.lds_bytes == g["lds"]
    assert (dec.plan.workspace_bytes(1) == g["state"]) if g["use_global"] else (dec.plan.workspace_bytes(1) == 0)


# ---- a. layer widths -------------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("Z", sorted(S.WIDTHS))
def test_layer_widths(gpu, Z, early_stop):
    """64: the widest layer a wavefront takes; 65: a second wavefront with one working lane; 1024: 16
    wavefronts, all 16 vote words (the last frame never stops, and only a word past the eighth says so);
    1025, 2049: a second and a third trip of the layer loop, taken by thread 0 alone."""
    want = S.width_want(Z, early_stop)
    dec = _qc_dec(S.width_base(Z), Z, S.WIDTH_ITER, early_stop)
    _holds(dec, S.WIDTHS[Z])
    for B in S.width_batches(Z):
        _same(_soft(dec, S.width_llr(Z)[:B]), want, B)


@pytest.mark.parametrize("early_stop", [True, False])
def test_strided_layer_loop_on_workspace_state(gpu, monkeypatch, early_stop):
    monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    Z = 1025
    want = S.width_want(Z, early_stop)
    dec = _qc_dec(S.width_base(Z), Z, S.WIDTH_ITER, early_stop)
    _holds(dec, S.WIDTH_GLOBAL[Z])
    for B in S.width_batches(Z):
        _same(_soft(dec, S.width_llr(Z)[:B]), want, B)


# ---- b. planner edges ------------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("nb", sorted(S.LADDER))
def test_frames_per_workgroup_ladder(gpu, nb, early_stop):
    """fpb = 4, 3, 2, 1 at their boundaries, the last plan the LDS holds, and the first the planner itself
    moves to the workspace; a workgroup full, ragged, and followed by a second."""
    want = S.ladder_want(nb, early_stop)
    llr = S.ladder_llr(nb)
    dec = _qc_dec(S.ladder_base(nb), S.LADDER_Z, S.LADDER_ITER, early_stop)
    _holds(dec, S.LADDER[nb])
    for B in S.ladder_batches(nb):
        got = _soft(dec, llr[:B])
        _same(got, want, B)
        assert np.array_equal(got[2][:, 512:], llr[:B, 512:])  # a variable of no check keeps its LLR


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("Z", sorted(S.BLOCK_EDGE))
def test_block_mapping_lds_edge(gpu, Z, early_stop):
    """state + 128 vote bytes <= 160 KB at Z = 909, not at 910."""
    base, llr = S.edge_case(Z)
    dec = _qc_dec(base, Z, S.EDGE_ITER, early_stop)
    _holds(dec, S.BLOCK_EDGE[Z])
    _same(_soft(dec, llr), S.edge_want(Z, early_stop))


# ---- c. packing edges ------------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name", sorted(S.PACKS))
def test_packing_edges(gpu, name, early_stop):
    """The minimum, a NaN, a zero and two zeros at the last position(s) of a check of degree 16 (one word
    full), 17 and 33 (the first of the two- and three-word forms), 65 and 2047 (all 11 position bits)."""
    base, Z, max_iter, llr = S.pack_case(name)
    want = S.pack_want(name, early_stop)
    dec = _qc_dec(base, Z, max_iter, early_stop)
    _holds(dec, S.PACKS[name])
    _same(_soft(dec, llr), want)


# ---- d. irregular layers ---------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name", sorted(S.IRREGULAR))
def test_irregular_layers(gpu, name, early_stop):
    """Degrees on both sides of 16, 32 and 64 in neighbouring lanes, a zero-degree row, two empty layers and
    a layer of one check; special values in the last two frames."""
    H, layers, llr = S.irregular_case(name)
    want = S.irregular_want(name, early_stop)
    dec = S.L().LayeredMSDecoder(H, max_iter=S.IRR_ITER, normalization=S.NORM, early_stop=early_stop, layers=layers)
    _holds(dec, S.IRREGULAR[name])
    for B in (1, len(llr)):
        _same(_soft(dec, llr[:B]), want, B)


# ---- e. posteriors across chunks -------------------------------------------------------
def _chunked(plan_of, llr, want, chunk, reserved):
    """decode_batch on a device input, then plan.decode_soft into a pitched posterior whose padding keeps
    its sentinel; the stream's workspace is one chunk of state slices."""
    dec = plan_of()
    plan = dec.plan
    assert plan.info.reserved == reserved  # the state is in the workspace
    frames, n = llr.shape
    unit = plan.workspace_bytes(1)
    assert unit > 0 and plan.workspace_bytes(frames) == chunk * unit and frames > 2 * chunk
    dev = torch.from_numpy(np.array(llr)).cuda()
    got = dec.decode_batch(dev, return_iterations=True, return_llr=True)
    assert all(x.is_cuda for x in got)
    _same(got, want)
    sentinel = 99 if llr.dtype == np.int8 else -777.0
    wide = torch.full((frames, n + 24), sentinel, dtype=dev.dtype, device="cuda")
    bits = torch.full((frames, n), 7, dtype=torch.uint8, device="cuda")
    its = torch.full((frames,), -1, dtype=torch.int32, device="cuda")
    plan.decode_soft(dev, bits, its, wide[:, :n])
    _same((bits, its, wide[:, :n]), want)
    assert bool((wide[:, n:] == sentinel).all())
    assert plan.workspace_stats() == (1, chunk * unit)


@pytest.mark.parametrize("name", sorted(S.CHUNKED))
def test_posteriors_across_chunks(gpu, monkeypatch, name):
    """13 frames in chunks of 5, 5 and 3 through lms_decode_impl, for each of the four layered decoders:
    the bits, counts and posterior rows behind the first chunk, with and without a row pitch."""
    monkeypatch.setenv("PL_LDPC_CHUNK", str(S.CHUNK))
    monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    make, llr, want = S.chunk_case(name)
    _chunked(make, llr, want, S.CHUNK, S.CHUNKED[name]["reserved"])


def test_posteriors_across_chunks_of_the_planners_own_workspace_plan(gpu, monkeypatch):
    nb, chunk, _ = S.CHUNK_LADDER
    monkeypatch.setenv("PL_LDPC_CHUNK", str(chunk))
    llr, want = S.chunk_ladder_case()
    _chunked(lambda: _qc_dec(S.ladder_base(nb), S.LADDER_Z, S.LADDER_ITER, True), llr, want, chunk, 10)

"""The input routes of the flooding decoders' decode_batch (BPDecoder, MSDecoder)
on the (504, 252) golden code: CUDA views with a row pitch, other dtypes and
strides, `out=`, empty batches.  Expected values are the reference's recorded
outputs (tests/golden/ldpc_bp_504.npz, ldpc_ms_504.npz) and the C oracle.
Seven frames leave a ragged last workgroup at one and at two frames per group."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

B, N = 7, 504


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


@pytest.fixture(scope="module")
def cases(oracle):
    """algo -> (make_decoder, llr [7, 504], bits, iterations, bits and iterations of the fp32-rounded llr)."""
    L = _L()
    bp, ms = golden("ldpc_bp_504.npz"), golden("ldpc_ms_504.npz")
    Hbp, Hms = (L.csr_to_dense(d["row_ptr"], d["col_idx"], N) for d in (bp, ms))  # each fixture has its own code
    out = {}
    for algo, d, mk, llr, bits, norm in (
            ("bp", bp, lambda: L.BPDecoder(Hbp, max_iter=20), bp["harness_llr"][:B], bp["harness_bits"][:B], 1.0),
            ("ms", ms, lambda: L.MSDecoder(Hms, max_iter=20, normalization=0.75), ms["llr"][:B], ms["ms_0.75"][:B],
             0.75)):
        def orc(x):
            return oracle.ldpc_decode(d["row_ptr"], d["col_idx"], N, x, algo=algo, max_iter=20, norm=norm, threads=4)
        ob, oi = orc(llr)
        assert np.array_equal(ob, bits)  # the oracle restates the fixture; its iteration counts stand in for MS
        its = bp["harness_iters"][:B] if algo == "bp" else oi
        for a in (llr, bits, its):
            a.setflags(write=False)
        out[algo] = (mk, llr, bits, its, orc(llr.astype(np.float32).astype(np.float64)))
    return out


def _host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("algo", ["bp", "ms"])
def test_device_routes(gpu, cases, algo):
    mk, llr, bits, its, _ = cases[algo]
    dec = mk()
    # a view with row pitch n + 40 and NaN padding, decoded where it lies
    wide = torch.full((B, N + 40), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :N] = torch.tensor(llr, device="cuda")
    gb, gi = dec.decode_batch(wide[:, :N], return_iterations=True)
    assert gb.is_cuda and gb.dtype == torch.uint8 and gb.shape == (B, N)
    assert gi.is_cuda and gi.dtype == torch.int32 and gi.shape == (B,)
    assert np.array_equal(_host(gb), bits) and np.array_equal(_host(gi), its)
    # only the bits asked for: a bare tensor
    g1 = dec.decode_batch(wide[:, :N])
    assert isinstance(g1, torch.Tensor) and np.array_equal(_host(g1), bits)
    # non-unit inner stride: every other column of a double-width buffer
    dbl = torch.full((B, 2 * N), float("nan"), dtype=torch.float64, device="cuda")
    dbl[:, ::2] = torch.tensor(llr, device="cuda")
    assert dbl[:, ::2].stride(1) == 2
    assert np.array_equal(_host(dec.decode_batch(dbl[:, ::2])), bits)
    # device out=: the bits land in it
    out = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
    gb, gi = dec.decode_batch(wide[:, :N], out=out, return_iterations=True)
    assert gb.data_ptr() == out.data_ptr() and np.array_equal(_host(out), bits) and np.array_equal(_host(gi), its)


@pytest.mark.parametrize("algo", ["bp", "ms"])
def test_fp32_tensor_is_widened(gpu, cases, algo):
    """A CUDA fp32 tensor is decoded as .to(float64) of it: the oracle on the widened values."""
    mk, llr, _, _, (wb, wi) = cases[algo]
    gb, gi = mk().decode_batch(torch.tensor(llr.astype(np.float32), device="cuda"), return_iterations=True)
    assert gb.dtype == torch.uint8 and gi.dtype == torch.int32
    assert np.array_equal(_host(gb), wb) and np.array_equal(_host(gi), wi)


@pytest.mark.parametrize("algo", ["bp", "ms"])
def test_host_out_is_ignored(gpu, cases, algo):
    """The flooding decoders return a fresh int64 array on the host route and leave `out` alone."""
    mk, llr, bits, its, _ = cases[algo]
    out = np.full((B, N), -1, dtype=np.int64)
    gb, gi = mk().decode_batch(llr.copy(), out=out, return_iterations=True)  # the shared llr is read-only
    assert gb is not out and np.all(out == -1)
    assert gb.dtype == np.int64 and gi.dtype == np.int64
    assert np.array_equal(gb, bits) and np.array_equal(gi, its)


@pytest.mark.parametrize("algo", ["bp", "ms"])
def test_empty_cuda_batch(gpu, cases, algo):
    dec = cases[algo][0]()
    gb, gi = dec.decode_batch(torch.empty((0, N), dtype=torch.float64, device="cuda"), return_iterations=True)
    assert gb.is_cuda and gb.shape == (0, N) and gb.dtype == torch.uint8
    assert gi.is_cuda and gi.shape == (0,) and gi.dtype == torch.int32
    assert dec._plan is None  # no library call: not even the plan was made


def test_degree_one_check_empty_batches(gpu):
    """MSDecoder on a code with a degree-1 check: the empty host batch comes back
    without the runnability check, the empty CUDA batch raises as a full one does."""
    L = _L()
    d = golden("ldpc_ms_504.npz")
    H = L.csr_to_dense(d["row_ptr"], d["col_idx"], N)
    keep = int(np.flatnonzero(H[0])[0])
    H[0] = 0
    H[0, keep] = 1
    dec = L.MSDecoder(H, max_iter=5)
    z = dec.decode_batch(np.zeros((0, N)))
    assert z.shape == (0, N) and z.dtype == np.int64
    with pytest.raises(ValueError, match="zero-size array to reduction operation minimum"):
        dec.decode_batch(torch.empty((0, N), dtype=torch.float64, device="cuda"))

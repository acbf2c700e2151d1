"""Addressing of the polar tree kernel (polar_tree.hip): channel rows and the
per-wave workspace slice are reached as a wave-uniform base plus 32-bit
offsets.  Rows far past the first, stale multi-pass workspaces, the slice
bounds and unaligned rows, all against the C oracle, bit for bit.

Small batches would run on the small-batch instances (tree_table_small), so
every case runs twice: with PL_TREE_SMALL=0 set before the plan is created
(the product instance) and with the default."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = pytest.mark.parametrize("small", ["0", None], ids=["product", "default"])


def _P():
    import polarcode_and_ldpc_amd.polar as P
    return P


def _mismatch(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).any(axis=1).sum())


def _decoder(monkeypatch, small, N, L, waves=None):
    """(decoder, frozen set) of the rate-1/2 code; L = 0: SC.  The environment
    is read when the plan is created."""
    P = _P()
    if small is not None:
        monkeypatch.setenv("PL_TREE_SMALL", small)
    if waves is not None:
        monkeypatch.setenv("PL_POLAR_WAVES", str(waves))
    K = N // 2
    fr = P.construct_frozen_set(N, K, 2.0)
    dec = P.SCDecoder(N, K, frozen_bits=fr) if L == 0 else P.SCLDecoder(N, K, L, frozen_bits=fr)
    assert dec.plan.info.reserved == 4  # the tree kernel
    return dec, fr


def _noisy(dec, N, B, snr, seed):
    """LLRs [B, N] of random codewords over AWGN at `snr` dB (device)."""
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    msg = torch.empty((B, N // 2), dtype=torch.uint8, device="cuda")
    _native.random_bits(seed, 0, msg)
    cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    _native.polar_encode(dec.plan, msg, cw)
    return AWGNChannel(snr).llr_batch_device(cw, N, B, seed=seed + 1)


def _oracle_bits(oracle, N, L, fr, llr):
    x = llr.cpu().numpy()
    return oracle.sc_decode(N, fr, x, threads=16) if L == 0 else oracle.scl_decode(N, L, fr, x, threads=16)


@SMALL
@pytest.mark.parametrize("ld", [65536, 65537])
@pytest.mark.parametrize("L", [8, 0])
def test_rows_beyond_4gib(gpu, oracle, monkeypatch, small, L, ld):
    """8 256 rows at a pitch of 65 536 doubles: the last rows start more than
    4 GiB past the first, so a frame group's base needs 64-bit arithmetic.
    Pitch 65 537 is odd: the rows are staged instead of read in place as
    pairs.  Every frame equals the contiguous decode of the same LLRs; the
    first and last 64 equal the oracle's."""
    N, B = 128, 8256
    dec, fr = _decoder(monkeypatch, small, N, L)
    llr = _noisy(dec, N, B, 3.0, 301)
    big = torch.empty(((B - 1) * ld + N,), dtype=torch.float64, device="cuda")  # only the view is written
    assert big.numel() * 8 > (1 << 32)
    view = big.as_strided((B, N), (ld, 1))
    view.copy_(llr)
    got = torch.empty((B, N // 2), dtype=torch.uint8, device="cuda")
    want = torch.empty((B, N // 2), dtype=torch.uint8, device="cuda")
    dec.plan.decode(view, got)
    dec.plan.decode(llr, want)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    idx = torch.cat([torch.arange(0, 64), torch.arange(B - 64, B)]).cuda()
    assert _mismatch(got[idx].cpu().numpy(), _oracle_bits(oracle, N, L, fr, llr[idx])) == 0


@SMALL
@pytest.mark.parametrize("L", [8, 0])
def test_rows_of_one_group_2gib_apart(gpu, oracle, monkeypatch, small, L):
    """A pitch of 2^25 doubles: the rows of one frame group span 2^31 bytes or
    more, past what a 32-bit lane offset from the group's first row reaches, so
    the kernel reads them through per-lane addresses.  Two groups and a ragged
    third; every frame equals the oracle's."""
    N, B, ld = 128, 19, 1 << 25
    dec, fr = _decoder(monkeypatch, small, N, L)
    llr = _noisy(dec, N, B, 3.0, 351 + L)
    big = torch.empty(((B - 1) * ld + N,), dtype=torch.float64, device="cuda")  # only the view is written
    view = big.as_strided((B, N), (ld, 1))
    view.copy_(llr)
    out = torch.empty((B, N // 2), dtype=torch.uint8, device="cuda")
    dec.plan.decode(view, out)
    torch.cuda.synchronize()
    assert _mismatch(out.cpu().numpy(), _oracle_bits(oracle, N, L, fr, llr)) == 0


@SMALL
@pytest.mark.parametrize("N,L", [(1024, 8), (1024, 32), (1024, 16), (1024, 4), (2048, 8), (4096, 8), (512, 16), (256, 2),
                                 (1024, 0), (4096, 0)])
def test_stale_workspace_ragged_tail(gpu, oracle, monkeypatch, small, N, L):
    """A grid of 3 wavefronts decodes 3 groups each, over the workspace the
    earlier groups left behind, and a ragged last group of 5 frames: one case
    per frames-per-wave count, tier split and walk depth."""
    fpw = 64 // max(L, 1)
    dec, fr = _decoder(monkeypatch, small, N, L, waves=3)
    B = 3 * 3 * fpw + 5
    llr = _noisy(dec, N, B, 1.0 if L == 32 else 3.0, 311 + N + L)
    out = torch.empty((B, N // 2), dtype=torch.uint8, device="cuda")
    dec.plan.decode(llr, out)
    torch.cuda.synchronize()
    assert _mismatch(out.cpu().numpy(), _oracle_bits(oracle, N, L, fr, llr)) == 0


@SMALL
@pytest.mark.parametrize("N", [1024, 4096])
def test_workspace_slice_bounds(gpu, oracle, monkeypatch, small, N):
    """The caller's workspace (NaN masks, the scheduler block, two wavefront
    slices) sits inside a larger tensor filled with a sentinel.  After a decode
    the bytes before it and after its last slice are untouched, as are the
    mask words of wavefronts that do not exist and the scheduler block past
    its counter; the bits equal the oracle's."""
    L, G, S = 8, 1 << 16, 0x5A
    dec, fr = _decoder(monkeypatch, small, N, L, waves=2)
    plan = dec.plan
    unit = plan.workspace_bytes(1)
    slice_ = plan.workspace_bytes(64 // L + 1) - unit
    head = unit - slice_  # the mask region and the 4096-byte scheduler block
    need = plan.workspace_bytes(1 << 20)
    assert slice_ > 0 and head > 4096 and need == head + 2 * slice_  # two resident wavefronts
    B = 2 * 2 * (64 // L) + 3
    llr = _noisy(dec, N, B, 3.0, 331 + N)
    big = torch.full((G + need + G,), S, dtype=torch.uint8, device="cuda")
    assert (big.data_ptr() + G) % 256 == 0
    out = torch.empty((B, N // 2), dtype=torch.uint8, device="cuda")
    plan.decode(llr, out, ws=big[G:G + need])
    torch.cuda.synchronize()
    assert _mismatch(out.cpu().numpy(), _oracle_bits(oracle, N, L, fr, llr)) == 0
    assert bool((big[:G] == S).all()), "bytes before the workspace changed"
    assert bool((big[G + need:] == S).all()), "bytes after the last slice changed"
    masks_used = 2 * 8 * 64  # u64 [2 wavefronts][64 passes]
    assert bool((big[G + masks_used:G + head - 4096] == S).all()), "mask words of absent wavefronts changed"
    assert bool((big[G + head - 4096 + 4:G + head] == S).all()), "the scheduler block past its counter changed"


@SMALL
@pytest.mark.parametrize("N,L", [(2048, 8), (1024, 32)])
def test_unaligned_base_and_pitch(gpu, oracle, monkeypatch, small, N, L):
    """Rows at a pitch of N + 1 doubles from a base one double past a 16-byte
    boundary: no row is 16-byte aligned throughout, so depth 0 is staged."""
    pad, off, B = 1, 1, 70
    dec, fr = _decoder(monkeypatch, small, N, L)
    llr = _noisy(dec, N, B, 1.0 if L == 32 else 3.0, 341 + N + L)
    buf = torch.full((B * (N + pad) + off + 8,), float("nan"), dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + B * (N + pad)].view(B, N + pad)[:, :N]
    view.copy_(llr)
    out = torch.empty((B, N // 2), dtype=torch.uint8, device="cuda")
    dec.plan.decode(view, out)
    torch.cuda.synchronize()
    assert _mismatch(out.cpu().numpy(), _oracle_bits(oracle, N, L, fr, llr)) == 0

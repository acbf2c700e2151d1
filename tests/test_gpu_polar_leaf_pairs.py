"""The tree kernel's leaf loop decodes leaves as (even, odd) pairs, reads the
frozen mask one 32-leaf word at a time and keeps narrow pointer rows at list
capacities <= 8 (polar_tree.hip, TG::PAIR / FZW / NARROW).  Frozen sets built in
DECODE order (leaf i decodes index bitrev(i)) put every pair shape, rate-0 quads
and octets at every alignment, frozen prefixes and the frame's two ends on the
pair and word boundaries; every decoded bit is compared with the C oracle.

Each case decodes twice: with the plan as planned (small batches pick the
small-batch instance where there is one) and with a plan created under
PL_TREE_SMALL=0 (the product instance)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, list size): LCAP = 8 at every N the tree kernel serves below 2048, list
# sizes below the capacity 8, and the capacities 4 and 32 (5-bit rows) at N = 1024
INSTANCES = [(128, 8), (256, 8), (512, 8), (1024, 8), (1024, 5), (1024, 7), (1024, 4), (1024, 32)]
FRAMES = 21  # a ragged last group at 2, 8 and 16 frames per wavefront


def _P():
    import polarcode_and_ldpc_amd.polar as P
    return P


def _mismatch(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).any(axis=1).sum())


def _frozen_from_decode_mask(m):
    """Frozen indices of the decode-order mask m (True = frozen leaf)."""
    N = len(m)
    n = N.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % n)[::-1], 2) for i in range(N)])
    return np.sort(rev[np.nonzero(m)[0]])


def _stamp(m, start, pat):
    for j, c in enumerate(pat):
        assert 0 <= start + j < len(m), (start, pat)
        m[start + j] = c == "F"


def _background(N, rng):
    """Random pair shapes: each aligned pair is FI, IF, II or FF."""
    m = np.zeros(N, bool)
    for p in range(N // 2):
        s = rng.randint(4)
        m[2 * p], m[2 * p + 1] = s in (0, 3), s in (1, 3)
    return m


def _pair_masks(N, rng):
    """Pair p has shape (p + v) % 4 of (even frozen / odd info, even info / odd
    frozen, both info, both frozen): over v = 0..3 every shape sits on every
    pair, among them (0, 1), (30, 31), (32, 33), (62, 63), (64, 65), (N-2, N-1)."""
    shapes = ("FI", "IF", "II", "FF")
    out = []
    for v in range(4):
        m = np.zeros(N, bool)
        for p in range(N // 2):
            _stamp(m, 2 * p, shapes[(p + v) % 4])
        out.append(m)
    return out


def _node_masks(N, rng):
    """All-frozen runs of 4 and 8 leaves, fenced by info leaves, over random pair
    shapes.  At the word boundaries 31/32 and 63/64 a run ends at the boundary,
    starts at it, crosses it from a pair boundary (not a node of its size) or
    from an odd leaf; runs of 4 at leaves 80 + v and of 8 at 96 + v start at
    every offset of an octet over v = 0..7."""
    out = []
    for v in range(8):
        m = _background(N, rng)
        for w, S, kind in ((32, 4 if v < 4 else 8, v % 4), (64, 8 if v < 4 else 4, (v + 1) % 4)):
            start = (w - S, w, w - S // 2, w - S // 2 - 1)[kind]
            _stamp(m, start - 1, "I" + "F" * S + "I")
        _stamp(m, 80 + v - 1, "I" + "F" * 4 + "I")
        _stamp(m, 96 + v - 1, "I" + "F" * 8 + "I")
        out.append(m)
    return out


def _prefix_masks(N, rng):
    """A frozen prefix of p leaves, then six info leaves (the list grows 1 -> 2 ->
    4 -> 8 across pairs, from an odd first info leaf for p = 2^k - 1 and 2^k + 1,
    from an even one for p = 2^k and 2^k + 2; p = 0: leaf 0 is an info bit);
    leaf N - 1 is an info bit, leaf N - 2 frozen in every other mask."""
    out = []
    for p in [0] + [(1 << k) + d for k in (2, 5, 6) for d in (-1, 1, 0, 2)]:
        m = _background(N, rng)
        m[:p] = True
        _stamp(m, p, "IIIIII")
        m[N - 1] = False
        m[N - 2] = len(out) % 2 == 0
        out.append(m)
    return out


FAMILIES = {"pairs": _pair_masks, "nodes": _node_masks, "prefix": _prefix_masks}


def _noisy_frames(N, fr, B, rng, snr_lo=-2.0, snr_hi=2.0):
    P = _P()
    K = N - len(fr)
    msg = rng.randint(0, 2, (B, K))
    cw = P.PolarEncoder(N, K, frozen_bits=fr).encode_batch(msg)
    snr = rng.uniform(snr_lo, snr_hi, size=(B, 1))
    sigma = np.sqrt(1.0 / (2.0 * 10 ** (snr / 10.0)))
    return 2.0 * ((1.0 - 2.0 * cw) + sigma * rng.randn(B, N)) / sigma ** 2, msg


def _plans(N, fr, L, monkeypatch, crc=None):
    """(tag, plan): as planned, and created with the small-batch instances off."""
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.polar.utils import CRC_POLYNOMIALS
    mask = np.zeros(N, np.uint8)
    mask[fr] = 1
    out = []
    for tag, env in (("planned", None), ("product", "0")):
        if env is None:
            monkeypatch.delenv("PL_TREE_SMALL", raising=False)
        else:
            monkeypatch.setenv("PL_TREE_SMALL", env)
        plan = _native.polar_plan(N, N - len(fr), mask, L)
        if crc:
            plan.set_crc(int(crc.split("-")[1]), CRC_POLYNOMIALS[crc])
        out.append((tag, plan))
    monkeypatch.delenv("PL_TREE_SMALL", raising=False)
    assert out[1][1].small_batch_frames() == 0
    return out


def _decode(plan, llr, ws_waves=0):
    """Decoded bits; ws_waves > 0: on a caller workspace of that many
    wavefronts' slices, filled with garbage."""
    d = torch.from_numpy(llr).cuda()
    K = plan.info.n_out
    out = torch.empty((len(llr), K), dtype=torch.uint8, device="cuda")
    if ws_waves:
        fpw = 1
        while plan.workspace_bytes(fpw + 1) == plan.workspace_bytes(1):
            fpw += 1
        unit = plan.workspace_bytes(1)
        slice_ = plan.workspace_bytes(fpw + 1) - unit
        ws = torch.full((unit + (ws_waves - 1) * slice_,), 0xA5, dtype=torch.uint8, device="cuda")
        plan.decode(d, out, ws=ws)
    else:
        plan.decode(d, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("N,L", INSTANCES)
def test_pair_shapes_vs_oracle(gpu, oracle, monkeypatch, N, L, family):
    rng = np.random.RandomState(1000 * N + 10 * L + len(family))
    for v, m in enumerate(FAMILIES[family](N, rng)):
        fr = _frozen_from_decode_mask(m)
        llr, _ = _noisy_frames(N, fr, FRAMES, rng)
        want = oracle.scl_decode(N, L, fr, llr, threads=8)
        for tag, plan in _plans(N, fr, L, monkeypatch):
            assert _mismatch(_decode(plan, llr), want) == 0, (family, v, tag)


@pytest.mark.parametrize("L", [8, 32])
def test_three_wave_grid_passes_vs_oracle(gpu, oracle, monkeypatch, L):
    """A workspace of three wavefronts' slices: each wavefront decodes the
    batch's frame groups in many passes over the workspace and LDS its earlier
    frames left behind (garbage before the first).  Noisy frames (-2 dB), a
    ragged last group, every frame against the oracle."""
    P = _P()
    N, K = 1024, 512
    fr = P.construct_frozen_set(N, K, 2.0)
    B = 509 if L == 8 else 255
    rng = np.random.RandomState(17 + L)
    llr, msg = _noisy_frames(N, fr, B, rng, -2.0, -2.0)
    want = oracle.scl_decode(N, L, fr, llr, threads=16)
    assert 0 < _mismatch(want, msg) < B  # a noisy regime: some frames in error
    for tag, plan in _plans(N, fr, L, monkeypatch):
        assert _mismatch(_decode(plan, llr, ws_waves=3), want) == 0, tag


def test_cascl_crc8_vs_oracle(gpu, oracle, monkeypatch):
    """CRC-aided selection (CRC-8) at the end of the pair loop's last walk."""
    from polarcode_and_ldpc_amd.polar.utils import crc_encode
    P = _P()
    N, K, L, crc = 1024, 512, 8, "CRC-8"
    fr = P.construct_frozen_set(N, K, 2.0)
    rng = np.random.RandomState(88)
    B = 45
    msg = np.stack([crc_encode(rng.randint(0, 2, K - 8), crc) for _ in range(B)])
    cw = P.PolarEncoder(N, K, frozen_bits=fr).encode_batch(msg)
    snr = rng.uniform(0.0, 1.5, size=(B, 1))
    sigma = np.sqrt(1.0 / (2.0 * 10 ** (snr / 10.0)))
    llr = 2.0 * ((1.0 - 2.0 * cw) + sigma * rng.randn(B, N)) / sigma ** 2
    want = oracle.cascl_decode(N, L, fr, llr, crc, threads=8)
    for tag, plan in _plans(N, fr, L, monkeypatch, crc=crc):
        assert _mismatch(_decode(plan, llr), want) == 0, tag


def _special_set(N, rng):
    return _frozen_from_decode_mask(_node_masks(N, rng)[3])


def test_single_inf_input_per_frame_vs_oracle(gpu, oracle, monkeypatch):
    """One +-inf input in every frame (at a frozen or an info index): the frame
    stays on the tree kernel, paths reach -inf metrics."""
    N, L = 1024, 8
    rng = np.random.RandomState(5)
    fr = _special_set(N, rng)
    llr, _ = _noisy_frames(N, fr, 61, rng, 0.0, 2.0)
    for f in range(len(llr)):
        p = rng.randint(N)
        llr[f, p] = (np.inf, -np.inf)[f % 2] * (1.0 if llr[f, p] >= 0 else -1.0) * (1.0, -1.0)[(f // 2) % 2]
    want = oracle.scl_decode(N, L, fr, llr, threads=8)
    for tag, plan in _plans(N, fr, L, monkeypatch):
        assert _mismatch(_decode(plan, llr), want) == 0, tag


def test_nan_inputs_take_the_redo_path_vs_oracle(gpu, oracle, monkeypatch):
    """NaN inputs in a third of the frames: those frames are flagged and decoded
    again in the reference's candidate order, the others keep the kernel's bits."""
    N, L = 1024, 8
    rng = np.random.RandomState(6)
    fr = _special_set(N, rng)
    llr, _ = _noisy_frames(N, fr, 61, rng, 0.0, 2.0)
    for f in range(0, len(llr), 3):
        llr[f, rng.choice(N, size=1 + f % 5, replace=False)] = np.nan
    want = oracle.scl_decode(N, L, fr, llr, threads=8)
    for tag, plan in _plans(N, fr, L, monkeypatch):
        assert _mismatch(_decode(plan, llr), want) == 0, tag

"""The NumPy restatement of the quasi-cyclic layered sum-product decoder
(tests/qc_bp_ref.py) on the CPU: against a per-check scalar loop of the
definition (array_equal), against an independent layered 2 atanh(prod tanh)
decoder on converged frames, the box-plus identities, special inputs and the
clamp.  No device."""
import functools
import math

import numpy as np
import pytest

from qc_bp_ref import boxplus, check_update, clampq, qc_bp_ref

LN2 = math.log(2.0)


def random_base(mb, nb, Z, dv, seed):
    """Every block column gets dv blocks in distinct block rows, random shifts."""
    rs = np.random.RandomState(seed)
    base = np.full((mb, nb), -1, dtype=np.int64)
    for j in range(nb):
        base[rs.choice(mb, dv, replace=False), j] = rs.randint(0, Z, dv)
    return base


def awgn(n, frames, snr_db, seed):
    """All-zero codeword over BPSK + AWGN, LLR = 2 y / sigma^2."""
    rng = np.random.RandomState(seed)
    sigma = np.sqrt(1.0 / (2.0 * 10.0 ** (snr_db / 10.0)))
    return 2.0 * (1.0 + sigma * rng.randn(frames, n)) / sigma ** 2


# ---- the definition, one check and one Python float at a time ---------------------------------
def _f(x):
    return float(np.asarray(x).reshape(()))


def _clampq1(x, clip):
    if x != x:
        return 0.0
    return clip if x > clip else (-clip if x < -clip else x)


def _boxplus1(a, b):
    from polarcode_and_ldpc_amd.channel import libm_np
    m = abs(b) if abs(b) < abs(a) else abs(a)
    s = -m if (a < 0) != (b < 0) else m
    cp = _f(libm_np.log1p(_f(libm_np.expm1(-abs(a + b))) + 1.0))
    cm = _f(libm_np.log1p(_f(libm_np.expm1(-abs(a - b))) + 1.0))
    return s + (cp - cm)


def scalar_ref(base, Z, L, max_iter, clip, early_stop, layer_order=None):
    base = np.asarray(base)
    mb, nb = base.shape
    order = list(range(mb)) if layer_order is None else list(layer_order)
    bits, its, post = [], [], []
    for frame in np.asarray(L, dtype=np.float64):
        P = [_clampq1(float(x), clip) for x in frame]
        R = {}
        done = max_iter
        for it in range(max_iter):
            for i in order:
                cols = [j for j in range(nb) if base[i, j] >= 0]
                d = len(cols)
                if d == 0:
                    continue
                for r in range(Z):
                    v = [c * Z + (r + int(base[i, c])) % Z for c in cols]
                    q = [_clampq1(P[v[j]] - R.get((i, r, j), 0.0), clip) for j in range(d)]
                    F = [q[0]]
                    for j in range(1, d - 1):
                        F.append(_boxplus1(F[j - 1], q[j]))
                    Bk = {d - 1: q[d - 1]}
                    for j in range(d - 2, 0, -1):
                        Bk[j] = _boxplus1(q[j], Bk[j + 1])
                    for j in range(d):
                        rn = Bk[1] if j == 0 else F[d - 2] if j == d - 1 else _boxplus1(F[j - 1], Bk[j + 1])
                        P[v[j]] = q[j] + rn
                        R[(i, r, j)] = rn
            if early_stop:
                par = 0
                for i in order:
                    cols = [j for j in range(nb) if base[i, j] >= 0]
                    for r in range(Z):
                        par |= sum(P[c * Z + (r + int(base[i, c])) % Z] <= 0 for c in cols) & 1
                if par == 0:
                    done = it + 1
                    break
        bits.append([int(x <= 0) for x in P])
        its.append(done)
        post.append(P)
    return np.array(bits, dtype=np.int64), np.array(its, dtype=np.int64), np.array(post, dtype=np.float64)


def same_bits(a, b):
    """array_equal by bit pattern: -0.0 is not +0.0."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("case", ["plain", "order_and_empty_row", "clip4", "specials"])
def test_vectorised_equals_the_scalar_loop(case):
    Z = 5
    base = random_base(4, 8, Z, 3, seed=11)
    L = awgn(8 * Z, 6, 0.0, seed=12)
    kw = dict(max_iter=6, clip=64.0, early_stop=True)
    if case == "order_and_empty_row":
        base[1] = -1
        base[2, :] = -1
        base[2, [1, 6]] = [3, 0]  # a degree-2 row: its two inputs swap
        kw["layer_order"] = [3, 1, 0, 2]
    if case == "clip4":
        kw["clip"] = 4.0
    if case == "specials":
        L[0, 3], L[1, 5], L[2, 7], L[3, :], L[4, :] = np.nan, np.inf, -np.inf, np.inf, 0.0
        L[5, 2] = -0.0
        kw["early_stop"] = False
    got = qc_bp_ref(base, Z, L, **kw)
    want = scalar_ref(base, Z, L, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert same_bits(got[2], want[2])


# ---- against an independent layered tanh-rule decoder -----------------------------------------
def tanh_ref(base, Z, L, max_iter, clip, early_stop):
    """The textbook rule R_j = 2 atanh(prod_{k != j} tanh(q_k / 2)) on the same schedule, with
    np.tanh / np.arctanh: no box-plus, no recursion, no libm restatement."""
    base = np.asarray(base)
    mb, nb = base.shape
    P = np.clip(np.nan_to_num(np.asarray(L, dtype=np.float64), nan=0.0, posinf=clip, neginf=-clip), -clip, clip)
    rr = np.arange(Z)[:, None]
    V = {}
    for i in range(mb):
        cols = np.nonzero(base[i] >= 0)[0]
        V[i] = cols[None, :] * Z + (rr + base[i, cols][None, :]) % Z
    B = P.shape[0]
    R = {i: np.zeros((B, Z, V[i].shape[1])) for i in range(mb)}
    its = np.full(B, max_iter, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    for it in range(max_iter):
        for i in range(mb):
            q = np.clip(P[:, V[i]] - R[i], -clip, clip)
            t = np.tanh(q / 2)
            Rn = np.empty_like(q)
            for j in range(q.shape[-1]):
                pr = np.prod(np.delete(t, j, axis=-1), axis=-1)
                Rn[..., j] = 2 * np.arctanh(np.clip(pr, -1 + 1e-16, 1 - 1e-16))
            Pv = P[:, V[i]]
            Pv[live] = (q + Rn)[live]
            P[:, V[i]] = Pv
            R[i][live] = Rn[live]
        if early_stop:
            hard = P <= 0
            bad = np.zeros(B, dtype=bool)
            for i in range(mb):
                bad |= (hard[:, V[i]].sum(-1) & 1).any(-1)
            its[live & ~bad] = it + 1
            live = live & bad
            if not live.any():
                break
    return (P <= 0).astype(np.int64), its, P


TANH_CASES = [(27, -1.0), (27, 0.0), (96, -0.5)]


@functools.lru_cache(maxsize=None)
def _tanh_case(Z, snr):
    base = random_base(4, 8, Z, 3, seed=500 + Z)
    L = awgn(8 * Z, 256, snr, seed=700 + Z)
    return base, L, qc_bp_ref(base, Z, L, 20, 64.0, True)


def test_agrees_with_the_tanh_rule_on_converged_frames():
    """On frames where the restatement stops before max_iter the two decoders take the same hard
    decisions in the same number of iterations; they differ through rounding only, so at most 1 % of
    the converged frames may disagree."""
    converged = differ = 0
    for Z, snr in TANH_CASES:
        base, L, (bits, its, _) = _tanh_case(Z, snr)
        print(Z, snr, "restatement iterations:", np.bincount(its, minlength=21))
        assert len(np.unique(its[its < 20])) >= 3, "the iteration counts do not spread"
        assert (its == 20).any(), "every frame converges"
        tb, ti, _ = tanh_ref(base, Z, L, 20, 64.0, True)
        conv = its < 20
        same = (bits == tb).all(axis=1) & (its == ti)
        converged += int(conv.sum())
        differ += int((conv & ~same).sum())
    print("converged frames:", converged, "of which differ:", differ)
    assert converged >= 300
    assert differ <= converged // 100


# ---- the box-plus ----------------------------------------------------------------------------
def test_boxplus_identities():
    rng = np.random.RandomState(1)
    a = np.concatenate([rng.randn(4000) * 8, rng.randn(500) * 1e-3, [64.0, -64.0, 1e-300, 2.0 ** 20, 131.5]])
    b = np.concatenate([rng.randn(4000) * 8, rng.randn(500) * 40, [64.0, 64.0, -3.0, -2.0 ** 20, -131.5]])
    ab = boxplus(a, b)
    assert np.isfinite(ab).all()
    # a zero input erases: exactly 0
    for z in (0.0, -0.0):
        assert np.array_equal(boxplus(a, np.full_like(a, z)), np.zeros_like(a))
        assert np.array_equal(boxplus(np.full_like(a, z), a), np.zeros_like(a))
    # symmetry: in the order of the inputs and in their signs, bit for bit
    assert same_bits(boxplus(b, a), ab)
    assert same_bits(boxplus(-a, -b), ab)
    assert same_bits(boxplus(-a, b), -ab) and same_bits(boxplus(a, -b), -ab)
    # |a [+] b| <= min(|a|, |b|) up to rounding, sign = product of the signs
    assert (np.abs(ab) <= np.minimum(np.abs(a), np.abs(b)) + 1e-12).all()
    nz = ab != 0
    assert np.array_equal(np.sign(ab[nz]), (np.sign(a) * np.sign(b))[nz])
    # the tanh rule, where that is well conditioned
    ok = np.minimum(np.abs(a), np.abs(b)) < 15
    ref = 2 * np.arctanh(np.tanh(a[ok] / 2) * np.tanh(b[ok] / 2))
    assert np.abs(ab[ok] - ref).max() < 1e-9


def test_degree_two_swaps_and_degree_three_is_one_boxplus_each():
    rng = np.random.RandomState(2)
    q = rng.randn(50, 2) * 6
    assert same_bits(check_update(q), q[:, ::-1])
    q = rng.randn(50, 3) * 6
    Rn = check_update(q)
    assert same_bits(Rn[:, 0], boxplus(q[:, 1], q[:, 2]))
    assert same_bits(Rn[:, 1], boxplus(q[:, 0], q[:, 2]))
    assert same_bits(Rn[:, 2], boxplus(q[:, 0], q[:, 1]))


def test_clampq():
    x = np.array([np.nan, np.inf, -np.inf, 5.0, -5.0, 4.0, -4.0, 0.0, -0.0, 3.5])
    cnt = {"k": 0}
    y = clampq(x, 4.0, cnt, "k")
    assert same_bits(y, np.array([0.0, 4.0, -4.0, 4.0, -4.0, 4.0, -4.0, 0.0, -0.0, 3.5]))
    assert cnt["k"] == 5


# ---- special inputs and the bound --------------------------------------------------------------
@pytest.mark.parametrize("clip", [64.0, 4.0, 2.0 ** 20])
def test_special_inputs_stay_finite_and_bounded(clip):
    Z = 27
    base = random_base(4, 8, Z, 3, seed=500 + Z)
    L = awgn(8 * Z, 8, 1.0, seed=5)
    L[0, 3], L[1, 5], L[2, 7], L[3, :], L[4, :], L[5, :] = np.nan, np.inf, -np.inf, np.inf, 0.0, -np.inf
    L[6, :] = np.nan
    for early_stop in (True, False):
        bits, its, P = qc_bp_ref(base, Z, L, 20, clip, early_stop)
        assert np.isfinite(P).all()
        assert np.abs(P).max() <= 2 * clip + LN2
        # all +inf: with the early stop every posterior is positive and the frame stops at once (without
        # it the clamped q = clampq(P - R) is no extrinsic sum any more and the saturated frame drifts:
        # bounded, not pinned); all zero / all NaN: erasures stay erasures
        if early_stop:
            assert not bits[3].any() and its[3] == 1
        assert not P[4].any() and bits[4].all() and not P[6].any() and bits[6].all()
        # all -inf on a code whose rows have even and odd degrees: just bounded
        assert bits[5].any()


def test_small_clip_acts():
    """clip = 4.0 at 1 dB: channel LLRs and messages beyond 4 exist, so both clamps act, the posteriors
    stay under 2 clip + ln 2; some frames stop and some never do."""
    Z = 27
    base = random_base(4, 8, Z, 3, seed=500 + Z)
    L = awgn(8 * Z, 67, 1.0, seed=600 + Z)
    assert (np.abs(L) > 4.0).any()
    cnt = {}
    bits, its, P = qc_bp_ref(base, Z, L, 20, 4.0, True, clamps=cnt)
    assert cnt["llr"] == int((np.abs(L) > 4.0).sum()) > 0 and cnt["q"] > 0
    assert np.abs(P).max() <= 8.0 + LN2 and np.abs(P).max() > 4.0
    assert 0 < (its < 20).sum() < 67
    wide = {}
    b64 = qc_bp_ref(base, Z, L, 20, 64.0, True, clamps=wide)
    assert wide["llr"] == 0 and not same_bits(b64[2], P)

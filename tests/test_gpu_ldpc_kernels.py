"""Every flooding LDPC kernel instance the planner can pick (csrc/ldpc.hip)
decodes the codes of tests/ldpc_codes.py bit-exactly like the C oracle: hard
decisions and iteration counts equal, no tolerance.

Each case first asserts the kernel it runs (tests/test_ldpc_codes_host.py pins
the same table on the host).  Inputs:
  awgn     all-zero-codeword AWGN frames below the code's waterfall, 50
           iterations.  Without early stop every frame runs all 50, so a
           last-bit difference in a message (a wrong summation order, say) grows
           until decisions differ; the early-stop run adds the iteration counts.
           On widecols (variable degrees up to 128), summing the messages
           sequentially instead of pairwise changes the decisions of 166 (min-sum
           0.75), 201 (min-sum 1.0) and 7 (BP) of these 256 frames at 50
           iterations, of 12, 102 and 0 at 20.
  special  +-0, +-inf, NaN and erased LLRs (ldpc_codes.special_llrs), 20
           iterations.

What these cases found: with the lean tanh(x/2) / 2 atanh of ldpc.hip (<= 4 /
<= 2 ulp) the generic kernel's BP differed from the oracle on widecols in 7 of
the 256 frames (43, 59, 85, 151, 194, 239, 253; with early stop also in one
iteration count), min-sum in none.  They are the 7 frames of the sequential-sum
experiment, and exactly the ones that change when libm's tanh in a scratch copy
of the oracle is replaced by a correctly rounded one: the last bit of tanh
decides them.  ldpc_decode_kernel now evaluates tanh and atanh as libm does,
bit for bit (csrc/libm_exact.hpp), so its BP is the oracle's on any code.
"""
import functools

import numpy as np
import pytest
import torch

import ldpc_codes as C
from ldpc_codes import BP, MS, DEFAULT, GENERIC, REG

pytestmark = pytest.mark.gpu

# min-sum normalizations beyond (1.0, 0.75): 1.25 reaches the compact kernel's instance without
# pre-scaled state on r1500_36; 0.0 and -0.5 are outside (0, 1]
EXTRA_NORMS = {"r1500_36": (1.25, 0.0, -0.5), "irr2048": (1.25, 0.0, -0.5), "diag_deg15": (1.25,),
               "r8194_36": (1.25,), "moved504": (1.25,), "widecols": (1.25,)}
BP_SPECIAL = {("moved504", DEFAULT), ("irr96", DEFAULT), ("widecols", DEFAULT), ("r1000_36", REG)}
SPECIAL_ITER = 20


def _cases():
    out = []
    for (cid, algo, ov) in C.PLANS:
        if cid == "r2048_36":  # the (3,6)-regular min-sum kernel: test_gpu_ldpc.py, and the pitch test below
            continue
        norms = (1.0,) if algo == BP else (1.0, 0.75) + (EXTRA_NORMS.get(cid, ()) if ov == DEFAULT else ())
        for norm in norms:
            for es in (False, True):
                out.append((cid, algo, ov, norm, es, "awgn"))
        if algo == MS:
            for norm in (0.75,) + ((1.25,) if cid == "r1500_36" else ()):
                for es in (False, True):
                    out.append((cid, algo, ov, norm, es, "special"))
        elif (cid, ov) in BP_SPECIAL:
            for es in (False, True):
                out.append((cid, algo, ov, 1.0, es, "special"))
    return out


def _id(case):
    cid, algo, ov, norm, es, inputs = case
    return "%s-%s-%s-%g-%s-%s" % (cid, "ms" if algo else "bp", C.OVERRIDE_ENV[ov] or "default", norm,
                                  "es" if es else "noes", inputs)


def _inputs(cid, inputs):
    return (C.awgn_llrs(cid), C.MAX_ITER) if inputs == "awgn" else (C.special_inputs(cid), SPECIAL_ITER)


@functools.lru_cache(maxsize=None)
def _oracle(cid, algo, norm, es, inputs):
    """The oracle's (bits, iterations), computed once per input and decoder
    setting and shared by the kernel overrides; read only."""
    from oracle import oracle as O
    H, rp, ci = C.code(cid)
    llr, max_iter = _inputs(cid, inputs)
    bits, its = O.ldpc_decode(rp, ci, H.shape[1], llr, "ms" if algo else "bp", max_iter, es, norm, threads=16)
    bits.setflags(write=False)
    its.setflags(write=False)
    return bits, its


def _decoder(cid, algo, norm, es, max_iter):
    import polarcode_and_ldpc_amd.ldpc as L
    H = C.code(cid)[0]
    return L.MSDecoder(H, max_iter, norm, es) if algo == MS else L.BPDecoder(H, max_iter, es)


def _assert_plan(dec, cid, algo, ov):
    want = C.PLANS[(cid, algo, ov)]
    assert dec.plan.info.reserved == want["kernel"]
    if "lds" in want:
        assert dec.plan.info.lds_bytes == want["lds"]
    if want["kernel"] == 1:  # generic kernel: state in LDS (all of it) or in the workspace
        E = len(C.code(cid)[2])
        assert (dec.plan.workspace_bytes(1) == 16 * E) == bool(want["use_global"])
        assert (dec.plan.info.lds_bytes >= 16 * E) != bool(want["use_global"])


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_kernel_vs_oracle(gpu, oracle, monkeypatch, case):
    cid, algo, ov, norm, es, inputs = case
    if C.OVERRIDE_ENV[ov]:
        monkeypatch.setenv("PL_LDPC_KERNEL", C.OVERRIDE_ENV[ov])
    else:
        monkeypatch.delenv("PL_LDPC_KERNEL", raising=False)
    llr, max_iter = _inputs(cid, inputs)
    dec = _decoder(cid, algo, norm, es, max_iter)
    _assert_plan(dec, cid, algo, ov)
    if dec.plan.info.reserved == 5:  # the instance the case is there for (pick_kernel's predicate, restated)
        assert C.compact_instance(cid, norm) == C.COMPACT_INSTANCE[(cid, norm)]
    want_b, want_i = _oracle(cid, algo, norm, es, inputs)
    if inputs == "awgn":
        # the frames must not converge: at least half run to max_iter in the oracle's early-stop decode
        _, es_iters = _oracle(cid, algo, norm, True, inputs)
        assert 2 * np.count_nonzero(es_iters == max_iter) >= len(es_iters)
        if not es:
            assert np.all(want_i == max_iter)
    got_b, got_i = dec.decode_batch(llr.copy(), return_iterations=True)  # the shared inputs stay read-only
    bad = np.flatnonzero(np.any(got_b != want_b, axis=1))
    bad_i = np.flatnonzero(got_i != want_i)
    print("%s: bits differ in %d, iterations in %d of %d frames" % (_id(case), bad.size, bad_i.size, len(llr)))
    assert bad.size == 0, "bits differ in %d of %d frames (first: %s)" % (bad.size, len(llr), bad[:8])
    assert bad_i.size == 0, "iterations differ in frames %s" % bad_i[:8]


def test_every_kernel_instance_is_covered():
    """The cases above reach every (kernel, variant / instance, algorithm) the
    table of ldpc_codes.py names."""
    seen = set()
    for cid, algo, ov, norm, es, inputs in _cases():
        p = C.PLANS[(cid, algo, ov)]
        inst = C.COMPACT_INSTANCE[(cid, norm)] if p["kernel"] == 5 else (p["reg_variant"], p["use_global"], p["threads"])
        seen.add((p["kernel"], algo, inst, inputs if algo == MS else "awgn"))
    for inputs in ("awgn", "special"):
        for v in (1, 2, 3, 4):
            assert (2, MS, (v, 0, 256), inputs) in seen
        for inst in ("8,0,0", "0,0,0", "8,3,6", "8,3,6,PRE"):
            assert (5, MS, inst, inputs) in seen
        assert {(1, MS, (0, 0, 256), inputs), (1, MS, (0, 1, 1024), inputs)} <= seen
    for v in (1, 2, 3, 4):
        assert {(2, BP, (v, 0, 256), "awgn"), (7, BP, (v, 0, 256), "awgn")} <= seen
    assert {(1, BP, (0, 0, 256), "awgn"), (1, BP, (0, 1, 256), "awgn"), (1, BP, (0, 1, 1024), "awgn")} <= seen


# ---- row pitch > n, row starts 8- but not 16-byte aligned ----

# id: (code, decoder, kernel code, environment)
PITCH = {
    "generic_lds_bp": ("irr96", "bp", 1, {}),
    "generic_global_bp": ("irr2048", "bp", 1, {}),
    "reg_ms": ("r504_36", "ms", 2, {}),
    "grp_bp_fpg1": ("r504_36", "bp", 7, {"PL_BP_FPG": "1"}),
    "grp_bp_fpg2": ("r504_36", "bp", 7, {"PL_BP_FPG": "2"}),
    "compact_ms": ("r1500_36", "ms", 5, {}),
    "ms36": ("r2048_36", "ms", 8, {}),
    "layered": ("r504_36", "lms", 9, {}),
}


@pytest.mark.parametrize("case", sorted(PITCH))
def test_llr_row_pitch(gpu, monkeypatch, case):
    """Every kernel family reads frame f at llr + f * pitch: 9 frames decoded
    from the view X[:, 3:3+n] of a [9, n + 37] tensor (NaN outside the view)
    equal the decode of the view's contiguous copy."""
    import polarcode_and_ldpc_amd.ldpc as L
    cid, kind, kernel, env = PITCH[case]
    monkeypatch.delenv("PL_LDPC_KERNEL", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H = C.code(cid)[0]
    n = H.shape[1]
    dec = (L.BPDecoder(H, C.MAX_ITER) if kind == "bp" else
           L.MSDecoder(H, C.MAX_ITER, 0.75) if kind == "ms" else L.LayeredMSDecoder(H, C.MAX_ITER, 0.75))
    assert dec.plan.info.reserved == kernel
    B = 9
    X = torch.full((B, n + 37), float("nan"), dtype=torch.float64, device=gpu)
    X[:, 3:3 + n] = torch.from_numpy(C.awgn_llrs(cid)[:B].copy())
    view = X[:, 3:3 + n]
    assert view.stride() == (n + 37, 1) and view.data_ptr() % 16 == 8  # n + 37 is odd: every other row start
    dense = view.contiguous()
    out = []
    for x in (dense, view):
        bits = torch.zeros((B, n), dtype=torch.uint8, device=gpu)
        its = torch.zeros((B,), dtype=torch.int32, device=gpu)
        dec.plan.decode(x, bits, its)
        out.append((bits, its))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert int(out[0][1].min()) >= 1  # the iteration counts were written

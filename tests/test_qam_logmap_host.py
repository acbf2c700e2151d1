"""The exact log-MAP demapper, everything that needs no GPU: the NumPy restatement of glibc's expm1 and log1p
(channel/libm_np.py) against the recorded fixture and the live C library, channel.QAMModem's host methods against
the definition written as loops (tests/qam_logmap_ref.py), the properties the definition states, the accuracy
against the a-posteriori LLR in mpmath, the calibration of the LLRs as probabilities, and the harness's option.

The definition: include/polarldpc.h at pl_qam_demap_logmap.  logmap_inputs() and calibration() are what the GPU
tests share (tests/test_gpu_qam_logmap.py)."""
import json
import math

import numpy as np
import pytest

import qam_fading_ref as F
import qam_logmap_ref as LR
import qam_ref as Q
from test_qam_fading_host import fading_inputs
from test_qam_host import bits_view, host_inputs, same_bits
from polarcode_and_ldpc_amd.channel import QAMModem
from polarcode_and_ldpc_amd.channel import libm_np
from polarcode_and_ldpc_amd.channel.qam import sigma_of

MS = Q.MS
SNRS = (-20.0, 3.0, 12.0, 60.0)
needs_glibc = pytest.mark.skipif(not LR.libm_is_the_fixtures(), reason=LR.SKIP_REASON)
# beyond host_inputs' specials (every level, every midpoint -- a tie in D_v --, +-0, +-1e200, +-inf, NaN): the
# largest |r| whose d_a stay finite, and the first ones past it.  At that size r - x_a rounds to r for every
# level, so the d_a of an axis value overflow together: all of them or none.
BIG = [1.3407807929942596e154, -1.3407807929942596e154, 1.3407807929942597e154, -1.5e154]


def modem(m, demapper="maxlog", _cache={}):
    if (m, demapper) not in _cache:
        _cache[m, demapper] = QAMModem(m, demapper=demapper)
    return _cache[m, demapper]


def logmap_inputs(m, E, B, seed=0):
    """host_inputs' y (its specials included) with BIG written behind the specials where the frame has room"""
    bits, y = host_inputs(m, E, B, seed)
    flat = y.reshape(-1)
    n0 = 2 ** (m // 2) * 2 + 6  # host_inputs' specials
    if flat.size >= 2 * n0 + 2 * len(BIG):
        flat[n0:n0 + len(BIG)] = BIG
    return bits, y


def same_up_to_zero_sign(got, want):
    """bit for bit, with max-log's -0.0 allowed to be +0.0"""
    w = want.copy()
    w[w == 0] = 0.0
    return same_bits(got, w)


# ---- the libm restatement ----
@pytest.mark.parametrize("name", ["expm1", "log1p"])
def test_libm_np_equals_the_fixture(name):
    args, want = LR.fixture()[name]
    assert len(args) > 400
    got = getattr(libm_np, name)(args)
    assert got.dtype == np.float64 and np.array_equal(bits_view(got), bits_view(want))
    assert np.array_equal(bits_view(getattr(libm_np, name)(args.reshape(-1, 1))[:, 0]), bits_view(want))


def test_libm_np_specials_and_domain():
    e = libm_np.expm1(np.array([-np.inf, np.nan, -0.0, -1e-320, -800.0]))
    assert e[0] == -1.0 and np.isnan(e[1]) and bits_view(e[2:3])[0] == 1 << 63 and e[3] == -1e-320 and e[4] == -1.0
    l1 = libm_np.log1p(np.array([np.nan, 0.0, 7.0]))
    assert np.isnan(l1[0]) and bits_view(l1[1:2])[0] == 0 and l1[2] == math.log(8.0)
    with pytest.raises(AssertionError):
        libm_np.expm1(np.array([0.5]))
    with pytest.raises(AssertionError):
        libm_np.log1p(np.array([-0.5]))


@needs_glibc
def test_libm_np_equals_the_live_library():
    """10^6 arguments of each, half log-uniform from 2^-60 on and half uniform, over the demapper's ranges"""
    rng = np.random.default_rng(2026)
    n = 500000
    x = np.concatenate([-np.exp(rng.uniform(math.log(2.0 ** -60), math.log(45.0), n)), -rng.uniform(0.0, 40.0, n)])
    want = np.array([math.expm1(v) for v in x])
    assert np.array_equal(bits_view(libm_np.expm1(x)), bits_view(want))
    x = np.concatenate([np.exp(rng.uniform(math.log(2.0 ** -60), math.log(7.0), n)), rng.uniform(0.0, 7.0, n)])
    want = np.array([math.log1p(v) for v in x])
    assert np.array_equal(bits_view(libm_np.log1p(x)), bits_view(want))


# ---- the host methods against the loops ----
@needs_glibc
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("E", [1, 5, 64, 131])
def test_demap_host_equals_the_loops(m, E):
    for B in (1, 5):
        _, y = logmap_inputs(m, E, B)
        for snr in SNRS:
            for dt in (np.float64, np.float32):
                got = modem(m).demap_host(y, E, snr, dtype=dt, method="logmap")
                want = LR.demap(y, E, m, sigma_of(snr), dtype=dt)
                assert same_bits(got, want), (B, snr, dt)
            assert same_bits(modem(m, "logmap").demap_host(y[0], E, snr), LR.demap(y[:1], E, m, sigma_of(snr))[0])


@needs_glibc
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("E", [1, 5, 64, 131])
def test_demap_csi_host_equals_the_loops(m, E):
    S = -(-E // m)
    for B in (1, 5):
        for Lc in sorted({1, 3, S, 2 ** 30}):
            _, h = fading_inputs(m, E, B, Lc)  # H_SPECIALS on its first coefficients
            y = logmap_inputs(m, E, B)[1]
            for snr in SNRS:
                for dt in (np.float64, np.float32):
                    got = modem(m).demap_csi_host(y, h, E, snr, coherence=Lc, dtype=dt, method="logmap")
                    want = LR.demap_csi(y, h, E, m, sigma_of(snr), Lc, dtype=dt)
                    assert same_bits(got, want), (B, Lc, snr, dt)


@pytest.mark.parametrize("m", MS)
def test_nan_where_max_log_has_nan_and_erasures(m):
    E, B = 131, 5
    _, y = logmap_inputs(m, E, B)
    for snr in SNRS:
        ml, lm = modem(m).demap_host(y, E, snr), modem(m).demap_host(y, E, snr, method="logmap")
        assert np.isnan(ml).any() and np.all(np.isnan(lm[np.isnan(ml)]))
        assert np.array_equal(np.isnan(ml), np.isnan(lm))  # and, on these inputs, nowhere else
    yf, h = fading_inputs(m, E, B, 1)
    with np.errstate(over="ignore"):
        g = h[:, 0::2] * h[:, 0::2] + h[:, 1::2] * h[:, 1::2]
    lm = modem(m).demap_csi_host(yf, h, E, 3.0, coherence=1, method="logmap")
    erased = np.repeat(g == 0.0, m, axis=1)[:, :E]
    assert erased.any() and np.all(bits_view(lm)[erased] == 0)


# ---- the properties ----
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_qpsk_equals_max_log(dt):
    for E in (1, 5, 64, 131):
        _, y = logmap_inputs(2, E, 5)
        y2, h = fading_inputs(2, E, 5, 3)
        for snr in SNRS:
            assert same_up_to_zero_sign(modem(2).demap_host(y, E, snr, dtype=dt, method="logmap"),
                                        modem(2).demap_host(y, E, snr, dtype=dt))
            assert same_up_to_zero_sign(modem(2).demap_csi_host(y2, h, E, snr, coherence=3, dtype=dt, method="logmap"),
                                        modem(2).demap_csi_host(y2, h, E, snr, coherence=3, dtype=dt))


def received(m, E, B, snr, seed=0):
    """(bits, y): random bits through modulate_host and NumPy-generator noise at snr"""
    rng = np.random.default_rng(seed + 31 * m)
    bits = rng.integers(0, 2, (B, E), dtype=np.uint8)
    x = modem(m).modulate_host(bits)
    return bits, x + sigma_of(snr) * rng.standard_normal(x.shape)


@pytest.mark.parametrize("m", MS)
def test_at_60_db_equals_max_log(m):
    """received symbols at 60 dB: sigma is 1 / 220 of the level spacing or less, every other level's q is far
    below -56 ln 2, and the correction vanishes"""
    E, B = 1027, 5
    bits, y = received(m, E, B, 60.0)
    for dt in (np.float64, np.float32):
        assert same_up_to_zero_sign(modem(m).demap_host(y, E, 60.0, dtype=dt, method="logmap"),
                                    modem(m).demap_host(y, E, 60.0, dtype=dt))
    S = modem(m).S(E)
    h = np.random.default_rng(m).standard_normal((B, 2 * S)) * F.C
    x = modem(m).modulate_host(bits)
    yf = modem(m).fade_host(x, h, y - x, 1)
    # deep fades are demapped with a small weight: keep the symbols whose own q stay below the threshold
    strong = np.repeat(h[:, 0::2] ** 2 + h[:, 1::2] ** 2 > 0.05, m, axis=1)[:, :E]
    lm = modem(m).demap_csi_host(yf, h, E, 60.0, coherence=1, method="logmap")
    ml = modem(m).demap_csi_host(yf, h, E, 60.0, coherence=1)
    assert strong.mean() > 0.9 and same_up_to_zero_sign(lm[strong], ml[strong])


@pytest.mark.parametrize("m", MS)
def test_unit_gain_equals_the_awgn_demapper(m):
    for E in (1, m + 1, 64, 131):
        _, y = logmap_inputs(m, E, 3)
        y = np.where(np.isfinite(y), y, 0.25)
        S = -(-E // m)
        for Lc in (1, 3, 2 ** 30):
            h = np.zeros((3, 2 * F.blocks(S, Lc)))
            h[:, 0::2] = 1.0
            for snr in SNRS:
                for dt in (np.float64, np.float32):
                    got = modem(m).demap_csi_host(y, h, E, snr, coherence=Lc, dtype=dt, method="logmap")
                    assert same_bits(got, modem(m).demap_host(y, E, snr, dtype=dt, method="logmap")), (E, Lc, snr, dt)


@pytest.mark.parametrize("m", MS)
def test_defaults_reproduce_max_log(m):
    """the constructor's default, method=None and method="maxlog" are today's demapper (held to qam_ref's and
    qam_fading_ref's loops); a logmap modem's method=None is logmap"""
    E, B, snr = 65, 2, 7.5
    _, y = host_inputs(m, E, B)
    y2, h = fading_inputs(m, E, B, 3)
    assert QAMModem(m).demapper == "maxlog" and modem(m, "logmap").demapper == "logmap"
    for dt in (np.float64, np.float32):
        want = Q.demap(y, E, m, sigma_of(snr), dtype=dt)
        want2 = F.demap_csi(y2, h, E, m, sigma_of(snr), 3, dtype=dt)
        for kw in ({}, {"method": None}, {"method": "maxlog"}):
            assert same_bits(QAMModem(m).demap_host(y, E, snr, dtype=dt, **kw), want)
            assert same_bits(QAMModem(m).demap_csi_host(y2, h, E, snr, coherence=3, dtype=dt, **kw), want2)
        assert same_bits(modem(m, "logmap").demap_host(y, E, snr, dtype=dt, method="maxlog"), want)
        assert same_bits(modem(m, "logmap").demap_host(y, E, snr, dtype=dt),
                         modem(m).demap_host(y, E, snr, dtype=dt, method="logmap"))
        assert same_bits(modem(m, "logmap").demap_csi_host(y2, h, E, snr, coherence=3, dtype=dt),
                         modem(m).demap_csi_host(y2, h, E, snr, coherence=3, dtype=dt, method="logmap"))
    if m > 2:
        assert not same_bits(modem(m, "logmap").demap_host(y, E, snr), Q.demap(y, E, m, sigma_of(snr)))


def test_constructor_and_repr():
    assert repr(QAMModem(6)) == "QAMModem(bits_per_symbol=6)"
    assert repr(QAMModem(6, demapper="maxlog")) == "QAMModem(bits_per_symbol=6)"
    assert repr(QAMModem(6, demapper="logmap")) == "QAMModem(bits_per_symbol=6, demapper='logmap')"
    with pytest.raises(AssertionError, match="'exact'"):
        QAMModem(6, demapper="exact")
    with pytest.raises(AssertionError, match="'map'"):
        QAMModem(6).demap_host(np.zeros((1, 2)), 6, 3.0, method="map")
    with pytest.raises(AssertionError, match="'map'"):
        QAMModem(6).demap_csi_host(np.zeros((1, 2)), np.ones((1, 2)), 6, 3.0, method="map")


# ---- accuracy ----
@pytest.mark.parametrize("m", MS)
def test_accuracy_against_mpmath(m):
    """Every LLR within qam_logmap_ref.logmap_bound_mp (its docstring derives the bound from the operation count)
    of log sum_0 e^(-W d_a) - log sum_1 e^(-W d_a) at 100 digits from the same doubles r, x_a, W: levels, midpoints,
    zero and received values at every SNR of the grid; weights w and w g.  The largest error / bound is printed
    (DESIGN.md 4.4e records it)."""
    import mpmath
    table = LR.level_table(m)
    hb = m // 2
    rng = np.random.default_rng(m)
    lev = [xa for xa, _ in table]
    fixed = lev + [(lev[i] + lev[i + 1]) / 2 for i in range(len(lev) - 1)] + [0.0, 2.5, -3.0]
    worst = 0.0
    for snr in SNRS:
        w = 1.0 / (2.0 * (sigma_of(snr) * sigma_of(snr)))
        r = np.array(fixed + (rng.choice(lev, 24) + sigma_of(snr) * rng.standard_normal(24)).tolist())
        y = np.zeros((1, 2 * len(r)))
        y[0, 0::2] = r
        for g in (None, 0.3, 2.7):
            if g is None:
                llr = modem(m).demap_host(y, len(r) * m, snr, method="logmap")
                W = w
            else:
                h = np.zeros((1, 2))
                h[0, 0] = math.sqrt(g)
                g2 = h[0, 0] * h[0, 0]
                yy = y * h[0, 0]
                llr = modem(m).demap_csi_host(yy, h, len(r) * m, snr, coherence=2 ** 30, method="logmap")
                W = w * g2
            for s in range(len(r)):
                rs = r[s] if g is None else (h[0, 0] * yy[0, 2 * s]) / g2
                for p in range(hb):
                    exact = LR.exact_mp(rs, table, p, W)
                    bound = LR.logmap_bound_mp(rs, table, p, W)
                    err = abs(mpmath.mpf(float(llr[0, s * m + 2 * p])) - exact)
                    assert err <= bound, (snr, g, rs, p, float(err), float(bound))
                    worst = max(worst, float(err / bound))
    print("qam logmap m=%d: largest error / bound = %.3f" % (m, worst))


# ---- calibration ----
AWGN_POINTS = [(2, 3.0), (4, 6.0), (6, 10.0), (6, 4.0), (8, 14.0), (8, 8.0)]
RAYLEIGH_POINTS = [(2, 6.0), (4, 10.0), (6, 15.0), (8, 20.0)]


def calibration(llr, bits, m):
    """z [m] of LLRs [n, m] (positive decides 0) against the sent bits [n, m]: (errors - sum p) / sqrt(sum p (1 - p))
    with p = 1 / (1 + e^|L|), the error probability the LLR itself predicts"""
    llr = np.asarray(llr, dtype=np.float64).reshape(-1, m)
    bits = np.asarray(bits).reshape(-1, m)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(np.abs(llr)))
    errors = ((llr < 0) != (bits != 0)).sum(axis=0)
    return (errors - p.sum(axis=0)) / np.sqrt((p * (1.0 - p)).sum(axis=0))


def _calibrate_host(m, snr, fading):
    n, chunk = 1 << 20, 1 << 16
    rng = np.random.default_rng(1000 * m + int(10 * snr) + (7 if fading else 0))
    out = {"logmap": [], "maxlog": []}
    sent = []
    for _ in range(n // chunk):
        bits = rng.integers(0, 2, (1, chunk * m), dtype=np.uint8)
        x = modem(m).modulate_host(bits)
        noise = sigma_of(snr) * rng.standard_normal(x.shape)
        sent.append(bits)
        if fading:
            h = rng.standard_normal(x.shape) * F.C
            y = modem(m).fade_host(x, h, noise, 1)
        for method in out:
            if fading:
                out[method].append(modem(m).demap_csi_host(y, h, chunk * m, snr, coherence=1, method=method))
            else:
                out[method].append(modem(m).demap_host(x + noise, chunk * m, snr, method=method))
    sent = np.concatenate(sent, axis=1)
    return {k: calibration(np.concatenate(v, axis=1), sent, m) for k, v in out.items()}


@pytest.mark.parametrize("m,snr", AWGN_POINTS)
def test_calibration_awgn(m, snr):
    """2^20 symbols: the log-MAP LLR predicts its own error rate within 5 standard errors at every bit position;
    max-log on the same symbols is off by more than 10 at every position of m >= 4 (the test can see a missing or
    wrongly signed correction)"""
    z = _calibrate_host(m, snr, False)
    print("m=%d AWGN %.0f dB: z logmap %s, maxlog %s" % (m, snr, np.round(z["logmap"], 2), np.round(z["maxlog"], 1)))
    assert np.all(np.abs(z["logmap"]) <= 5), z["logmap"]
    if m >= 4:
        assert np.all(np.abs(z["maxlog"]) > 10), z["maxlog"]


@pytest.mark.parametrize("m,snr", RAYLEIGH_POINTS)
def test_calibration_rayleigh(m, snr):
    """fast Rayleigh fading (Lc = 1), h = C (g0, g1) from NumPy normals, channel state at the demapper"""
    z = _calibrate_host(m, snr, True)
    print("m=%d Rayleigh %.0f dB: z logmap %s, maxlog %s" % (m, snr, np.round(z["logmap"], 2), np.round(z["maxlog"], 1)))
    assert np.all(np.abs(z["logmap"]) <= 5), z["logmap"]


# ---- the harness ----
def test_cli_demapper_with_cpu_stub(capsys, tmp_path):
    from polarcode_and_ldpc_amd.harness import ber
    common = ["--cpu-stub", "--snr=0:1:1", "--frames", "64", "--batch", "32"]
    with pytest.raises(SystemExit):
        ber.main(common + ["--demapper", "logmap"])  # needs --modulation
    assert "--demapper needs --modulation" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ber.main(common + ["--modulation", "64qam", "--demapper", "exact"])
    capsys.readouterr()
    keys, results = [], []
    for i, extra in enumerate((["--demapper", "logmap"], ["--demapper", "maxlog"], [])):
        path = tmp_path / ("stub%d.jsonl" % i)
        ber.main(common + ["--modulation", "64qam", "--log", str(path)] + extra)
        results.append(json.loads(capsys.readouterr().out.strip().splitlines()[-1])["points"])
        keys.append(json.loads(path.read_text().splitlines()[0])["key"])
    assert keys[0].get("demapper") == "logmap" and "demapper" not in keys[1] and keys[1] == keys[2]
    assert results[0] == results[1] == results[2]
    path = tmp_path / "plain.jsonl"
    ber.main(common + ["--log", str(path)])
    capsys.readouterr()
    assert json.loads(path.read_text().splitlines()[0])["key"] == keys[2]


def test_run_key_helper():
    from polarcode_and_ldpc_amd.harness.ber import _demapper_key
    assert _demapper_key(QAMModem(6)) == {} and _demapper_key(QAMModem(6, demapper="logmap")) == {"demapper": "logmap"}

"""The host side of tests/test_gpu_ldpc_layered_shapes.py (no GPU): the geometry
columns of tests/layered_shapes.py, computed from the text of lms_geom, against
the planner through pl_debug_ldpc_layered_plan_probe; the two restatements
against each other on an expanded H; the conditions every builder's frames are
there for; and what the case tables reach."""
import numpy as np
import pytest

import layered_shapes as S
from layered_ref import layered_ms_ref


def _irregular_probe(name, force_global=0):
    H, layers, _ = S.irregular_case(name)
    rp, ci = S.L().dense_to_csr(H)
    return S.probe(rp, ci, S.IRR_N, layers, S.IRR_ITER, force_global)


def _probe_of(case):
    kind, _, key = case.partition("_")
    if kind == "width":
        z, _, glob = key.partition("_")
        return S.qc_probe(S.width_base(int(z)), int(z), S.WIDTH_ITER, 1 if glob else 0)
    if kind == "ladder":
        return S.qc_probe(S.ladder_base(int(key)), S.LADDER_Z, S.LADDER_ITER)
    if kind == "edge":
        return S.qc_probe(S.L().qc_random_base(5, 10, int(key), 3, seed=7), int(key), S.EDGE_ITER)
    if kind == "pack":
        base, Z, max_iter, _ = S.pack_case(key)
        return S.qc_probe(base, Z, max_iter)
    assert kind == "irregular"
    return _irregular_probe(key)


@pytest.mark.parametrize("case", sorted(S.all_geometries()))
def test_geometry_tables_equal_the_planner(case):
    p = _probe_of(case)
    assert S.geometry(p) == S.all_geometries()[case]
    assert p.kernel == (10 if p.use_global else 9)
    assert p.lds_bytes <= 160 * 1024


def test_planner_edges_are_edges():
    """The ladder's neighbours sit on both sides of 65536 / fpb and of the 160 KB of LDS; the block edge
    on both sides of 160 KB less the 128 vote bytes."""
    g = S.LADDER
    for hi, lo, fpb in ((22, 23, 4), (32, 33, 3), (54, 55, 2)):
        assert g[hi]["fpb"] == fpb and g[lo]["fpb"] == fpb - 1
        assert 65536 // g[hi]["state"] == fpb and 65536 // g[lo]["state"] == fpb - 1
        assert g[lo]["state"] - g[hi]["state"] == 512  # one block column of 64 posteriors
    assert g[310]["state"] == 160 * 1024 and g[311]["state"] == 160 * 1024 + 512
    assert (g[310]["use_global"], g[311]["use_global"]) == (0, 1)
    e = S.BLOCK_EDGE
    assert e[909]["state"] + 128 <= 160 * 1024 < e[910]["state"] + 128 and e[910]["state"] < 160 * 1024
    assert (e[909]["use_global"], e[910]["use_global"]) == (0, 1)


def test_irregular_codes():
    for name, m, widest in (("block", 122, 70), ("wave", 112, 60)):
        H, layers, _ = S.irregular_case(name)
        assert H.shape == (m, S.IRR_N) and [len(l) for l in layers] == [40, 0, 0, 3, widest, 1, 8]
        assert sorted(np.concatenate(layers).tolist()) == list(range(m))
        for l in layers:
            assert H[l].sum(axis=0).max(initial=0) <= 1  # a layer's rows share no column
        assert H.sum(axis=1)[layers[0]].tolist() == S.IRR_LAYERS[name][0]
        p = _irregular_probe(name)
        assert (p.maxdc, p.n_layers, p.max_layer, p.mw) == (255, 7, widest, 9)
        assert _irregular_probe(name, 1).use_global == 1


@pytest.mark.parametrize("Z", [65, 1025])
@pytest.mark.parametrize("early_stop", [True, False])
def test_the_two_restatements_agree(Z, early_stop):
    """qc_layered_ms_ref from the base matrix and layered_ms_ref on the expanded H with the block rows as
    layers: bits, iteration counts and posteriors, on the frames of a."""
    base, llr = S.width_base(Z), S.width_llr(Z)
    a = S.width_want(Z, early_stop)
    b = layered_ms_ref(S.L().qc_expand(base, Z), llr, S.L().qc_block_layers(2, Z), S.WIDTH_ITER, S.NORM, early_stop)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2], equal_nan=True)
    if early_stop:
        assert a[1].min() < S.WIDTH_ITER and a[1].max() == S.WIDTH_ITER


def test_the_two_restatements_agree_on_crafted_frames():
    """... and on c.'s frames at degree 17: the minimum, the NaN and the zeros at the last position."""
    base, Z, max_iter, llr = S.pack_case("deg17")
    a = S.pack_want("deg17", False)
    b = layered_ms_ref(S.L().qc_expand(base, Z), llr, S.L().qc_block_layers(3, Z), max_iter, S.NORM, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2], equal_nan=True) and np.isnan(a[2]).any()


@pytest.mark.parametrize("early_stop", [True, False])
def test_builders_hold_their_conditions(early_stop):
    """Every expectation the GPU file compares against is built (the builders assert the mix of iteration
    counts, the crafted positions and the NaN posteriors) and has the shape of its frames."""
    for Z in S.WIDTHS:
        want = S.width_want(Z, early_stop)
        assert want[2].shape == S.width_llr(Z).shape == (5 + (Z == 1024), 4 * Z)
        assert S.width_batches(Z) == ([1, 5, 6] if Z == 1024 else [1, 5])
    for nb in S.LADDER:
        assert S.ladder_want(nb, early_stop)[2].shape == (9, 64 * nb)
        assert S.ladder_batches(nb) == sorted({1, S.LADDER[nb]["fpb"], S.LADDER[nb]["fpb"] + 1, 9})
    for Z in S.BLOCK_EDGE:
        assert S.edge_want(Z, early_stop)[2].shape == (3, 10 * Z)
    for name in S.PACKS:
        assert S.pack_want(name, early_stop)[0].shape == S.pack_case(name)[3].shape
    for name in S.IRREGULAR:
        assert S.irregular_want(name, early_stop)[2].shape == (11, S.IRR_N)


def test_chunk_cases_differ_across_chunks():
    for name in S.CHUNKED:
        _, llr, want = S.chunk_case(name)
        assert len(llr) == S.CHUNK_FRAMES == 13 and want[2].dtype == llr.dtype
        S.chunks_differ(want, int(want[1].max()))
    llr, want = S.chunk_ladder_case()
    assert len(llr) == S.CHUNK_LADDER[2] and S.LADDER[S.CHUNK_LADDER[0]]["use_global"] == 1


def test_every_instance_and_regime_is_covered():
    """From the case tables alone (the first test holds them against the planner): all four (WAVE, GLOBAL)
    instances of ldpc_layered_kernel, every rung of the frames-per-workgroup ladder, the smallest and the
    largest workgroups with one, two and three trips of the layer loop, and every meta-word count the
    packing edges are there for."""
    rows = list(S.all_geometries().values())
    assert {(g["wave"], g["use_global"]) for g in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {g["fpb"] for g in rows if g["wave"] and not g["use_global"]} == {1, 2, 3, 4}
    assert {64, 128, 1024} <= {g["threads"] for g in rows}
    assert {g["trips"] for g in rows if g["threads"] == 1024 and not g["use_global"]} == {1, 2, 3}
    assert (1024, 2) in {(g["threads"], g["trips"]) for g in rows if g["use_global"]}
    assert {1, 2, 3, 4, 9, 65} <= {g["mw"] for g in rows}
    # the chunked decodes reach both mappings of the generic kernel on the workspace and the three QC decoders
    assert {(c.get("wave"), c.get("use_global")) for c in S.CHUNKED.values()} >= {(1, 1), (0, 1)}
    assert {c.get("reserved") for c in S.CHUNKED.values()} >= {12, 14, 16}

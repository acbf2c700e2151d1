"""The host side of tests/test_gpu_ldpc_qc_fixed_shapes.py (no GPU): the geometry
columns of tests/qc_fixed_shapes.py, computed from the text of qc_fixed_plan_build
and qc_map, against the planner through pl_debug_ldpc_qc_fixed_plan_probe; the
conditions every builder's frames are there for, on the restatement
(tests/qc_fixed_ref.py); and what the case tables reach."""
import numpy as np
import pytest

import qc_fixed_shapes as S
from qc_layered_ref import block_row_vars

GEOMETRIES = S.all_geometries


@pytest.mark.parametrize("case", sorted(["lift_%d" % z for z in S.LIFT] + ["stuck_%d" % z for z in S.STUCK_R] + ["d32"] +
                                        ["edge_" + k for k in S.EDGES] + ["pack_" + k for k in S.PACK] + ["rate_" + k for k in S.RATE]))
def test_geometry_tables_equal_the_planner(case):
    """(kernel, dcap, mw, fpw, fpb, threads, lds_bytes, use_global, state_bytes) of every row."""
    base, Z, max_iter, p, row = GEOMETRIES()[case]
    got = S.probe(base, Z, max_iter, p)
    assert S.geometry(got) == row
    assert got.kernel == 15 + got.use_global and got.lds_bytes <= S.LDS_MAX
    assert (got.norm16, got.llr_max, got.msg_max) == (p["norm16"], p["llr_max"], p["msg_max"])
    assert got.off_p == 4 * np.asarray(base).shape[0] * Z * got.mw  # P behind the check words
    assert got.maxdc == (np.asarray(base) >= 0).sum(axis=1).max()


def test_the_parametrised_names_are_the_tables():
    assert len(GEOMETRIES()) == len(S.LIFT) + len(S.STUCK_R) + 1 + len(S.EDGES) + len(S.PACK) + len(S.RATE)
    assert sorted(S.STUCK_R) == [z for z in sorted(S.LIFT) if z > 64]


def test_frames_per_workgroup_and_lds_of_the_4_8_plans():
    """Frames per workgroup and dynamic LDS of the (4, 8) plans, their pools and batches."""
    assert [S.fpg(z) for z in sorted(S.LIFT)] == [128, 84, 8, 4, 4, 1, 1, 1, 1, 1]
    assert [S.LIFT[z]["lds"] for z in sorted(S.LIFT)] == [6144, 6720, 6144, 3200, 6080, 1696, 3200, 9344, 24128, 24704]
    assert [len(S.z_pool(z)) for z in sorted(S.LIFT)] == [129, 85, 9, 5, 5, 16, 16, 9, 9, 9]
    assert S.z_batches(2) == [1, 127, 129] and S.z_batches(33) == [1, 3, 5] and S.z_batches(384) == [1, 2, 9]
    # the stop mask of frame f of a wavefront is shifted by f Z bits: past bit 31 at Z = 2, 3 and 32
    assert [(S.LIFT[z]["fpw"] - 1) * z for z in (2, 3, 32)] == [62, 60, 32]
    # 33, 63: one frame a wavefront and idle lanes behind it; block mapping: 2, 2, 6, 16, 16 wavefronts
    assert [S.LIFT[z]["fpw"] for z in (33, 63)] == [1, 1]
    assert [S.LIFT[z]["threads"] // 64 for z in (65, 128, 384, 1000, 1024)] == [2, 2, 6, 16, 16]


def test_planner_edges_are_edges():
    """Every pair sits on both sides of the 160 KB of LDS (less the 128 vote bytes in the block mapping); the
    ladder's neighbours on both sides of 65536 / fpb."""
    E = {k: v[5] for k, v in S.EDGES.items()}
    for pair in ("block_1w", "block_2w"):
        lds, ws = E[pair + "_lds"], E[pair + "_ws"]
        assert lds["state"] + 128 == lds["lds"] == 163808 <= S.LDS_MAX < ws["state"] + 128 and ws["lds"] == 128
        assert (lds["kernel"], ws["kernel"]) == (15, 16) and lds["mw"] == ws["mw"] == (1 if pair == "block_1w" else 2)
        assert lds["threads"] == ws["threads"] == 1024
    assert (E["block_1w_lds"]["dcap"], E["block_2w_lds"]["dcap"]) == (8, 32)
    for pair in ("subwave", "z1"):
        lds, ws = E[pair + "_lds"], E[pair + "_ws"]
        assert lds["state"] * lds["fpw"] == lds["lds"] == S.LDS_MAX < ws["state"] * ws["fpw"] and ws["lds"] == 0
        assert (lds["kernel"], lds["fpb"], ws["kernel"], ws["fpb"]) == (15, 1, 16, 4)
    assert (E["subwave_lds"]["state"], E["z1_lds"]["state"], E["z1_ws"]["state"]) == (81920, 2560, 2576)
    assert [E["fpb_%d" % nb]["fpb"] for nb in (128, 129, 213, 214, 384, 385)] == [4, 3, 3, 2, 2, 1]
    for hi, lo, fpb in ((128, 129, 4), (213, 214, 3), (384, 385, 2)):
        a, b = E["fpb_%d" % hi], E["fpb_%d" % lo]
        assert 65536 // (2 * a["state"]) == fpb and 65536 // (2 * b["state"]) == fpb - 1
        assert b["state"] - a["state"] == 32  # one block column of 32 byte-wide posteriors
        assert a["lds"] == 2 * a["state"] * fpb and b["lds"] == 2 * b["state"] * (fpb - 1)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("Z", sorted(S.LIFT))
def test_lifting_size_frames_hold_their_conditions(Z, early_stop):
    """The pools hold frames that stop early and frames that run all 20 iterations, in every batch above one
    frame and, for Z <= 32, within the first wavefront; the stuck frame of Z > 64 never stops at llr_max = 127,
    and its unsatisfied checks after iteration 1 sit at index r or above."""
    want = S.z_want(Z, early_stop)
    assert want[2].shape == S.z_pool(Z).shape == (len(S.z_pool(Z)), 8 * Z) and want[2].dtype == np.int8
    assert np.abs(S.z_pool(Z)[:-1].astype(np.int64)).max() <= 31
    if Z > 64:
        r = S.stuck_frame(Z)[1]
        stuck = S.stuck_want(Z, early_stop)
        assert stuck[1][-1] == S.Z_ITER and r == S.STUCK_R[Z] and r >= 64 * (Z >= 128) and (Z < 384 or r >= 256)
        # the other frames never reach the input clamp: the two settings differ in the stuck frame alone
        assert all(np.array_equal(a[:-1], b[:-1]) for a, b in zip(want, stuck))


def test_z1024_degree_32_frames():
    base, llr = S.d32_case()
    assert (base >= 0).sum(axis=1).tolist() == S.D32["degrees"] and llr.shape == (3, 32 * 1024)
    want = S.d32_want()
    assert want[1].min() < S.D32["max_iter"] and want[1].max() == S.D32["max_iter"]


@pytest.mark.parametrize("name", sorted(S.EDGES))
def test_planner_edge_frames_hold_their_conditions(name):
    deg, mb, nb, Z, frames, _ = S.EDGES[name]
    want = S.edge_want(name)
    assert want[2].shape == (frames, nb * Z)
    if not name.startswith("fpb"):
        assert frames == (65 if Z == 1 else 3)
    assert want[1].min() < S.EDGE_ITER <= 6 and want[1].max() == S.EDGE_ITER


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name", sorted(S.PACK))
def test_packing_frames_hold_their_conditions(name, early_stop):
    """pack_want asserts the six crafted properties on L[V]; here what they mean for the check words."""
    degrees, nb, Z, max_iter, noisy, g = S.PACK[name]
    base, llr = S.pack_case(name)
    want = S.pack_want(name, early_stop)
    assert want[2].shape == llr.shape == (noisy + 6, nb * Z)
    d = degrees[0]
    assert (g["dcap"], g["mw"]) == {8: (8, 1), 14: (16, 1), 16: (16, 2), 32: (32, 2), 33: (0, 3), 64: (0, 3),
                                    65: (0, 4), 2047: (0, 65)}[d]
    V = block_row_vars(np.asarray(base), Z, 0)
    c = {k: llr[noisy + i].astype(np.int64)[V] for i, k in enumerate(S.CRAFTED)}
    # iteration 1, row 0: q = L[V].  idx1 = d - 1 fills its field: 13 in 4 bits, 2046 in 11
    assert (np.abs(c["min_last"]).argmin(axis=1) == d - 1).all()
    # the minima stored for all_127 are 127 x 16 >> 4 = 127, below no clamp
    assert S.FULL["norm16"] == 16 and S.FULL["msg_max"] == 127 and (np.abs(c["all_127"]).min(axis=1) == 127).all()
    # all_negative: parity d mod 2, the last flag word holds (d - 1) % 32 + 1 flags; last_negative: its top one
    assert ((c["all_negative"] < 0).sum(axis=1) % 2 == d % 2).all()
    assert ((c["last_negative"] < 0).sum(axis=1) == 1).all()
    if name == "deg2047":
        assert max_iter == 3 and len(llr) == 6 and Z == 2


@pytest.mark.parametrize("reordered", [True, False])
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name", sorted(S.RATE))
def test_rate_matched_frames_hold_their_conditions(name, early_stop, reordered):
    """rate_want asserts the conditions, in the layer order that keeps the minimum 0 and in the natural
    one; here the shape of the case."""
    base, Z, llr, cw, fillers = S.rate_case(name)
    order, both = S.rate_layer_order(base)
    assert sorted(order) == list(range(base.shape[0])) and order[:len(both)] == both
    assert all(base[i, 0] >= 0 and base[i, 1] >= 0 for i in both)
    assert not any(base[i, 0] >= 0 and base[i, 1] >= 0 for i in order[len(both):])
    assert len(fillers) == Z // 2 + 3 and fillers[-1] == (base.shape[1] - base.shape[0]) * Z - 1
    assert not cw[:, fillers].any() and len(llr) == S.RATE[name][0]
    want = S.rate_want(name, early_stop, reordered)
    assert (want[2][:, fillers] > 0).all() and np.array_equal(want[0][0::2], cw[0::2])
    if early_stop:
        assert (want[1][0::2] < S.RATE_ITER).all() and want[1].max() == S.RATE_ITER
    else:
        assert (want[1] == S.RATE_ITER).all()
    if not reordered:  # the order shows in the posteriors
        assert not np.array_equal(want[2], S.rate_want(name, early_stop, True)[2])


def test_every_instance_and_regime_is_covered():
    """From the case tables alone (the first test holds them against the planner)."""
    rows = [v[4] for v in GEOMETRIES().values()]
    assert {g["kernel"] for g in rows} == {15, 16}
    # every register cap and word count, in LDS; the workspace by the planner's own choice in both mappings
    assert {(g["dcap"], g["mw"]) for g in rows if g["kernel"] == 15} >= {(8, 1), (16, 1), (16, 2), (32, 2), (0, 3), (0, 4)}
    assert {g["lds"] for g in rows if g["kernel"] == 16} == {0, 128}
    assert {g["fpb"] for g in rows if g["kernel"] == 15 and g["fpw"] == 2} == {1, 2, 3, 4}
    assert {g["fpw"] for g in rows} >= {1, 2, 21, 32, 64}
    assert {g["threads"] for g in rows} >= {64, 128, 192, 256, 384, 1024}
    assert max(g["lds"] for g in rows) == S.LDS_MAX and 163808 in {g["lds"] for g in rows}
    assert 65 in {g["mw"] for g in rows}

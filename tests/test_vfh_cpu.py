"""The VFH global descriptor on the host (no GPU): the declarations and bindings, the host type "VFH", the restatement vfh_ref.py
against hand-derived answers, the scenes of vfh_scenes.py against the undecided cap and against a float32 transcription, and stored
308-float rows through the data file."""
import json
import math
import os
import struct

import numpy as np
import pytest

import global_host as gh
import global_ref as gr
import host_binding as hb
import vfh_ref as vr
import vfh_scenes as vs
from test_host_layer import _BoostReader, _cfg, _toy_codebook

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VFH = {"Type": "VFH"}


def gcfg(global_features=VFH, features=None, **voting):
    j = json.loads(_cfg())
    if global_features is not None:
        j["Children"]["GlobalFeatures"] = global_features
    if features is not None:
        j["Children"]["Features"] = features
    j["Children"]["Voting"]["Parameters"].update(voting)
    return json.dumps(j)


# ---- declarations and bindings -----------------------------------------------------------------------------------------------------

def test_the_header_declares_the_entry_and_its_timer():
    text = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    assert "int  ismhip_global_vfh(" in text and '"global_vfh"' in text and "#define ISMHIP_VFH_DIM 308" in text
    assert "features/features_vfh.cpp:27-70" in text


def test_the_entry_is_exported_and_the_abi_version_stays(pkg):
    L = pkg.capi.lib()
    assert "ismhip_global_vfh" in pkg.capi.EXPORTS and L.ismhip_global_vfh is not None
    assert L.ismhip_abi_version() == 4 and callable(pkg.capi.global_vfh)


# ---- the host type -------------------------------------------------------------------------------------------------------------------

def test_vfh_loads_round_trips_and_reports_308():
    m = hb.Model()
    m.config_from_json(gcfg(UseGlobalFeatures=True))
    out = json.loads(m.config_to_json())
    assert out["Children"]["GlobalFeatures"] == VFH and out["Children"]["Voting"]["Parameters"]["UseGlobalFeatures"] is True
    L = hb.lib()
    assert L.ism3d_global_descriptor_length(m.h) == 308
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())
    assert json.loads(m2.config_to_json()) == out and L.ism3d_global_descriptor_length(m2.h) == 308
    m3 = hb.Model()
    m3.config_from_json(gcfg({"Type": "GRSD"}))                       # a pass-through child has no length
    assert L.ism3d_global_descriptor_length(m3.h) == 0


def test_the_shipped_vfh_config_loads_and_differs_from_the_global_one_in_the_child_only():
    j = json.load(open(os.path.join(ROOT, "config", "modelnet10_shot_vfh.ism")))["ObjectConfig"]
    g = json.load(open(os.path.join(ROOT, "config", "modelnet10_shot_global.ism")))["ObjectConfig"]
    assert j["Children"]["GlobalFeatures"] == VFH
    g["Children"]["GlobalFeatures"] = VFH
    assert j == g
    m = hb.Model()
    m.config_from_json(json.dumps(j))
    assert hb.lib().ism3d_global_descriptor_length(m.h) == 308


def test_the_refusal_of_an_unbuilt_global_type_lists_vfh():
    with pytest.raises(hb.HostError) as e:
        hb.Model().config_from_json(gcfg({"Type": "GRSD"}, UseGlobalFeatures=True))
    assert '"GRSD"' in str(e.value) and "SHORT_SHOT_GLOBAL, SHOT_GLOBAL, VFH" in str(e.value)


def test_vfh_as_the_local_features_child_is_still_refused():
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: .*SpinImage, RSD, CoSPAIR\)"):
        hb.Model().config_from_json(gcfg(None, features={"Type": "VFH", "Parameters": {}}))


def test_stored_308_float_rows_round_trip_through_the_data_file(tmp_path):
    """Voting::iSaveData's field order read back with struct.unpack, as test_global_cpu.py does for 32-float rows"""
    rng = np.random.default_rng(18)
    cb = _toy_codebook(rng)
    cls, inst = [0, 1, 1, 2], [4, 5, 6, 7]
    rf = np.zeros((4, 9), f32); desc = (rng.random((4, 308)) * 100).astype(f32); radius = rng.random(4).astype(f32)
    m = hb.Model()
    m.config_from_json(gcfg(UseGlobalFeatures=True))
    m.set_codebook(cb, 3)
    m.set_dimensions(0, 0.9, 0.5, 0.01, 0.02)
    gh.set_global_features(m, cls, inst, rf, desc, radius)
    path = str(tmp_path / "v.ism")
    m.write(path)
    data = open(str(tmp_path / "v.ismd"), "rb").read()
    m0 = hb.Model()
    m0.config_from_json(gcfg())
    m0.set_codebook(cb, 3)
    m0.set_dimensions(0, 0.9, 0.5, 0.01, 0.02)
    m0.write(str(tmp_path / "v0.ism"))
    at = len(open(str(tmp_path / "v0.ismd"), "rb").read()) - 12                    # where the global features start
    r = _BoostReader(data)
    r.o = at
    assert r.u() == 3
    k = 0
    for c, n_clouds in ((0, 1), (1, 2), (2, 1)):
        assert (r.u(), r.u()) == (c, n_clouds)
        for _ in range(n_clouds):
            assert r.u() == 1
            assert [r.f() for _ in range(9)] == [0.0] * 9
            row = r.vf()
            assert len(row) == 308 and np.array_equal(row, desc[k])
            assert r.f() == radius[k] and r.u() == inst[k]
            k += 1
    assert (r.u(), r.u()) == (0, 0) and r.o == len(data)
    assert data[at:at + 4] == struct.pack("<I", 3)
    m2 = hb.Model()
    m2.read(path)
    g = gh.global_features(m2)
    assert g["desc"].shape == (4, 308) and np.array_equal(g["desc"], desc) and g["cls"].tolist() == cls and g["inst"].tolist() == inst


# ---- the restatement against hand-derived answers ---------------------------------------------------------------------------------------
ORIGIN = f32([0, 0, 0])
NC = f32([0.8, 0.0, 0.6])
P2 = f32([[1, 0, 0], [-1, 0, 0]])
N2 = f32([[0, 0.8, 0.6], [0, 0.8, 0.6]])


def test_a_pair_on_an_axis():
    """c = 0, nc = (0.8, 0, 0.6), p = (1, 0, 0), n = (0, 0.8, 0.6): a1 = 0.8, a2 = 0: no swap, u = nc. f3 = 0.8 -> 45 * 0.9 = 40.5: bin 40.
    v = d x u = (0, -0.6, 0) -> (0, -1, 0); w = u x v = (0.6, 0, -0.8); f2 = v . n = -0.8 -> 4.5: bin 4; x = u . n = 0.36, y = w . n = -0.48,
    f1 = atan2(-0.48, 0.36) = -0.92730 -> 45 * (f1 + pi) / 2 pi = 15.86: bin 15; f4 = 1 -> 100.5, clamped to 44.
    The mirror point (-1, 0, 0): a1 = -0.8; f3 -> 4.5: bin 4; v = (0, 1, 0), w = (-0.6, 0, 0.8): f2 = 0.8: bin 40, f1 = +0.92730 -> 29.14: bin 29"""
    out = vr.vfh_counts(P2, N2, ORIGIN, NC, viewpoint=(0, 0, 5))
    want = np.zeros(308, np.int64)
    for b in (15, 45 + 4, 90 + 40, 135 + 44, 29, 45 + 40, 90 + 4):
        want[b] += 1
    want[135 + 44] += 1
    want[180 + 102] = 2                      # d = (0, 0, 1): n . d = 0.6 -> 0.8 * 128 = 102.4
    assert out["m"] == 2 and out["undecided"] == 0
    for k in ("counts", "lower", "upper"):
        assert np.array_equal(out[k], want), k
    t = vr.pairs64(P2, N2, ORIGIN, NC)["t"]
    assert abs(t[0, 0] - 45 * (math.atan2(-0.48, 0.36) + math.pi) / (2 * math.pi)) < 1e-5 and abs(t[0, 1] - 4.5) < 1e-5 and abs(t[0, 2] - 40.5) < 1e-5
    b32 = vr.pairs32(P2, N2, ORIGIN, NC)
    assert b32["bins"].tolist() == [[15, 4, 40, 44], [29, 40, 4, 44]] and not b32["reject"].any()


def test_the_roles_swap_when_the_points_cosine_is_the_larger():
    """nc = (0, 0, 0.5) (not normalised), p = (1, 0, 0), n = (0.6, 0.8, 0): a1 = 0, a2 = 0.6: swap: source p with u = n, target nc, d = (-1, 0, 0).
    f3 = -0.6 -> 45 * 0.2 = 9 exactly: an edge, undecided between bins 8 and 9. v = d x u = (0, 0, -0.8) -> (0, 0, -1): f2 = v . nc = -0.5 ->
    45 * 0.25 = 11.25: bin 11; x = u . nc = 0, y = w . nc = 0: the pole, all 45 bins of f1 are candidates"""
    out = vr.vfh_counts(f32([[1, 0, 0], [1, 0, 0]]), f32([[0.6, 0.8, 0], [0.6, 0.8, 0]]), ORIGIN, f32([0, 0, 0.5]))
    assert out["undecided"] == 2 and out["shape_undecided"] == 2
    assert out["lower"][45 + 11] == 2 and out["upper"][45 + 11] == 2
    assert out["lower"][:45].sum() == 0 and (out["upper"][:45] == 2).all()
    assert out["lower"][90:135].sum() == 0 and out["upper"][90 + 8] == 2 and out["upper"][90 + 9] == 2 and out["upper"][90:135].sum() == 4


def test_the_distance_block_is_zero_by_default_and_filled_with_the_flag():
    counts = vr.vfh_counts(P2, N2, ORIGIN, NC)["counts"]
    row, filled = vr.row_of_counts(counts, 2), vr.row_of_counts(counts, 2, fill_size_component=True)
    assert counts[135:180].sum() == 2 and (row[135:180] == 0).all() and filled[135 + 44] == 200.0
    assert np.array_equal(np.delete(row, np.s_[135:180]), np.delete(filled, np.s_[135:180]))


def test_shape_blocks_divide_by_m_minus_one_and_the_viewpoint_block_by_m():
    """three points (one with a NaN normal does not count): m = 3: 100 / 2 = 50 per shape deposit, float(100 / 3) per viewpoint deposit"""
    P = f32([[1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 5, 0]])
    N = f32([[0, 0.8, 0.6], [0, 0.8, 0.6], [0, 0.8, 0.6], [np.nan, 0, 0]])
    out = vr.vfh_counts(P, N, ORIGIN, NC, viewpoint=(0, 0, 5))
    assert out["m"] == 3
    row = vr.row_of_counts(out["counts"], out["m"])
    assert row[15] == 100.0 and row[29] == 50.0 and row[45 + 4] == 100.0
    assert row[180 + 102] == f32(3.0 * f64(f32(100.0 / 3.0))) and row[180:].sum() == row[180 + 102]
    assert abs(float(row[:45].sum()) - 150.0) < 1e-4                  # PCL's own normalisation: the shape blocks sum to 100 m / (m - 1)


def test_fewer_than_two_normals_give_a_nan_row():
    out = vr.vfh_counts(P2, f32([[0, 0.8, 0.6], [np.inf, 0, 0]]), ORIGIN, NC)
    assert out["m"] == 1 and out["counts"].sum() == 0
    assert np.isnan(vr.row_of_counts(out["counts"], out["m"])).all() and np.isnan(vr.row_of_counts(np.zeros(308), 0)).all()
    nc, m = vr.normal_centroid(f32([[np.nan, 0, 0]]))
    assert m == 0 and np.isnan(nc).all()


def test_a_zero_view_direction_sends_every_viewpoint_deposit_to_bin_64():
    assert np.array_equal(vr.view_direction(ORIGIN, (0, 0, 0)), ORIGIN)
    out = vr.vfh_counts(P2, N2, ORIGIN, NC, viewpoint=(0, 0, 0))
    assert out["counts"][180 + 64] == 2 and out["counts"][180:].sum() == 2 and out["vp_undecided"] == 0
    d = vr.view_direction(f32([0, 0, 2]), (0, 0, 0))
    assert np.array_equal(d, f32([0, 0, -1]))


def test_a_point_at_the_centroid_is_rejected_but_deposits_in_the_viewpoint_block():
    out = vr.vfh_counts(f32([[0, 0, 0], [1, 0, 0], [-1, 0, 0]]), f32([[0, 0, 1]] + N2.tolist()), ORIGIN, NC, viewpoint=(0, 0, 5))
    assert out["m"] == 3 and out["counts"][:180].sum() == 8 and out["counts"][180:].sum() == 3 and out["counts"][180 + 127] == 1
    assert out["total_lower"].tolist() == [2, 2, 2, 2, 3] and out["undecided"] == 0


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
CASES = {c["name"]: c for c in vs.all_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_scenes_keep_within_the_undecided_cap_and_float32_agrees_outside_the_margin(name):
    """per scene at most 1 % of the depositing points undecided, with the centroid and nc taken in float64 and cast; the float32
    transcription never lands outside the float64 candidate bins, and its raw coordinates stay inside the margin"""
    case = CASES[name]
    deposits = undecided = 0
    worst = np.zeros(5)
    for region in case["regions"]:
        p, n = vs.selected(case, region)
        if len(p) == 0:
            continue
        c, _ = gr.centroid_radius(p)
        nc, m = vr.normal_centroid(n)
        out = vr.vfh_counts(p, n, c, nc)
        assert out["m"] == m and (out["lower"] <= out["counts"]).all() and (out["counts"] <= out["upper"]).all()
        if m < 2:
            continue
        deposits += m
        undecided += out["undecided"]
        dis = vr.disagreements(p, n, c, nc)
        assert dis["outside"] == 0, (name, region, dis)
        worst = np.maximum(worst, dis["worst"])
    print(f"{name}: {deposits} depositing points, {undecided} undecided ({100.0 * undecided / max(deposits, 1):.3f} %), "
          f"max |t32 - t64| f1 {worst[0]:.3g} f2 {worst[1]:.3g} f3 {worst[2]:.3g} f4 {worst[3]:.3g} viewpoint {worst[4]:.3g}")
    assert undecided <= 0.01 * deposits
    assert worst.max() <= vr.MARGIN


def test_the_ball_regions_select_exactly_the_sizes_asked_for():
    case = CASES["balls"]
    assert [len(vs.selected(case, r)[0]) for r in case["regions"]] == vs.BALL_SIZES


def test_the_planar_patch_crowds_single_bins():
    case = CASES["plane"]
    p, n = vs.selected(case, case["regions"][0])
    c, _ = gr.centroid_radius(p)
    nc, m = vr.normal_centroid(n)
    assert np.array_equal(nc, n[0])
    out = vr.vfh_counts(p, n, c, nc)
    assert out["counts"][180 + 115] == m and out["counts"][22] == m and out["counts"][45 + 22] == m and out["counts"][90 + 22] == m


def test_the_centred_scene_has_its_centroid_at_the_origin_and_one_rejected_pair():
    case = CASES["centred"]
    p, n = vs.selected(case, case["regions"][0])
    c, _ = gr.centroid_radius(p)
    nc, m = vr.normal_centroid(n)
    assert np.array_equal(c, ORIGIN) and np.linalg.norm(nc) > 0.1
    out = vr.vfh_counts(p, n, c, nc)
    assert vr.pairs64(p, n, c, nc)["reject"].sum() == 1 and out["total_upper"][0] == m - 1 and out["counts"][180:].sum() == m

"""The GASD global descriptor on the host (no GPU): the declarations and bindings, the host type "GASD", the restatement gasd_ref.py
against hand-derived answers, the scenes of gasd_scenes.py against the undecided cap and against a float32 transcription, and stored
984-float rows through the data file.

Before the feature these fail: every test of the header, the exports and the host type (the header has no such entry, EXPORTS no such
names, "GASD" is a pass-through child without a length, the configuration file does not exist, the refusal lists three types) and the
colourless-cloud refusal. The restatement's own tests, the data-file round trip and "GASD as the local Features child is refused" hold
on either side: they pin the reference the GPU tests use and what must not change."""
import json
import os
import struct

import numpy as np
import pytest

import gasd_ref as ga
import gasd_scenes as gs
import global_host as gh
import global_ref as gr
import host_binding as hb
from test_host_layer import _BoostReader, _cfg, _toy_codebook

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GASD = {"Type": "GASD", "Parameters": {"GasdWithColor": True}}
GASD_SHAPE = {"Type": "GASD", "Parameters": {"GasdWithColor": False}}


def gcfg(global_features=GASD, features=None, **voting):
    j = json.loads(_cfg())
    if global_features is not None:
        j["Children"]["GlobalFeatures"] = global_features
    if features is not None:
        j["Children"]["Features"] = features
    j["Children"]["Voting"]["Parameters"].update(voting)
    return json.dumps(j)


# ---- declarations and bindings -----------------------------------------------------------------------------------------------------

def test_the_header_declares_both_entries_the_defines_and_the_timer():
    text = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    assert "int  ismhip_global_gasd(" in text and "int  ismhip_gasd_hue_bins(" in text and '"global_gasd"' in text
    assert "#define ISMHIP_GASD_DIM 984" in text and "#define ISMHIP_GASD_SHAPE_DIM 512" in text
    assert "features/features_gasd.cpp" in text


def test_the_entries_are_exported_and_the_abi_version_stays(pkg):
    L = pkg.capi.lib()
    for name in ("ismhip_global_gasd", "ismhip_gasd_hue_bins"):
        assert name in pkg.capi.EXPORTS and getattr(L, name) is not None
    assert L.ismhip_abi_version() == 4 and callable(pkg.capi.global_gasd) and callable(pkg.capi.gasd_hue_bins)


# ---- the host type -------------------------------------------------------------------------------------------------------------------

def test_gasd_loads_round_trips_and_reports_984_and_512():
    L = hb.lib()
    for child, dim in ((GASD, 984), (GASD_SHAPE, 512)):
        m = hb.Model()
        m.config_from_json(gcfg(child, UseGlobalFeatures=True))
        out = json.loads(m.config_to_json())
        assert out["Children"]["GlobalFeatures"] == child and out["Children"]["Voting"]["Parameters"]["UseGlobalFeatures"] is True
        assert L.ism3d_global_descriptor_length(m.h) == dim
        m2 = hb.Model()
        m2.config_from_json(m.config_to_json())
        assert json.loads(m2.config_to_json()) == out and L.ism3d_global_descriptor_length(m2.h) == dim


def test_a_missing_parameter_gets_the_references_default_true():
    for child in ({"Type": "GASD"}, {"Type": "GASD", "Parameters": {}}):
        m = hb.Model()
        m.config_from_json(gcfg(child, UseGlobalFeatures=True))
        assert hb.lib().ism3d_global_descriptor_length(m.h) == 984


def test_the_shipped_gasd_config_loads_and_differs_from_the_global_one_in_the_child_only():
    j = json.load(open(os.path.join(ROOT, "config", "modelnet10_shot_gasd.ism")))["ObjectConfig"]
    g = json.load(open(os.path.join(ROOT, "config", "modelnet10_shot_global.ism")))["ObjectConfig"]
    assert j["Children"]["GlobalFeatures"] == GASD_SHAPE
    g["Children"]["GlobalFeatures"] = GASD_SHAPE
    assert j == g
    m = hb.Model()
    m.config_from_json(json.dumps(j))
    assert hb.lib().ism3d_global_descriptor_length(m.h) == 512


def test_the_refusal_of_an_unbuilt_global_type_lists_gasd():
    with pytest.raises(hb.HostError) as e:
        hb.Model().config_from_json(gcfg({"Type": "GRSD"}, UseGlobalFeatures=True))
    assert '"GRSD"' in str(e.value) and "SHORT_SHOT_GLOBAL, SHOT_GLOBAL, VFH, GASD" in str(e.value)


def test_gasd_as_the_local_features_child_is_still_refused():
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: .*SpinImage, RSD, CoSPAIR"):
        hb.Model().config_from_json(gcfg(None, features={"Type": "GASD", "Parameters": {}}))


def test_the_host_refuses_a_colourless_cloud_under_gasd_with_colour():
    """on the host, before any device work: training, and detection with UseGlobalFeatures; GasdWithColor false takes the cloud"""
    rng = np.random.default_rng(9)
    xyz = rng.normal(size=(200, 3)).astype(f32)
    nrm = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(f32)
    m = hb.Model()
    m.config_from_json(gcfg(UseGlobalFeatures=True))
    m.add_training(xyz, nrm, 0, 0)
    with pytest.raises(hb.HostError, match="GASD needs coloured point clouds"):
        m.train()
    with pytest.raises(hb.HostError, match="GASD needs coloured point clouds"):
        m.detect_batch(np.array([0, 200], np.uint32), xyz, nrm)


def test_stored_984_float_rows_round_trip_through_the_data_file(tmp_path):
    """Voting::iSaveData's field order read back with struct.unpack, as test_vfh_cpu.py does for 308-float rows"""
    rng = np.random.default_rng(22)
    cb = _toy_codebook(rng)
    cls, inst = [0, 1, 1, 2], [4, 5, 6, 7]
    rf = np.zeros((4, 9), f32); desc = (rng.random((4, 984)) * 100).astype(f32); radius = rng.random(4).astype(f32)
    m = hb.Model()
    m.config_from_json(gcfg(UseGlobalFeatures=True))
    m.set_codebook(cb, 3)
    m.set_dimensions(0, 0.9, 0.5, 0.01, 0.02)
    gh.set_global_features(m, cls, inst, rf, desc, radius)
    path = str(tmp_path / "g.ism")
    m.write(path)
    data = open(str(tmp_path / "g.ismd"), "rb").read()
    m0 = hb.Model()
    m0.config_from_json(gcfg())
    m0.set_codebook(cb, 3)
    m0.set_dimensions(0, 0.9, 0.5, 0.01, 0.02)
    m0.write(str(tmp_path / "g0.ism"))
    at = len(open(str(tmp_path / "g0.ismd"), "rb").read()) - 12                    # where the global features start
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
            assert len(row) == 984 and np.array_equal(row, desc[k])
            assert r.f() == radius[k] and r.u() == inst[k]
            k += 1
    assert (r.u(), r.u()) == (0, 0) and r.o == len(data)
    assert data[at:at + 4] == struct.pack("<I", 3)
    m2 = hb.Model()
    m2.read(path)
    g = gh.global_features(m2)
    assert g["desc"].shape == (4, 984) and np.array_equal(g["desc"], desc) and g["cls"].tolist() == cls and g["inst"].tolist() == inst


# ---- the restatement against hand-derived answers ---------------------------------------------------------------------------------------
ORIGIN = f32([0, 0, 0])
TIE_FRAME = f32([[1, 0, 0], [0, -1, 0], [0, 0, -1]])
# t = (x, -y, -z) / 3. Shape grid, coord = 3 t + 3: (-3, 0, 0) -> cell (0, 3, 3) = 21; (0, 2, 0) -> t.y = -2/3: float32 (-2/3) * 3 rounds
# to -2 exactly, coord 1 -> (3, 1, 3) = 117; (0, -2, 0) -> (3, 5, 3) = 141; (0, 0, 1) -> t.z = -1/3 -> coord 2 -> (3, 3, 2) = 128;
# (0, 0, -1) -> (3, 3, 4) = 130; (3, 0, 0) -> coord 6: the padding cell, dropped.
TIE_SHAPE = [-1, 21, 117, 141, 128, 130]
# Colour grid, coord = 2 t + 2: (-3, 0, 0) -> (0, 2, 2) = cell 10, green: hue 120 -> bin 4; (0, 2, 0) -> 2 - 4/3 = 0.67 -> (2, 0, 2) = 34,
# blue: hue 240 -> bin 8; (0, -2, 0) -> 3.33 -> (2, 3, 2) = 46, grey: hue 0 -> bin 0; (0, 0, 1) -> 1.33 -> (2, 2, 1) = 41, (255, 128, 0): hue
# 60 * 128 / 255 = 30.1 -> bin 1; (0, 0, -1) -> 2.67 -> (2, 2, 2) = 42, cyan: hue 180 -> bin 6; (3, 0, 0) -> coord 4: dropped.
TIE_COLOUR = [-1, 216 + 10 * 12 + 4, 216 + 34 * 12 + 8, 216 + 46 * 12 + 0, 216 + 41 * 12 + 1, 216 + 42 * 12 + 6]


def test_hue_bins_of_hand_computed_colours():
    """pure red 0 -> bin 0; pure green 120 -> 4; pure blue 240 -> 8; a grey: 1 / 0 is not finite, hue 0 -> bin 0; (255, 128, 0): 30.1 -> 1;
    a hue below 0 (max == r, g < b) wraps: (255, 0, 128) -> 60 * (-128 / 255) + 360 = 329.9 -> bin 10"""
    got = ga.hue_bins32(np.array([0xff0000, 0x00ff00, 0x0000ff, 0x777777, 0xff8000, 0xff0080, 0x000000, 0xffffff], np.uint32))
    assert got.tolist() == [0, 4, 8, 0, 1, 10, 0, 0]
    assert ga.hue_bins32(np.array([0x01ff0000], np.uint32)).tolist() == [0]            # bits 24..31 are ignored


def test_the_six_point_scene_by_hand():
    """covariance diag(18, 8, 2): z = -e_z (turned away from the view direction), x = +e_x by the fallback rule (one point on either
    side), y = z cross x = -e_y; max_coord 3. Only the point at +max_coord is lost."""
    fr = ga.frame64(gs.TIE_POINTS, ORIGIN)
    assert np.array_equal(fr["C"], np.diag([18.0, 8.0, 2.0])) and fr["tie"] and not fr["undecided"] and not fr["degenerate"]
    assert (fr["pos"], fr["neg"]) == (1, 1)
    assert np.array_equal(fr["frame"], TIE_FRAME.astype(f64))
    assert ga.max_coord32(gs.TIE_POINTS, ORIGIN, TIE_FRAME) == 3.0 and ga.max_coord64(gs.TIE_POINTS, ORIGIN, TIE_FRAME) == 3.0
    shape, colour = ga.bins32(gs.TIE_POINTS, gs.TIE_COLOURS, ORIGIN, TIE_FRAME, 3.0)
    assert shape.tolist() == TIE_SHAPE and colour.tolist() == TIE_COLOUR
    out = ga.gasd_counts(gs.TIE_POINTS, gs.TIE_COLOURS, ORIGIN, TIE_FRAME, 3.0)
    want = np.zeros(984, np.int64)
    for b in TIE_SHAPE[1:] + TIE_COLOUR[1:]:
        want[b] += 1
    assert (out["lower"] <= want).all() and (want <= out["upper"]).all() and out["n"] == 6
    row = ga.row_of_counts(want, 6)
    assert row.shape == (984,) and row[21] == 20.0 and row.sum() == 200.0       # 100 / 5 per deposit
    short = ga.row_of_counts(want[:512], 6, with_color=False)
    assert short.shape == (512,) and np.array_equal(short[:216], row[:216]) and (short[216:] == 0).all()


def test_a_sign_majority_turns_x():
    """five points, two at x > 0 and three at x < 0 after centring: the negative count is the larger, x is negated"""
    p = f32([[4, 0, 0], [4, 0.5, 0], [-1, 0, 0.1], [-3, -0.5, 0], [-4, 0, -0.1]])
    c, _ = gr.centroid_radius(p)
    fr = ga.frame64(p, c)
    t = (p.astype(f64) - c.astype(f64)) @ fr["frame"][0]
    assert not fr["tie"] and not fr["undecided"] and (t > 0).sum() == 3 and (t < 0).sum() == 2
    assert abs(np.linalg.det(fr["frame"]) - 1) < 1e-12 and fr["frame"][2] @ [0, 0, 1] <= 0


def test_a_two_point_coloured_region_by_hand():
    """(-1, 0, 0) orange and (1, 0, 0) red in the frame of the axes, max_coord 1: the red point sits at +max_coord and is lost from both
    grids; the other lands in shape cell (0, 3, 3) = 21 and colour cell (0, 2, 2) = 10 with hue bin 1; n = 2: 100 per deposit"""
    p, rgba = f32([[-1, 0, 0], [1, 0, 0]]), np.array([0xff8000, 0xff0000], np.uint32)
    out = ga.gasd_counts(p, rgba, ORIGIN, np.eye(3, dtype=f32), 1.0)
    want = np.zeros(984, np.int64)
    want[21] = 1; want[216 + 10 * 12 + 1] = 1
    shape, colour = ga.bins32(p, rgba, ORIGIN, np.eye(3, dtype=f32), 1.0)
    assert shape.tolist() == [21, -1] and colour.tolist() == [337, -1]
    assert (out["lower"] <= want).all() and (want <= out["upper"]).all()
    assert out["total_upper"].tolist() == [2, 2]               # float64 cannot tell coord 6 - 0 from 6: the lost point is a candidate
    row = ga.row_of_counts(want, 2)
    assert row[21] == 100.0 and row[337] == 100.0 and row.sum() == 200.0
    assert np.isnan(ga.row_of_counts(want, 1)).all() and np.isnan(ga.row_of_counts(want, 0, with_color=False)).all()


def test_a_deposit_near_a_face_is_a_candidate_for_both_cells():
    """max_coord 3 and t.x = 1: coord 4.0, on the face between cells 3 and 4; the other point is clear of every face"""
    p = f32([[1, 0.5, 0.5], [-3, 0.5, 0.5]])
    out = ga.gasd_counts(p, None, ORIGIN, np.eye(3, dtype=f32), 3.0, with_color=False)
    a, b = (3 * 6 + 3) * 6 + 3, (4 * 6 + 3) * 6 + 3
    assert out["undecided"] == 1 and out["upper"][a] == 1 and out["upper"][b] == 1 and out["lower"][a] == 0 and out["lower"][b] == 0
    assert out["lower"][21] == 1 and out["total_lower"][0] == 1 and out["total_upper"][0] == 2 and len(out["counts"]) == 512


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
CASES = {c["name"]: c for c in gs.all_cases()}
NO_CAP = ("plane", "ties")            # the plane lies on a face by construction; the six points sit on faces exactly (held bit for bit)


def host_frame(p):
    """what a device would hand the restatement: centroid, frame and max_coord, here from float64 cast to float32"""
    c, _ = gr.centroid_radius(p)
    fr = ga.frame64(p, c)
    frame = fr["frame"].astype(f32)
    return c, fr, frame, ga.max_coord32(p, c, frame)


@pytest.mark.parametrize("name", sorted(CASES))
def test_scenes_keep_within_the_undecided_cap_and_float32_agrees_outside_the_margin(name):
    """per scene at most 1 % of the deposits undecided (the plane is held on its z marginal instead), no region of a non-tie scene
    with an undecided x sign, the float32 transcription never outside the float64 candidates, |coord32 - coord64| below MARGIN"""
    case = CASES[name]
    deposits = undecided = 0
    worst = 0.0
    for region in case["regions"]:
        p, rgba = gs.selected(case, region)
        if len(p) < 2:
            continue
        c, fr, frame, mc = host_frame(p)
        if name != "ties":                                     # two points always tie (one on either side): the fallback rule, decided
            assert not fr["undecided"] and (not fr["tie"] or len(p) == 2), (name, region)
        if not mc > 0:
            assert name == "coincident"
            continue
        axes = (0, 1) if name == "plane" else (0, 1, 2)
        out = ga.gasd_counts(p, rgba, c, frame, mc, axes=axes)
        assert (out["lower"] <= out["counts"]).all() and (out["counts"] <= out["upper"]).all()
        deposits += out["deposits"]; undecided += out["undecided"]
        dis = ga.disagreements(p, rgba, c, frame, mc)
        assert dis["outside"] == 0, (name, region, dis)
        worst = max(worst, dis["worst"])
        shape, colour = ga.bins32(p, rgba, c, frame, mc)
        got = np.bincount(np.concatenate([shape[shape >= 0], colour[colour >= 0]]), minlength=984)
        if name == "plane":
            got = ga.z_marginal(got)
            full = ga.gasd_counts(p, rgba, c, frame, mc)
            print(f"plane: {full['undecided']} of {full['deposits']} deposits undecided with z counted")
            assert full["undecided"] > 0.5 * full["deposits"]
        assert (out["lower"] <= got).all() and (got <= out["upper"]).all(), (name, region)
    print(f"{name}: {deposits} deposits, {undecided} undecided ({100.0 * undecided / max(deposits, 1):.3f} %), max |coord32 - coord64| {worst:.3g} "
          f"(MARGIN {ga.MARGIN:.3g})")
    if name not in NO_CAP or name == "plane":
        assert undecided <= 0.01 * deposits
    assert worst < ga.MARGIN


def test_the_ball_regions_select_exactly_the_sizes_asked_for():
    case = CASES["balls"]
    assert [len(gs.selected(case, r)[0]) for r in case["regions"]] == gs.BALL_SIZES


def test_the_skewed_blob_has_a_clear_majority():
    p, _ = gs.selected(CASES["skewed"], (0, None, None))
    fr = host_frame(p)[1]
    assert min(fr["pos"], fr["neg"]) < 0.45 * len(p) and not fr["degenerate"]


def test_the_facing_pair_is_mirrored_and_z_is_negated_in_exactly_one():
    case = CASES["facing"]
    a, b = (ga.frame64(p, gr.centroid_radius(p)[0]) for p in (gs.selected(case, r)[0] for r in case["regions"]))
    m = np.array([1.0, 1.0, -1.0])
    assert np.abs(b["frame"][0] - a["frame"][0] * m).max() < 1e-6 and np.abs(b["frame"][1] - a["frame"][1] * m).max() < 1e-6
    assert np.abs(b["frame"][2] + a["frame"][2] * m).max() < 1e-6
    assert a["frame"][2][2] < -0.9 and b["frame"][2][2] < -0.9


def test_the_coincident_points_give_no_max_coord():
    case = CASES["coincident"]
    p, _ = gs.selected(case, case["regions"][0])
    assert len(p) == 2 and np.array_equal(p[0], p[1])
    c, fr, frame, mc = host_frame(p)
    assert np.array_equal(c, gs.COINCIDENT) and mc == 0 and (fr["C"] == 0).all()


def test_the_colour_ramp_holds_every_case_of_the_hue_rule():
    rgba = CASES["ramp"]["rgba"][0]
    r, g, b = ((rgba >> 16) & 255).astype(int), ((rgba >> 8) & 255).astype(int), (rgba & 255).astype(int)
    assert ((r == g) & (g == b)).sum() >= 5
    orders = {tuple(np.argsort([x, y, z], kind="stable")) for x, y, z in zip(r, g, b) if len({x, y, z}) == 3}
    assert len(orders) == 6
    assert set(ga.hue_bins32(rgba).tolist()) == set(range(12))
    hues = ga.hue_bins32(np.array([(x << 16) | (y << 8) | z for x, y, z in gs.HUES_30], np.uint32))
    assert all(abs(int(h) - k) <= 1 or {int(h), k} == {0, 11} for k, h in enumerate(hues))
    assert all(c in rgba.tolist() for c in [(x << 16) | (y << 8) | z for x, y, z in gs.HUES_30])

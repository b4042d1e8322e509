"""VoxelGridCulling on the CPU: the restatement tests/culling_ref.py against hand-derived answers, the selection worked by hand, the cap on
undecided keypoints of the generic scenes, and the host's KeypointsVoxelGridCulling configuration (keypoints_voxel_grid_culling.cpp:27-44:
names and defaults) -- parse, round trip, refusals. No GPU is touched."""
import json
import os
import re

import numpy as np
import pytest

import culling_ref as ref
import culling_scenes as scenes
import host_binding as hb
import voxel_ref

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
EXAMPLE = os.path.join(ROOT, "config", "modelnet10_shot_culling.ism")
DEFAULTS = {"LeafSize": float(f32(0.1)), "FilterMethodGeometry": "None", "FilterTypeGeometry": "CutOff", "FilterThresholdGeometry": float(f32(0.005)),
            "FilterMethodColor": "None", "FilterTypeColor": "CutOff", "FilterThresholdColor": float(f32(0.02)), "MaxSimilarColorDistance": float(f32(0.01)),
            "FilterCutoffRatio": 0.5, "DisableFilterInTraining": True, "CombineFilters": "RequireCombinedList", "RefineKeypointPosition": False}


# ---- the restatement against hand answers ---------------------------------------------------------------------------------------------
def test_exact_plane_patch():
    s = scenes.plane_patch()
    kp = np.array([[0.1, 0.1, 0.0]], f32)
    a = ref.scores(s["xyz"], kp, 0.035, geometry="curvature")
    assert a["count"][0] >= 30 and a["geo"][0] == 0.0                      # e3 and the z row of C are exactly 0
    pc = ref.principal_curvatures(s["xyz"], s["normals"], 0.035)
    assert not pc["pc1"].any() and not pc["pc2"].any() and (pc["count"] >= 10).all()   # n_j - n (n . n_j) is exactly 0
    # kpq by hand: every k1, k2 and K is 0, so 0 > FLT_MIN never moves max_k1 / max_K (they stay FLT_MIN) while 0 < FLT_MAX sets min_k2 = min_K = 0;
    # sum K = 0: kpq = 0 + 100 * FLT_MIN + |0| + 10 * FLT_MIN + |0|
    want = f32(f32(f32(100) * ref.FLT_MIN) + f32(f32(10) * ref.FLT_MIN))
    b = ref.scores(s["xyz"], kp, 0.035, geometry="kpq", pc=pc)
    assert b["geo"][0] == want and want > 0


def test_cylinder_strip_closed_form():
    """query at angle 0, n = (1, 0, 0): v_j = (0, sin phi_j, 0), mean 0 by symmetry, so pc2 = 0 and
    pc1 = sum_{j=-m..m} sin^2(j d) / (2 m + 1) = 1 / 2 - sin((2 m + 1) d) / (2 (2 m + 1) sin d)"""
    s = scenes.cylinder_strip()
    radius = 0.1505                                                         # chord 2 sin(phi / 2) < r: |j| <= 15
    pc = ref.principal_curvatures(s["xyz"], s["normals"], radius)
    i = scenes.CYL_HALF
    m, d = 15, scenes.CYL_STEP
    assert pc["count"][i] == 2 * m + 1
    want = 0.5 - np.sin((2 * m + 1) * d) / (2 * (2 * m + 1) * np.sin(d))
    assert abs(pc["pc1_64"][i] - want) <= 1e-6 * want                       # the float32 normals are rounded: 6e-8 relative each
    assert abs(pc["pc2_64"][i]) <= 1e-12 and pc["pc1"][i] == f32(pc["pc1_64"][i])


def test_fewer_than_three_points_is_nan():
    p = np.array([[0, 0, 0], [0.01, 0, 0]], f32)
    g, n, _ = ref.curvature(p, np.array([0.005, 0, 0], f32), 0.1)
    assert n == 2 and np.isnan(g)
    g, n, _ = ref.curvature(np.vstack([p, [[0, 0.01, 0]]]).astype(f32), np.array([0.005, 0, 0], f32), 0.1)
    assert n == 3 and g == 0.0                                              # three points span a plane
    assert np.isnan(ref.kpq(np.zeros(2, f32), np.zeros(2, f32), np.zeros(0, np.int64)))   # an empty ball


def test_two_colour_ball_by_hand(ora):
    cols = np.array([0x00C83C28] * 7 + [0x003C5ABE] * 3, np.uint32)
    lab = ref.lab_table(ora.rgb2lab, cols)
    far = ref.color_distance(lab[0], lab[7:8])[0]
    assert far > 0.05
    score, distant = ref.color_score(lab[0], lab, 0.01)
    assert distant == 3 and score == f32(3) / f32(10)
    score, distant = ref.color_score(lab[0], lab, float(far))               # exactly at MaxSimilarColorDistance: not distant
    assert distant == 0 and score == 0.0
    score, distant = ref.color_score(lab[0], lab, float(np.nextafter(far, f32(0))))
    assert distant == 3
    with np.errstate(all="ignore"):
        assert np.isnan(ref.color_score(lab[0], lab[:0], 0.01)[0])         # 0 / 0


def test_color_distance_formula():
    d = ref.color_distance(np.array([0.5, 0.25, -0.25], f32), np.array([[0.25, 0.5, 0.25], [-3, 3, 3]], f32))
    assert d[0] == f32((0.25 + (0.25 + 0.5) / 2) / 3) and d[1] == 1.0       # clamped


# ---- selection worked by hand ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", scenes.SELECT_CASES, ids=[c["name"] for c in scenes.SELECT_CASES])
def test_selection_by_hand(case):
    r = ref.select(case["g"], case["c"], **case["kw"])
    assert r["keep"].tolist() == case["keep"]
    assert np.array_equal(r["thresholds"], np.asarray(case["thr"], f32), equal_nan=True)


def test_cutoff_index_and_order():
    assert ref.cutoff_index(0.4, 5) == 2 and ref.cutoff_index(scenes.RATIO_BELOW_04, 5) == 1
    assert ref.cutoff_index(float(np.nextafter(f32(1), f32(0))), 5) == 4 and ref.cutoff_index(0.0, 1) == 0
    assert ref.cutoff_index(float(np.nextafter(f32(1), f32(0))), (1 << 24) + 3) == (1 << 24) + 2   # float32(size) rounds up by one: still inside
    assert ref.ascending([np.nan, 1, np.inf, 1, -np.inf, np.nan, -0.0, 0.0]).tolist() == [4, 6, 7, 1, 3, 2, 0, 5]
    mn, mx = ref.minmax([np.nan, 2, -1, 2, -1])
    assert mn == -1 and mx == 2
    mn, mx = ref.minmax([np.nan])
    assert mn == np.inf and mx == -np.inf


# ---- caps -----------------------------------------------------------------------------------------------------------------------------
def test_generic_scenes_have_few_undecided_keypoints():
    total = und = 0
    for k, (n, leaf, _seed) in enumerate(scenes.SCENES):
        s = scenes.scene(k)
        kp = voxel_ref.voxel_ref(s["xyz"], leaf, s["rgba"])["xyz"].astype(f32)
        a = ref.scores(s["xyz"], kp, leaf, geometry="curvature")
        print("scene %d: %d points, %d keypoints, %d undecided, ball %d .. %d" % (k, n, len(kp), a["undecided"].sum(), a["count"].min(), a["count"].max()))
        assert 20 <= len(kp) <= 150
        total += len(kp); und += int(a["undecided"].sum())
    assert und <= 0.01 * total


# ---- host -----------------------------------------------------------------------------------------------------------------------------
def _cfg(keypoints):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Keypoints"] = keypoints
    return json.dumps(j)


def test_type_is_accepted_with_reference_names_and_defaults():
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "VoxelGridCulling"}))                 # refused on the parent commit: "not built (built: VoxelGrid, ISS3D)"
    out = json.loads(m.config_to_json())["Children"]["Keypoints"]
    assert out["Type"] == "VoxelGridCulling" and sorted(out["Parameters"]) == sorted(DEFAULTS) and len(DEFAULTS) == 12
    for k, v in DEFAULTS.items():
        assert out["Parameters"][k] == v, k


def test_config_roundtrips(tmp_path):
    params = {"LeafSize": 0.25, "FilterMethodGeometry": "KPQ", "FilterTypeGeometry": "Threshold", "FilterThresholdGeometry": 0.5,
              "FilterMethodColor": "ColorDistance", "FilterTypeColor": "cutoff", "FilterThresholdColor": 0.125, "MaxSimilarColorDistance": 0.0625,
              "FilterCutoffRatio": 0.75, "DisableFilterInTraining": False, "CombineFilters": "RequireBoth", "RefineKeypointPosition": False}
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "VoxelGridCulling", "Parameters": params}))
    out = json.loads(m.config_to_json())
    assert out["Children"]["Keypoints"] == {"Type": "VoxelGridCulling", "Parameters": params}    # the strings are kept as written
    m2 = hb.Model()
    m2.config_from_json(json.dumps(out))
    assert json.loads(m2.config_to_json()) == out
    path = str(tmp_path / "culling.ism")
    m.write(path)
    m3 = hb.Model()
    m3.read(path, training=True)
    assert json.loads(m3.config_to_json()) == out


def test_shipped_example_loads():
    m = hb.Model()
    m.read(EXAMPLE, training=True)
    out = json.loads(m.config_to_json())["Children"]
    kp = out["Keypoints"]
    assert kp["Type"] == "VoxelGridCulling" and out["Features"]["Type"] == "SHOT"
    assert kp["Parameters"]["FilterMethodGeometry"] == "kpq" and kp["Parameters"]["FilterTypeGeometry"] == "CutOff"
    assert kp["Parameters"]["FilterCutoffRatio"] == 0.5 and kp["Parameters"]["DisableFilterInTraining"] is True


@pytest.mark.parametrize("params,message", [
    ({"FilterMethodGeometry": "gaussian"}, r"gaussian.*unrelated point"),
    ({"FilterMethodGeometry": "Gaussian"}, r"gaussian.*noise"),
    ({"FilterTypeGeometry": "Auto"}, r"auto.*experimental.*zero histogram step"),
    ({"RefineKeypointPosition": True}, r"RefineKeypointPosition.*later change"),
    ({"FilterCutoffRatio": 1.0}, r"FilterCutoffRatio.*\[0, 1\)"),
    ({"FilterCutoffRatio": -0.25}, r"FilterCutoffRatio.*\[0, 1\)"),
    ({"CombineFilters": "requireboth"}, r"CombineFilters.*silently drops every keypoint"),
    ({"CombineFilters": "Union"}, r"CombineFilters.*silently drops every keypoint"),
    ({"LeafSize": 0.0}, r"LeafSize.*positive"),
    ({"LeafSize": -0.1}, r"LeafSize.*positive"),
    ({"FilterMethodGeometry": "harris"}, r"FilterMethodGeometry.*built: none, curvature, kpq"),
    ({"FilterMethodColor": "hue"}, r"FilterMethodColor.*built: none, colordistance"),
    ({"FilterTypeColor": "auto"}, r"FilterTypeColor.*built: cutoff, threshold"),
])
def test_refusals_by_message(params, message):
    m = hb.Model()
    with pytest.raises(hb.HostError) as e:
        m.config_from_json(_cfg({"Type": "VoxelGridCulling", "Parameters": params}))
    assert re.search(message, str(e.value), re.S), str(e.value)


def test_other_unbuilt_types_stay_refused():
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"keypoint type \"Harris3D\" is not built \(built: VoxelGrid, ISS3D, VoxelGridCulling\)"):
        m.config_from_json(_cfg({"Type": "Harris3D"}))


def test_header_and_exports_list_the_three_entries(pkg):
    header = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    for name in ("ismhip_principal_curvatures", "ismhip_culling_scores", "ismhip_culling_select"):
        assert re.search(r"\bint\s+%s\(" % name, header) and name in pkg.capi.EXPORTS
    for timer in ("culling_pc", "culling_scores", "culling_select"):
        assert '"%s"' % timer in header
    for fn in ("principal_curvatures", "culling_scores", "culling_select", "voxel_culling_keypoints"):
        assert callable(getattr(pkg.capi, fn))

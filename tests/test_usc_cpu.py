"""USC on the host (-m "not gpu"): the restatement tests/usc_ref.py against three points worked by hand, every scene of usc_scenes.py
decided on at least nine of ten finite keypoints (what keeps the device test's interval check honest), and the host layer, the binding,
the pipeline and the shipped configuration know the new type and refuse what rows of 1960 floats cannot be served with."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import host_binding as hb
import usc_ref as ref
import usc_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
F = np.float32


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_three_points_by_hand():
    """Keypoint at the origin, identity frame, R = 1, r_min = 0.1: edges e_j = 0.1 * 10^(j/10) = 0.1, 0.1259, 0.1585, 0.1995, 0.2512,
    0.3162, 0.3981, 0.5012, 0.6310, 0.7943, 1. Elevation bins of 12.857 degrees, azimuth bins of 25.714.
      p1 = (0.5, 0, 0.1):      r = 0.5099 in (e_7, e_8] -> j = 7; theta = acos(0.1961) = 78.69 -> k = 6; u along x: phi = 0 -> l = 0.   bin 67
      p2 = (0, 0.3, -0.3):     r = 0.4243 in (e_6, e_7] -> j = 6; theta = 135 -> k = 10; u = (0, 0.3, 0): phi = 90 -> l = 3.          bin 526
      p3 = (-0.2, -0.2, 0.05): r = 0.2872 in (e_4, e_5] -> j = 4; theta = acos(0.1741) = 79.97 -> k = 6; x cross u = (0, 0, -0.2) points
                               against z, so phi = 360 - atan2(0.2, -0.2) = 360 - 135 = 225 -> l = 8.                              bin 1184
    Densities 1, 2, 3: deposits 2^32, (2^32 + 1) // 2 = 2147483648, (2^32 + 1) // 3 = 1431655765."""
    xyz = np.array([[0.5, 0, 0.1], [0, 0.3, -0.3], [-0.2, -0.2, 0.05]], F)
    lrf = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1]], F)
    d = ref.describe([0, 3], xyz, [0, 1], np.zeros((1, 3), F), lrf, 1.0, 0.1, np.array([1, 2, 3]))
    assert d["decided"][0] and not d["nan_row"][0] and d["count"][0] == 3 and d["skipped"][0] == 0
    want = np.zeros(ref.DIM, np.int64)
    want[67], want[526], want[1184] = 2 ** 32, 2147483648, 1431655765
    assert np.array_equal(d["q_lo"][0], want) and np.array_equal(d["q_hi"][0], want)
    # the row: Q * 2^-32 / cbrt(volume of the bin), the volume written out with math for bin (j, k) = (7, 6)
    e = [0.1 * 10 ** (j / 10) for j in range(11)]
    vol = (math.cos(6 * math.pi / 14) - math.cos(7 * math.pi / 14)) * (e[8] ** 3 - e[7] ** 3) / 3 * (2 * math.pi / 14)
    row = ref.row_from_q(d["q_lo"][0], d["lut"])
    assert row[67] == pytest.approx(1 / vol ** (1 / 3), rel=1e-6) and row[526] > 0 and row[1184] > 0 and np.count_nonzero(row) == 3
    assert ref.deposit(0) == ref.deposit(1) == 2 ** 32 and ref.deposit(300) == (2 ** 32 + 150) // 300


def test_edges_and_the_last_bin():
    """a value on an edge belongs to the bin below it and is undecided; a value beyond the last edge takes the last bin"""
    up = np.array([1.0, 2.0, 3.0]); eps = np.full(3, 1e-9)
    assert ref._bin_candidates(0.5, up, eps) == (0, [0])
    assert ref._bin_candidates(2.0, up, eps) == (1, [1, 2])
    assert ref._bin_candidates(2.0 + 1e-12, up, eps) == (2, [1, 2])
    assert ref._bin_candidates(99.0, up, eps) == (3, [3])
    lut, e, e32 = ref.tables(0.4, 0.04)
    assert e[0] == pytest.approx(0.04, rel=1e-7) and e[10] == pytest.approx(0.4, rel=1e-7) and np.all(np.diff(e) > 0)
    assert lut.shape == (10, 14) and np.all(lut > 0) and np.allclose(lut[:, :7], lut[:, :6:-1])      # the elevation bins mirror at the equator
    assert np.all(np.diff(lut[:, 0]) < 0)                                                          # larger shells, smaller weights


@pytest.mark.parametrize("name", scenes.NAMES)
def test_scene_is_decided_on_nine_of_ten_keypoints(ora, name):
    s = scenes.scene(name)
    xyz, kp = s["xyz"], s["kp"]
    lrf = s["lrf"]
    if lrf is None:
        lrf = ora.shot_lrf(s["pt_off"], xyz[:, 0], xyz[:, 1], xyz[:, 2], s["kp_off"], kp[:, 0], kp[:, 1], kp[:, 2], s["frame_radius"])
    dens = ref.density(s["pt_off"], xyz, s["density_radius"])
    d = ref.describe(s["pt_off"], xyz, s["kp_off"], kp, lrf, s["radius"], s["min_radius"], dens)
    finite = ~d["nan_row"]
    undecided = int((finite & ~d["decided"]).sum())
    print(f"{name}: {int(finite.sum())} finite keypoints of {len(kp)}, {undecided} undecided, density {dens[dens > 0].min() if (dens > 0).any() else 0} .. {dens.max()}, "
          f"ball {d['count'][finite].min() if finite.any() else 0} .. {d['count'].max()}")
    assert finite.sum() >= 5 and undecided * 10 <= finite.sum()
    assert np.all(d["q_lo"] <= d["q_hi"]) and np.array_equal(d["q_lo"][d["decided"]], d["q_hi"][d["decided"]])
    if name == "off":
        assert d["nan_row"].tolist() == [False] * 6 + [True] * 4 and np.all(d["count"][6:] == 0)      # a NaN row reports count 0
        assert not np.isfinite(lrf[6]).any() and np.isfinite(lrf[:6]).all()                          # keypoint 6: the frame, not the ball
        assert (ref._d2(xyz, kp[6])[0] < ref._r2(s["radius"])).sum() == 3 and (ref._d2(xyz, kp[7])[0] < ref._r2(s["radius"])).sum() == 0
    if name == "special":
        assert d["nan_row"].tolist() == [False, False, True] + [False] * 5 and d["skipped"][0] == 3 and d["skipped"][1] == 3
        q0, q1 = d["q_lo"][0].reshape(14, 14, 10), d["q_lo"][1].reshape(14, 14, 10)
        assert q0[0, 0].sum() > 0 and q0[0, 13].sum() > 0                       # the two points on the axis: phi = 0, theta 0 and 180
        assert q0[:, :, 0].sum() >= 2 * ref.deposit(dens[2])                    # r < r_min and the point just beyond the skip rule
        assert np.array_equal(q0.sum(0), q1.sum(0))                             # the turned frame moves deposits between azimuth bins only
    if name == "ragged":
        assert dens.max() >= 250 and dens[dens > 0].min() == 1
        assert d["nan_row"][3] and d["nan_row"][4]                              # the keypoints of the empty object


# ------------------------------------------------------------------------------------------------ header, binding, host layer
def test_header_and_binding(pkg):
    h = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    assert re.search(r"#define ISMHIP_KNN_MAX_DIM\s+2048\b", h) and re.search(r"#define ISMHIP_SHORT_CSHOT_MAX_DIM\s+1344\b", h)
    assert re.search(r"#define ISMHIP_USC_DIM\s+1960\b", h)
    assert re.search(r"int\s+ismhip_point_density\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, float density_radius, uint32_t\* density_out\);", h)
    assert re.search(r"int\s+ismhip_usc_tables\(float radius, float min_radius, double\* lut140_out, float\* edges11_out\);", h)
    assert re.search(r"int\s+ismhip_usc\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, const uint32_t\* kp_offsets_h,", h)
    assert "NAMED DEVIATION" in h and "features/features_usc.cpp" in h
    capi = pkg.capi
    for name in ("ismhip_point_density", "ismhip_usc_tables", "ismhip_usc"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert capi.USC_DIM == ref.DIM == 1960 and capi.KNN_MAX_DIM == 2048 and capi.USC_POINT_DENSITY_RADIUS == pytest.approx(0.1)
    assert pkg.pipeline.IsmConfig(feature="USC").dim == 1960


def test_tables_on_the_host(pkg):
    """ismhip_usc_tables is host code: libm against numpy within 4 double ulps, the edges equal after rounding to float"""
    for R, rmin in ((0.4, 0.04), (0.3, 0.03), (1.0, 0.1), (0.25, 0.025)):
        lut, e32 = pkg.capi.usc_tables(R, rmin)
        want, _, we32 = ref.tables(R, rmin)
        assert np.array_equal(e32, we32)
        assert np.all(np.abs(lut - want) <= 4 * np.spacing(want))
    for R, rmin in ((0.0, 0.0), (0.4, 0.4), (0.4, 0.0), (float("inf"), 0.1), (0.4, float("nan"))):
        with pytest.raises(ValueError):
            pkg.capi.usc_tables(R, rmin)


def _cfg(features=None, **edits):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Features"] = features or {"Type": "USC", "Parameters": {"Radius": 0.4, "ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}
    for path, v in edits.items():
        node = j
        keys = path.split("/")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = v
    return json.dumps(j)


def test_host_reads_usc_and_reports_its_length(tmp_path):
    """refused before this descriptor was built: this test fails on the parent commit"""
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "USC", "Parameters": {"Radius": 0.35, "ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}))
    want = json.loads(m.config_to_json())
    out = want["Children"]["Features"]
    assert out["Type"] == "USC" and out["Parameters"]["Radius"] == pytest.approx(0.35)
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m.h.value)) == 1960
    path = str(tmp_path / "usc.ism")
    m.write(path)
    m2 = hb.Model()
    m2.read(path, training=True)
    assert json.loads(m2.config_to_json()) == want
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m2.h.value)) == 1960
    m.close(); m2.close()


def test_host_default_radius():
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "USC", "Parameters": {"ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}))
    assert json.loads(m.config_to_json())["Children"]["Features"]["Parameters"]["Radius"] == pytest.approx(0.1)
    m.close()


def test_shipped_usc_config_loads():
    m = hb.Model()
    m.read(os.path.join(ROOT, "config", "modelnet10_usc.ism"), training=True)
    out = json.loads(m.config_to_json())["Children"]
    assert out["Features"]["Type"] == "USC" and out["Features"]["Parameters"]["Radius"] == pytest.approx(0.4)
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m.h.value)) == 1960
    shot = json.load(open(CFG))["ObjectConfig"]
    usc = json.load(open(os.path.join(ROOT, "config", "modelnet10_usc.ism")))["ObjectConfig"]
    shot["Children"]["Features"]["Type"] = "USC"
    assert shot == usc                                                   # the SHOT configuration, the Features child's type replaced
    m.close()


ACT = "Children/Codebook/Children/ActivationStrategy"


@pytest.mark.parametrize("edits, names", [
    ({ACT: {"Type": "Threshold", "Parameters": {"Threshold": 1.0}}}, r'ActivationStrategy "Threshold" with Features type "USC" is not built'),
    ({ACT: {"Type": "KNN", "Parameters": {"K": 17}}}, r'ActivationStrategy K 17 with Features type "USC" is not built'),
    ({"Children/FeatureWeighting": {"Type": "KNNActivation", "Parameters": {}}}, r'FeatureWeighting "KNNActivation" with Features type "USC" is not built'),
    ({"Children/FeatureWeighting": {"Type": "Incremental", "Parameters": {}}}, r'FeatureWeighting "Incremental" with Features type "USC" is not built'),
])
def test_what_rows_of_1960_floats_cannot_have_is_refused_by_name(edits, names):
    with pytest.raises(hb.HostError, match=names):
        hb.Model().config_from_json(_cfg(**edits))


def test_what_they_can_have_is_taken():
    """K = 16, KNNRule, k-means clustering and the ratio test stay available; the same three options with SHOT are not touched"""
    for edits in ({ACT: {"Type": "KNN", "Parameters": {"K": 16}}}, {ACT: {"Type": "KNNRule", "Parameters": {}}},
                  {ACT: {"Type": "KNN", "Parameters": {"K": 2, "UseDistanceRatio": True}}},
                  {"Children/Clustering": {"Type": "KMeansCount", "Parameters": {"ClusterCount": 50}}}):
        m = hb.Model(); m.config_from_json(_cfg(**edits)); m.close()
    shot = {"Type": "SHOT", "Parameters": {"Radius": 0.4, "ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}
    for edits in ({ACT: {"Type": "Threshold", "Parameters": {"Threshold": 1.0}}}, {ACT: {"Type": "KNN", "Parameters": {"K": 17}}},
                  {"Children/FeatureWeighting": {"Type": "Incremental", "Parameters": {}}}):
        m = hb.Model(); m.config_from_json(_cfg(shot, **edits)); m.close()


def test_usc_with_global_features_is_taken_as_before():
    """the global rows have their own length and their own cap (checked where they are searched): USC does not change either"""
    m = hb.Model()
    m.config_from_json(_cfg(**{"Children/GlobalFeatures": {"Type": "SHOT_GLOBAL", "Parameters": {}},
                               "Children/Voting/Parameters/UseGlobalFeatures": True}))
    assert json.loads(m.config_to_json())["Children"]["Voting"]["Parameters"]["UseGlobalFeatures"] is True
    m.close()


def test_pfh_is_still_refused_and_the_message_names_usc():
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: SHOT, BSHOT, CSHOT, FPFH, SHORT_SHOT, SHORT_CSHOT, ESF_LOCAL, "
                                           r"CGF, RIFT, SpinImage, RSD, CoSPAIR\) and USC"):
        m.config_from_json(_cfg({"Type": "PFH", "Parameters": {}}))
    with pytest.raises(hb.HostError, match="outside the MI355X hot path"):
        m.config_from_json(_cfg({"Type": "3DSC", "Parameters": {}}))
    m.close()

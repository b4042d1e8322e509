"""RSD on the host (no GPU): the restatement tests/rsd_ref.py against answers worked out by hand, proof that the edge scenes of
tests/rsd_scenes.py sit on both sides of every edge and that the generic scene leaves almost no pair undecided, the pair bookkeeping, and
the host layer: header, binding, configuration, the example config, refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import host_binding as hb
import rsd_ref as ref
import rsd_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
F = np.float32


def _hist(row):
    """[angle bin, distance bin]: element ba + 5 * bd of the row"""
    return np.asarray(row).reshape(5, 5).T


# ------------------------------------------------------------------------------------------------ hand-derived answers
def test_plane_gives_the_plane_radius_twice():
    """all normals equal: every pair has a = 1, theta = 0; Amin2 = Amax2 = 0: both radii (float)D * 1.1f; the histogram has angle bin 0 only"""
    s, a = scenes.scene("radii"), scenes.answer("radii")
    want = F(F(s["radius"]) * F(1.1))
    assert a["cnt"][0] == 50 and a["radii"][0].tolist() == [want, want]
    h = _hist(a["lo"][0])
    assert h[0].sum() + a["neglected"][0] == 50 * 49 // 2 and not h[1:].any() and a["undecided"][0] == 0


def test_two_point_radii():
    """one pair with angle theta in distance bin d >= 1: 1.1f * min(f_d / theta, R) for both"""
    s, a = scenes.scene("radii"), scenes.answer("radii")
    D = np.float64(F(s["radius"]))
    capped = 0
    for k, (d, th) in enumerate(scenes.RADII_THETA, start=1):
        theta = np.arccos(np.float64(F(np.cos(th))))                     # c is the float nearest to cos(th)
        assert abs(theta - th) < 1e-6
        f = (d + 0.5) * D / 5.0
        want = F(F(min(f / theta, D)) * F(1.1))
        capped += f / theta >= D
        assert a["cnt"][k] == 2 and a["radii_ok"][k]
        assert a["radii"][k].tolist() == [want, want], (d, th)
        h = _hist(a["lo"][k])
        assert h.sum() == 1 and h[min(4, int(5 * th / (np.pi / 2))), d] == 1
    assert 0 < capped < len(scenes.RADII_THETA)                          # both branches of the min


def test_counts_scene_and_special_rows():
    a = scenes.answer("counts")
    assert a["cnt"].tolist() == scenes.COUNTS
    assert np.isnan(a["row_lo"][0]).all() and np.isnan(a["radii"][0]).all() and not a["valid"][0]       # n = 0: NaN (deviation 1)
    assert not a["row_lo"][1].any() and a["radii"][1].tolist() == [0, 0]                               # n = 1: zeros in either mode
    assert a["lo"][2].sum() + a["neglected"][2] == 1 and a["lo"][3].sum() + a["neglected"][3] == 3
    assert np.isfinite(a["row_lo"][1:]).all()


def test_not_finite_keypoint_and_normals():
    """a keypoint that is not finite: NaN row, count 0; a normal that is not finite: its pairs are skipped (deviation 3), the others stay"""
    P = np.asarray([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0]], F)
    N = np.asarray([[1, 0, 0], [np.nan, 0, 0], [0, 1, 0]], F)
    r = ref.rsd_keypoint(P, N, [np.nan, 0, 0], 0.3)
    assert r["n"] == 0 and not r["valid"]
    r = ref.rsd_keypoint(P, N, [0, 0, 0], 0.3)
    assert r["n"] == 3 and r["pairs"] == 3 and r["skipped"] == 2 and r["lo"].sum() == 1
    assert _hist(r["lo"])[4, 0] == 1                                     # perpendicular normals, 0.07 apart: a = 0 -> theta = pi/2 -> bin 4


# ------------------------------------------------------------------------------------------------ the edge scenes sit on their edges
def test_angle_edges_on_both_sides():
    s, a = scenes.scene("angle_edges"), scenes.answer("angle_edges")
    names = scenes.ANGLE_EDGE_KEYPOINTS
    assert len(names) == len(a["cnt"]) and (a["cnt"] == 2).all() and (a["undecided"] == 0).all()
    ba = {}
    for k, name in enumerate(names):
        h = _hist(a["lo"][k])
        assert h.sum() == 1 and h[:, 1].sum() == 1                       # one pair, distance bin 1
        ba[name] = int(np.flatnonzero(h[:, 1])[0])
    for k in range(1, 5):                                                # a below cos(k pi / 10): theta above the edge, bin k; above: bin k - 1
        assert ba[(k, "below")] == k and ba[(k, "above")] == k - 1 and ba[(k, "at")] in (k - 1, k)
    assert ba["c = 1"] == 0 and ba["c = -1"] == 0 and ba["c above 1"] == 0
    assert ba["generic"] == ba["antiparallel"]
    k = names.index("c above 1")
    v = s["normals"][2 * k]
    assert F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2])) > F(1)


def test_dist_edges_on_both_sides():
    s, a = scenes.scene("dist_edges"), scenes.answer("dist_edges")
    names = scenes.DIST_EDGE_KEYPOINTS
    # dist == R sits ON the edge 5, so the restatement calls it undecided by its rule; every other pair is decided
    assert len(names) == len(a["cnt"]) and a["undecided"].tolist() == [1] + [0] * (len(names) - 1)
    bd = {}
    for k, name in enumerate(names):
        h = _hist(a["lo"][k])
        assert a["cnt"][k] == 2 and h.sum() + a["neglected"][k] + a["undecided"][k] == 1
        bd[name] = int(np.flatnonzero(h.sum(0))[0]) if h.sum() else 5
    for k in range(1, 5):
        assert bd[(k, "below")] == k - 1 and bd[(k, "above")] == k and bd[(k, "at")] in (k - 1, k)
    assert bd["one ulp wider"] == 5 and bd["coincident"] == 0
    # dist == R: d2 = 0.25 = D * D, and sqrt, * and / are correctly rounded: the coordinate is the integer 5 itself, whatever the
    # library, which the definition sends to bin 4 (deviation 4). The interval is {bin 4, neglected}; the device test asks for bin 4.
    _, d2, fin = ref.pair_terms(s["xyz"], s["normals"], np.array([0, 1]))
    _, td, dist, D = ref.bin_coordinates(np.ones(1, F), d2, s["radius"])
    assert fin.all() and d2[0] == F(0.25) and dist[0] == D and td[0] == 5.0
    assert _hist(a["hi"][0])[:, 4].sum() == 1 and a["lo"][0].sum() == 0 and a["neg_hi"][0] == 1


def test_overflow_scene_counts():
    a = scenes.answer("overflow")
    assert a["cnt"].tolist() == scenes.OVERFLOW and scenes.OVERFLOW[0] == scenes.OVERFLOW_CAP and scenes.OVERFLOW[1] == scenes.OVERFLOW_CAP + 1


# ------------------------------------------------------------------------------------------------ conditions on the inputs, bookkeeping
def test_generic_scene_is_decided_and_every_pair_is_accounted_for():
    for name in scenes.SCENES:
        a = scenes.answer(name)
        n = a["cnt"]
        print("%-12s keypoints %3d, n %d..%d, pairs %d, undecided %d, left out of the radii %d" %
              (name, len(n), n.min(), n.max(), a["pairs"].sum(), a["undecided"].sum(), (~a["radii_ok"]).sum()))
        assert np.array_equal(a["pairs"], n * (n - 1) // 2)
        # sum of the counts + neglected + skipped = n (n - 1) / 2, the undecided pairs between the two ends
        assert (a["lo"].sum(1) + a["neglected"] + a["skipped"] + a["undecided"] == a["pairs"]).all()
        assert (a["hi"] >= a["lo"]).all() and (a["hi"].sum(1) - a["lo"].sum(1) <= 4 * a["undecided"]).all()
    a = scenes.answer("generic")
    assert len(a["cnt"]) == 64 and a["cnt"].min() == 0 and 100 <= a["cnt"].max() <= 140
    assert len(np.unique(a["cnt"])) >= 20
    assert a["undecided"].sum() <= 0.01 * a["pairs"].sum()
    assert (~a["radii_ok"]).sum() <= 0.10 * len(a["cnt"])
    assert (a["lo"].sum(0) > 0).all()                                    # every one of the 25 bins is used
    assert a["neglected"].sum() > 0


# ------------------------------------------------------------------------------------------------ host layer
def test_header_and_binding(pkg):
    h = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    assert re.search(r"int\s+ismhip_rsd\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, const uint32_t\* kp_offsets_h,", h)
    assert re.search(r"#define ISMHIP_RSD_DIM\s+25\b", h) and re.search(r"#define ISMHIP_RSD_RADII_DIM\s+2\b", h)
    assert re.search(r"#define ISMHIP_ABI_VERSION\s+4\b", h)
    assert '"rsd"' in h and "features/features_rsd.cpp" in h and "ismhip_spin_image / ismhip_rsd" in h
    capi = pkg.capi
    assert "ismhip_rsd" in capi.EXPORTS and callable(capi.rsd)
    assert capi.RSD_DIM == ref.DIM == 25 and capi.RSD_RADII_DIM == ref.RADII_DIM == 2
    assert pkg.pipeline.IsmConfig(feature="RSD").dim == 25
    assert pkg.pipeline.IsmConfig(feature="RSD", use_full_rsd_histogram=False).dim == 2


def _cfg(features):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Features"] = features
    return json.dumps(j)


@pytest.mark.parametrize("full, dim", [(None, 25), (True, 25), (False, 2)])
def test_host_reads_rsd_and_reports_its_length(tmp_path, full, dim):
    """refused before this descriptor was built: this test fails on the parent commit"""
    params = {"Radius": 0.35, "ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}
    if full is not None:
        params["UseFullRSDHistogram"] = full
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "RSD", "Parameters": params}))
    want = json.loads(m.config_to_json())
    out = want["Children"]["Features"]
    assert out["Type"] == "RSD" and out["Parameters"]["Radius"] == pytest.approx(0.35)
    assert out["Parameters"]["UseFullRSDHistogram"] is (True if full is None else full)
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m.h.value)) == dim
    path = str(tmp_path / "rsd.ism")
    m.write(path)
    m2 = hb.Model()
    m2.read(path, training=True)
    assert json.loads(m2.config_to_json()) == want
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m2.h.value)) == dim
    m.close(); m2.close()


def test_host_default_radius():
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "RSD", "Parameters": {"ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}))
    out = json.loads(m.config_to_json())["Children"]["Features"]["Parameters"]
    assert out["Radius"] == pytest.approx(0.1) and out["UseFullRSDHistogram"] is True
    m.close()


def test_shipped_rsd_config_loads():
    m = hb.Model()
    m.read(os.path.join(ROOT, "config", "modelnet10_rsd.ism"), training=True)
    out = json.loads(m.config_to_json())["Children"]
    assert out["Features"]["Type"] == "RSD" and out["Keypoints"]["Type"] == "VoxelGrid"
    assert out["Features"]["Parameters"]["UseFullRSDHistogram"] is True
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m.h.value)) == 25
    m.close()


def test_unknown_feature_type_is_still_refused_and_the_message_names_rsd():
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: .*SpinImage, RSD, CoSPAIR\)"):
        m.config_from_json(_cfg({"Type": "PFH", "Parameters": {}}))
    m.close()

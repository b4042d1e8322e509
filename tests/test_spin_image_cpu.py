"""SpinImage on the host (no GPU): the restatement tests/spin_image_ref.py against answers worked out by hand, proof that no scene of
tests/spin_image_scenes.py (the cylinder scene apart, which plants its neighbours at the limit on purpose) leaves a neighbour's fate to
the last bit, and the host layer: header, binding, configuration, the example config, refusals."""
import json
import os
import re

import numpy as np
import pytest

import host_binding as hb
import spin_image_ref as ref
import spin_image_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
W = 8
STRIDE = 2 * W + 1


def _image(row):
    return np.asarray(row).reshape(W + 1, STRIDE)


# ------------------------------------------------------------------------------------------------ hand-derived answers
def test_three_point_hand_case():
    """(b) radius sqrt(2): bin = sqrt(2) / 8 / sqrt(2) = 0.125 (the float radius is off by 2e-8). The point (0.1875, 0, 0.0625) about the
    origin with axis +z: beta = 0.0625 = 0.5 bins, alpha = 0.1875 = 1.5 bins: ia = 1, ib = 0 + 8, a = b = 0.5, four deposits of 0.25.
    Given twice, with the centre itself (norm 0: counted, skipped): cnt = 3 > 1, sum of the bins 2, every entry 0.5 / 2."""
    a = scenes.answer("hand3")
    assert a["idx"].tolist() == [0] and a["axes"].tolist() == [[0, 0, 1]] and a["cnt"].tolist() == [3] and a["deposited"].tolist() == [2]
    img = _image(a["rows"][0])
    for e in [(1, 8), (1, 9), (2, 8), (2, 9)]:
        assert abs(img[e] - 0.25) <= 1e-6
    assert np.count_nonzero(img) == 4


def test_keypoint_off_the_cloud_fills_one_column():
    """(c) no equal point: index -1, the zero axis, every cosine 0: beta = 0, b = 0, ib = 8 -- only column 8, and the row sums to 1"""
    a = scenes.answer("off_cloud")
    assert (a["idx"] == -1).all() and not a["axes"].any() and (a["cnt"] > 1).all()
    for row in a["rows"]:
        img = _image(row)
        assert img[:, W].sum() == pytest.approx(1.0, abs=1e-6) and not np.delete(img, W, axis=1).any()


def test_lower_index_of_coincident_points_wins():
    """(d)"""
    s, a = scenes.scene("twins"), scenes.answer("twins")
    assert a["idx"].tolist() == [7, 7, 100]
    assert np.array_equal(a["axes"][0], s["normals"][7]) and np.array_equal(a["axes"][1], s["normals"][7])
    assert not np.array_equal(s["normals"][7], s["normals"][40])


def test_scaled_axis():
    """(e) |axis| = 1.5 and a neighbour along it: cosine 1.5, the whole row NaN, the count kept; |axis| = 0.5: every cosine halves, finite"""
    a = scenes.answer("scaled_axis")
    assert np.isnan(a["rows"][0]).all() and np.isfinite(a["rows"][1]).all()
    assert a["cnt"][0] == a["cnt"][1] > 50 and a["rows"][1].sum() == pytest.approx(1.0, abs=1e-6)


def test_counts_and_special_rows():
    """(f)"""
    a = scenes.answer("counts")
    rows, cnt, idx = a["rows"], a["cnt"], a["idx"]
    assert scenes.COUNT_KEYPOINTS[3] == "outside the cylinder"
    assert cnt.tolist() == [0, 0, 1, 3, 0, 0] and idx.tolist() == [-1, -1, 2, 3, -1, 6]
    for k in (0, 1, 2):                                                  # empty ball, ball off the grid, the keypoint's own point only: zero
        assert not rows[k].any()
    for k in (3, 4, 5):                                                  # 0 / 0, keypoint not finite, matched normal not finite: NaN as a whole
        assert np.isnan(rows[k]).all()
    assert np.isnan(a["axes"][5][0])


def test_cylinder_limit():
    """(g) of the six neighbours planted at lim (1 -+ 1e-6) the three inner ones deposit"""
    a = scenes.answer("cylinder")
    assert a["cnt"].tolist() == [7] and a["deposited"].tolist() == [scenes.CYLINDER_PLANTED]
    s = scenes.scene("cylinder")
    for keep, n_in in (([0, 1, 2], 1), ([0, 3, 4], 1), ([0, 5, 6], 1), ([0, 2, 4, 6], 0), ([0, 1, 3, 5], 3)):
        assert ref.spin_row(s["xyz"][keep], s["kp"][0], [0, 0, 1], s["radius"])["deposited"] == n_in


def test_ring_closed_form():
    """(h) 4000 neighbours with alpha = 5/16 = 2.5 bins and beta = 3/16 = 1.5 bins: four entries of 1000 / 4000"""
    a = scenes.answer("ring")
    assert a["cnt"].tolist() == [4001] and a["deposited"].tolist() == [4000]
    img = _image(a["rows"][0])
    for e in scenes.RING_ENTRIES:
        assert abs(img[e] - 0.25) <= 1e-6
    assert np.count_nonzero(img) == 4


def test_no_scene_leaves_a_neighbour_undecided():
    for name in scenes.SCENES:
        a = scenes.answer(name)
        print("%-12s keypoints %3d neighbours %6d undecided %d" % (name, len(a["cnt"]), a["cnt"].sum(), a["undecided"]))
        if name != "cylinder":
            assert a["undecided"] == 0, name
    assert scenes.answer("long_queue")["cnt"].tolist() == [20001]
    a = scenes.answer("sphere")
    assert (a["idx"] >= 0).all() and np.isfinite(a["rows"]).all() and (a["cnt"] > 50).all()
    for name, w in (("sphere_w1", 1), ("sphere_w25", 25)):
        assert scenes.answer(name)["rows"].shape == (64, ref.dim_of(w)) and np.isfinite(scenes.answer(name)["rows"]).all()
    b = scenes.answer("batch")
    assert (b["idx"] >= 0).sum() == 33 and (b["idx"] == -1).sum() == 3


# ------------------------------------------------------------------------------------------------ host layer
def test_header_and_binding(pkg):
    h = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    assert re.search(r"int\s+ismhip_keypoint_normals\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, const uint32_t\* kp_offsets_h,", h)
    assert re.search(r"int\s+ismhip_spin_image\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, const uint32_t\* kp_offsets_h,", h)
    assert re.search(r"#define ISMHIP_SPIN_IMAGE_WIDTH\s+8\b", h) and re.search(r"#define ISMHIP_SPIN_IMAGE_DIM\s+153\b", h)
    assert re.search(r"#define ISMHIP_ABI_VERSION\s+4\b", h)
    assert '"keypoint_normals"' in h and '"spin_image"' in h                  # the timer names
    capi = pkg.capi
    assert "ismhip_keypoint_normals" in capi.EXPORTS and "ismhip_spin_image" in capi.EXPORTS
    assert capi.SPIN_IMAGE_WIDTH == 8 and capi.SPIN_IMAGE_DIM == 153 == ref.dim_of(8)
    assert callable(capi.keypoint_normals) and callable(capi.spin_image)
    assert pkg.pipeline.IsmConfig(feature="SpinImage").dim == 153


def _cfg(features):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Features"] = features
    return json.dumps(j)


def test_host_config_loads_and_roundtrips(tmp_path):
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "SpinImage", "Parameters": {"ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}))
    out = json.loads(m.config_to_json())["Children"]["Features"]
    assert out["Type"] == "SpinImage" and out["Parameters"]["Radius"] == pytest.approx(0.1)      # Radius not given: the reference's default
    m.config_from_json(_cfg({"Type": "SpinImage", "Parameters": {"Radius": 0.35, "ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}))
    want = json.loads(m.config_to_json())
    assert want["Children"]["Features"]["Parameters"]["Radius"] == pytest.approx(0.35)
    m2 = hb.Model()
    m2.config_from_json(json.dumps(want))                                    # what we write, we read
    assert json.loads(m2.config_to_json()) == want
    path = str(tmp_path / "spin.ism")
    m.write(path)
    m3 = hb.Model()
    m3.read(path, training=True)
    assert json.loads(m3.config_to_json()) == want
    for x in (m, m2, m3):
        x.close()


def test_shipped_spin_image_config_loads():
    m = hb.Model()
    m.read(os.path.join(ROOT, "config", "modelnet10_spin_image_iss3d.ism"), training=True)
    out = json.loads(m.config_to_json())["Children"]
    assert out["Features"]["Type"] == "SpinImage" and out["Keypoints"]["Type"] == "ISS3D"
    assert out["Features"]["Parameters"]["Radius"] == pytest.approx(0.4)
    m.close()


def test_unknown_feature_type_is_still_refused_and_the_message_names_spin_image():
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: .*SpinImage.*\)"):
        m.config_from_json(_cfg({"Type": "PFH", "Parameters": {}}))
    m.close()

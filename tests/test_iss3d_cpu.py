"""ISS3D on the CPU: the restatement tests/iss3d_ref.py against hand-derived answers, and the host's KeypointsISS3D configuration
(keypoints/keypoints_iss3d.cpp:17-26: names and defaults) -- parse, round trip, refusals. No GPU is touched."""
import json
import os

import numpy as np
import pytest

import host_binding as hb
import iss3d_ref as ref
import iss3d_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
DEFAULTS = {"SalientRadius": 0.1, "NonMaxRadius": 0.05, "Gamma21": 0.975, "Gamma32": 0.975, "MinNeighbors": 5}


def test_exact_plane_has_no_keypoints():
    a = ref.iss3d(scenes.plane(), 0.05, 0.03)
    assert (a["count"] >= 5).all()
    assert np.array_equal(a["eig"][:, 2], np.zeros(len(a["eig"])))        # e3 is exactly 0: saliency 0, never a candidate
    assert (a["eig"][:, 0] > 0).all()
    assert not a["saliency"].any() and not a["keep"].any()


def test_cluster_below_min_neighbors_has_no_keypoints():
    a = ref.iss3d(scenes.small_cluster(), 1.0, 1.0, min_neighbors=5)
    assert np.array_equal(a["count"], [4, 4, 4, 4])
    assert not a["eig"].any() and not a["saliency"].any() and not a["keep"].any() and not a["undecided"].any()
    b = ref.iss3d(scenes.small_cluster(), 1.0, 1.0, min_neighbors=4)      # the same cluster with MinNeighbors 4 is searched
    assert (b["eig"][:, 0] > 0).all()


def test_six_point_cross_by_hand():
    """O = origin, +-a on x, +-b on y, +c on z with a = 0.04, b = 0.03, c = 0.02 and both radii 0.045.
    About O all six are neighbours: C = diag(2 a^2, 2 b^2, c^2), ratios 0.5625 and 0.2222: salient, saliency c^2.
    About the z point (distances c, sqrt(a^2 + c^2) = 0.0447, sqrt(b^2 + c^2) = 0.0361: all six again) the cross terms cancel:
    C = diag(2 a^2, 2 b^2, 5 c^2), sorted (2 a^2, 5 c^2, 2 b^2), ratios 0.625 and 0.9: salient, saliency 2 b^2 > c^2.
    The x points see O and the z point only (0.05 to the y points), the y points likewise: 3 < MinNeighbors, zero matrix.
    Suppression: O has the z point in its ball and loses; the z point wins."""
    a, b, c = (float(np.float32(v)) for v in (0.04, 0.03, 0.02))
    xyz = np.array([[0, 0, 0], [a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, c]], np.float32)
    r = ref.iss3d(xyz, 0.045, 0.045, 0.975, 0.975, 5)
    assert np.array_equal(r["count"], [6, 3, 3, 3, 3, 6])
    np.testing.assert_allclose(r["eig"][0], [2 * a * a, 2 * b * b, c * c], rtol=1e-12)
    np.testing.assert_allclose(r["eig"][5], [2 * a * a, 5 * c * c, 2 * b * b], rtol=1e-12)
    assert not r["eig"][1:5].any()
    np.testing.assert_allclose(r["saliency"], [c * c, 0, 0, 0, 0, 2 * b * b], rtol=1e-12)
    assert np.array_equal(r["keep"], [False, False, False, False, False, True])
    assert not r["undecided"].any()
    # a NonMaxRadius that isolates every point: fewer than MinNeighbors in the ball, no keypoint
    assert not ref.iss3d(xyz, 0.045, 0.015, 0.975, 0.975, 5)["keep"].any()
    # Gamma32 below 0.9 turns the z point away and O, no longer beaten, wins
    r2 = ref.iss3d(xyz, 0.045, 0.045, 0.975, 0.5, 5)
    assert np.array_equal(r2["keep"], [True, False, False, False, False, False])


def test_lattice_boundary_points_are_not_neighbours():
    """spacing 1 / 64, radius 4 / 64: every coordinate difference and the squared radius are exact in float32, and the six lattice points
    at exactly d2 == r2 do not count"""
    xyz = scenes.lattice()
    assert float(ref.r2_of(scenes.LATTICE_RADIUS)) == 16.0 / 4096.0
    a = ref.iss3d(xyz, scenes.LATTICE_RADIUS, scenes.LATTICE_RADIUS)
    want = scenes.lattice_counts()
    assert want.max() == 251 and np.array_equal(a["count"], want)          # 257 lattice offsets with |o|^2 <= 16, six of them == 16
    centre = np.nonzero((xyz == np.float32(4.0 / 64.0)).all(1))[0][0]
    assert a["count"][centre] == 251


def test_scenes_give_keypoints_and_no_undecided_point():
    for gammas in scenes.GAMMAS:
        for k in range(len(scenes.SCENES)):
            a = scenes.answer(k, gammas)
            print("scene %d gammas %s: salient %d keypoints %d undecided %d" % (k, gammas, (a["saliency"] > 0).sum(), a["keep"].sum(), a["undecided"].sum()))
            assert a["keep"].sum() >= 40 and a["undecided"].sum() == 0


def test_summation_order_margin():
    """forward against reversed summation order of the scatter stays four orders inside MARGIN"""
    p = scenes.scene(0)
    ns = ref.neighbours(p, scenes.SCENES[0][1])
    worst = 0.0
    for i in range(0, len(p), 7):
        w1 = np.linalg.eigvalsh(ref.scatter(p, i, ns[i])); w2 = np.linalg.eigvalsh(ref.scatter(p, i, ns[i][::-1]))
        worst = max(worst, np.abs(w1 - w2).max() / w1[2])
    assert worst <= 1e-4 * ref.MARGIN


def _cfg(keypoints):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Keypoints"] = keypoints
    return json.dumps(j)


def test_iss3d_config_parses_with_reference_names_and_defaults():
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "ISS3D"}))                            # every key missing: the reference's defaults
    out = json.loads(m.config_to_json())["Children"]["Keypoints"]
    assert out["Type"] == "ISS3D" and sorted(out["Parameters"]) == sorted(DEFAULTS)
    for k, v in DEFAULTS.items():
        assert out["Parameters"][k] == v
    params = {"SalientRadius": 0.24, "NonMaxRadius": 0.16, "Gamma21": 0.8, "Gamma32": 0.7, "MinNeighbors": 9}
    m.config_from_json(_cfg({"Type": "ISS3D", "Parameters": params}))
    out = json.loads(m.config_to_json())
    assert out["Children"]["Keypoints"] == {"Type": "ISS3D", "Parameters": params}
    m2 = hb.Model()
    m2.config_from_json(json.dumps(out))                                   # what we write, we read
    assert json.loads(m2.config_to_json()) == out


def test_shipped_iss3d_config_loads():
    m = hb.Model()
    m.read(os.path.join(ROOT, "config", "modelnet10_shot_iss3d.ism"), training=True)
    out = json.loads(m.config_to_json())
    assert out["Children"]["Keypoints"]["Type"] == "ISS3D" and out["Children"]["Features"]["Type"] == "SHOT"


def test_iss3d_config_roundtrips_through_the_model_file(tmp_path):
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "ISS3D", "Parameters": {"SalientRadius": 0.3, "NonMaxRadius": 0.2, "Gamma21": 0.9, "Gamma32": 0.85, "MinNeighbors": 7}}))
    want = json.loads(m.config_to_json())
    path = str(tmp_path / "iss.ism")
    m.write(path)
    m2 = hb.Model()
    m2.read(path, training=True)
    assert json.loads(m2.config_to_json()) == want


@pytest.mark.parametrize("key,value", [("SalientRadius", 0.0), ("SalientRadius", -0.1), ("NonMaxRadius", 0.0), ("NonMaxRadius", -1.0),
                                       ("Gamma21", 0.0), ("Gamma32", -0.5), ("MinNeighbors", -1), ("SalientRadius", "wide")])
def test_iss3d_config_refuses_bad_parameters(key, value):
    m = hb.Model()
    with pytest.raises(hb.HostError) as e:
        m.config_from_json(_cfg({"Type": "ISS3D", "Parameters": {key: value}}))
    assert key in str(e.value) or "invalid" in str(e.value)


def test_keypoint_factory_lists_iss3d():
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"built: VoxelGrid, ISS3D"):
        m.config_from_json(_cfg({"Type": "Harris3D"}))

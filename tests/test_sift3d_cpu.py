"""SIFT3D on the CPU: the restatement tests/sift3d_ref.py against known answers, the share of undecided extremum tests of every scene the
GPU tests use, the host's KeypointsSIFT3D configuration (keypoints/keypoints_sift3d.cpp:17-22: one parameter, Radius 0.05) -- parse,
round trip, refusals -- and the five entries in the header and in capi.EXPORTS. No GPU is touched."""
import json
import os
import re

import numpy as np
import pytest

import host_binding as hb
import sift3d_ref as ref
import sift3d_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
ENTRIES = ["ismhip_normal_curvature", "ismhip_voxel_downsample_xyzi", "ismhip_sift3d_scale_space", "ismhip_sift3d_extrema", "ismhip_sift3d_keypoints"]


def test_scales_bit_for_bit():
    """0.05 * 2^((i - 1) / 3) in float: 2^(-1/3), 1, 2^(1/3), 2^(2/3), 2, 2^(4/3) times 0.05f, each rounded once more by the product"""
    want = np.array([0x3D228CC4, 0x3D4CCCCD, 0x3D810413, 0x3DA28CC4, 0x3DCCCCCD, 0x3E010413], np.uint32)
    got = ref.scales(0.05, 3)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want)
    # the octave structure: scales[i + 3] is exactly twice scales[i]
    assert np.array_equal(got[3:], got[:3] * np.float32(2.0))


def test_constant_field_has_no_extremum():
    """a constant intensity: every response is the constant exactly (x / x), every dog value 0, and the strict comparisons give nothing"""
    xyz, _inten, _c = scenes.plane_with_bump(1.0, n_side=21, s0=0.05)
    D, B, cnt = ref.dog(xyz, np.ones(len(xyz), np.float32), ref.scales(0.02, 3))
    assert np.array_equal(D, np.zeros_like(D)) and (cnt >= 25).all()
    flags, und, _nn = ref.extrema(xyz, D, None)
    assert not flags.any() and not und.any()


@pytest.mark.parametrize("sign,flag", [(-1.0, 2), (1.0, 1)])
def test_gaussian_bump_gives_one_extremum_in_the_expected_column(sign, flag):
    """On a plane the response of a blob exp(-r^2 / 2 s0^2) at its centre is s0^2 / (s0^2 + s^2) at scale s, so |response_{i+1} -
    response_i| is largest where s passes s0. With s0 the geometric mean of scales[2] and scales[3] that is column 2: dog[.][2] =
    response_3 - response_2. The responses fall with the scale under a bump, so its centre is a MINIMUM of the differences (flag 1); a
    dip of the same shape gives the MAXIMUM (flag 2)."""
    sc = ref.scales(0.03, 3)
    s0 = float(np.sqrt(float(sc[2]) * float(sc[3])))
    xyz, inten, centre = scenes.plane_with_bump(sign, s0=s0)
    D, B, _cnt = ref.dog(xyz, inten, sc)
    flags, und, nn = ref.extrema(xyz, D, B)
    assert nn[centre, 0] == centre and (nn[centre] >= 0).all()
    assert np.argmax(np.abs(D[centre])) == 2
    assert flags[centre, 2] == flag and not und[centre].any()
    assert not flags[:, 0].any() and not flags[:, -1].any()          # the border columns never flag
    # nothing else of that kind within two blob widths of the centre in that column
    near = np.nonzero(np.linalg.norm(xyz - xyz[centre], axis=1) < 2.0 * s0)[0]
    assert [i for i in near if flags[i, 2] == flag] == [centre]


def test_knn_tie_rule():
    """duplicates and exact ties: (d2, index) ascending, the lowest index first; fewer than k points: padded with -1"""
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [-1, 0, 0], [0, 1, 0]], np.float32)
    nn = ref.knn(p, 7)
    assert nn[0].tolist() == [0, 2, 1, 3, 4, -1, -1]
    assert nn[2].tolist() == [0, 2, 1, 3, 4, -1, -1]                  # the duplicate's own index is not first: index order decides
    assert nn[1].tolist() == [1, 0, 2, 4, 3, -1, -1]


def test_lattice_boundary_points_are_neighbours():
    """spacing 1 / 64, scales 1 / 128, 1 / 64, 1 / 32: every d2 and every 9 s2 is exact in float32 and the points at exactly d2 == 9 s2
    count (<=)"""
    xyz = scenes.lattice()
    sc = np.array([1 / 128, 1 / 64, 1 / 32], np.float32)
    assert [float(np.float32(9.0) * s * s) for s in sc] == [9 / 16384, 9 / 4096, 36 / 4096]
    _D, _B, cnt = ref.dog(xyz, np.ones(len(xyz), np.float32), sc)
    assert np.array_equal(cnt, scenes.lattice_counts(reach2=36))
    _D, _B, cnt = ref.dog(xyz, np.ones(len(xyz), np.float32), sc[:2].tolist() + [1 / 64])
    want = scenes.lattice_counts(reach2=9)
    assert np.array_equal(cnt, want) and want.max() == 1 + 6 + 12 + 8 + 6 + 24 + 24 + 12 + 30     # |o|^2 = 0, 1, 2, 3, 4, 5, 6, 8, 9


def test_isolated_point_keeps_its_intensity():
    xyz = np.array([[0, 0, 0], [5, 5, 5]], np.float32)
    D, B, cnt = ref.dog(xyz, np.array([0.75, -0.25], np.float32), ref.scales(0.05, 3))
    assert np.array_equal(D, np.zeros_like(D)) and cnt.tolist() == [1, 1]


@pytest.mark.parametrize("k", range(len(scenes.SCENES)))
def test_scenes_have_extrema_and_few_undecided_tests(k):
    a = scenes.answer(k)
    share = scenes.undecided_share(a)
    print("scene %d: %d minima, %d maxima, undecided share %.4f, largest bound %.2e" %
          (k, (a["flags"] == 1).sum(), (a["flags"] == 2).sum(), share, np.nanmax(a["bound"])))
    assert (a["flags"] == 1).sum() >= 5 and (a["flags"] == 2).sum() >= 5
    assert share <= 0.02


def _cfg(keypoints):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Keypoints"] = keypoints
    return json.dumps(j)


def test_sift3d_config_parses_with_reference_name_and_default():
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "SIFT3D"}))
    out = json.loads(m.config_to_json())["Children"]["Keypoints"]
    assert out["Type"] == "SIFT3D" and list(out["Parameters"]) == ["Radius"]
    assert out["Parameters"]["Radius"] == pytest.approx(0.05, rel=1e-6)
    m.config_from_json(_cfg({"Type": "SIFT3D", "Parameters": {"Radius": 0.125}}))
    out = json.loads(m.config_to_json())
    assert out["Children"]["Keypoints"] == {"Type": "SIFT3D", "Parameters": {"Radius": 0.125}}
    m2 = hb.Model()
    m2.config_from_json(json.dumps(out))                                   # what we write, we read
    assert json.loads(m2.config_to_json()) == out


def test_sift3d_config_roundtrips_through_the_model_file(tmp_path):
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "SIFT3D", "Parameters": {"Radius": 0.25}}))
    want = json.loads(m.config_to_json())
    path = str(tmp_path / "sift.ism")
    m.write(path)
    m2 = hb.Model()
    m2.read(path, training=True)
    assert json.loads(m2.config_to_json()) == want


def test_shipped_sift3d_config_loads():
    m = hb.Model()
    m.read(os.path.join(ROOT, "config", "modelnet10_shot_sift3d.ism"), training=True)
    out = json.loads(m.config_to_json())
    assert out["Children"]["Keypoints"]["Type"] == "SIFT3D" and out["Children"]["Features"]["Type"] == "SHOT"


@pytest.mark.parametrize("value", [0.0, -0.05, "wide"])
def test_sift3d_config_refuses_bad_radius(value):
    m = hb.Model()
    with pytest.raises(hb.HostError) as e:
        m.config_from_json(_cfg({"Type": "SIFT3D", "Parameters": {"Radius": value}}))
    assert "Radius" in str(e.value) or "invalid" in str(e.value)


def test_harris3d_stays_refused_and_the_message_names_sift3d():
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"\(built: VoxelGrid, ISS3D, VoxelGridCulling\).*SIFT3D"):
        m.config_from_json(_cfg({"Type": "Harris3D"}))


def test_header_and_exports_list_the_five_entries(pkg):
    header = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    assert re.search(r"#define\s+ISMHIP_ABI_VERSION\s+4\b", header)
    for name in ENTRIES:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), name
        assert pkg.capi.EXPORTS.count(name) == 1, name

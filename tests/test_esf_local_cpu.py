"""ESF_LOCAL on the host (-m "not gpu"): the restatement tests/esf_ref.py against a row derived by hand, the stated values of the hash,
every scene of esf_scenes.py "sits where it claims", the margins of the restatement hold against the float32 transcription on every
scene, and the host layer, the binding, the pipeline and the shipped configuration know the new type."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import esf_ref as ref
import esf_scenes as scenes
import host_binding as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")
F = np.float32
B = ref.BINS


def _blocks(counts):
    return np.asarray(counts).reshape(10, B)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_hash_values_and_draws():
    """h as the header writes it out, worked by hand for x = 0 (seed 0: every step keeps 0) and by Python integers for the rest"""
    def h(s, x):
        v = (x * 0x9E3779B1 + s) % 2**32
        v ^= v >> 16; v = v * 0x7FEB352D % 2**32
        v ^= v >> 15; v = v * 0x846CA68B % 2**32
        return v ^ (v >> 16)
    assert int(ref.hash32(0, [0])[0]) == 0
    assert int(ref.hash32(ref.SEED, [0])[0]) == h(ref.SEED, 0) == 0x86BB2B32
    xs = [1, 2, 3, 59999, 2**31, 2**32 - 1]
    assert [int(v) for v in ref.hash32(ref.SEED, xs)] == [h(ref.SEED, x) for x in xs]
    assert [int(v) for v in ref.hash32(7, xs)] == [h(7, x) for x in xs]
    d = ref.draws(ref.SEED, np.arange(5), 190)
    assert d.tolist() == [[h(ref.SEED, 3 * t + k) * 190 >> 32 for k in range(3)] for t in range(5)]
    # the stream is flat enough to draw from: 60 000 indices into 10 cells, each within 5 % of its share
    share = np.bincount(ref.draws(ref.SEED, np.arange(20000), 10).ravel(), minlength=10)
    assert np.abs(share - 6000).max() < 300


def test_voxels_and_the_walk():
    """step 4 at its edges and PCL's lci on lines worked by hand"""
    g = np.asarray([-32.5, -32.0, -31.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 31.5, 32.0, 32.5])
    assert ref.cells(g).tolist() == [0, 0, 0, 31, 31, 31, 32, 32, 33, 63, 63, 63]
    occ = ref.occupancy(np.asarray([[0, 0, 0], [63, 31, 31]]))
    assert occ.sum() == 8 + 18 and occ[1, 1, 1] and occ[62, 30, 32] and not occ[2, 0, 0]
    full = np.ones((64, 64, 64), bool)
    # the same voxel: one cell; a neighbour: one cell (the walk stops one step short of the end); ten along x: ten cells
    vis, ins = ref.walk(full, [[5, 5, 5], [5, 5, 5], [5, 5, 5]], [[5, 5, 5], [5, 6, 5], [15, 5, 5]])
    assert vis.tolist() == [1, 1, 10] and ins.tolist() == [1, 1, 10]
    # a diagonal in x and y with a tie of the driving axis: x drives, y follows every step
    only = np.zeros((64, 64, 64), bool)
    for i in range(4):
        only[10 + i, 20 - i, 7] = True
    vis, ins = ref.walk(only, [[10, 20, 7]], [[14, 16, 7]])
    assert vis.tolist() == [4] and ins.tolist() == [4]
    # z drives (L = 4), x follows once its error 2 * 1 - 4 has been raised above 0, after the third cell: (0,0,0) (0,0,1) (0,0,2) (1,0,3)
    # visited, (1,0,4) is the end
    path = np.zeros((64, 64, 64), bool)
    for c in [(0, 0, 0), (0, 0, 1), (0, 0, 2), (1, 0, 3)]:
        path[c] = True
    vis, ins = ref.walk(path, [[0, 0, 0]], [[1, 0, 4]])
    assert vis.tolist() == [4] and ins.tolist() == [4]
    assert ref.line_class(np.array([10, 10, 10, 5]), np.array([9, 8, 7, 3])).tolist() == [ref.IN, ref.MIXED, ref.OUT, ref.OUT]
    assert ref.triangle_class(np.array([[10, 10, 10], [10, 10, 10], [10, 10, 10]]),
                              np.array([[7, 7, 7], [9, 9, 9], [8, 8, 8]])).tolist() == [ref.OUT, ref.IN, ref.MIXED]


def test_three_points_by_hand():
    """(c) g = (32, 0, 0), (-16, 24, 0), (-16, -24, 0), exact. Sides sqrt(2880), sqrt(2880), 48. Interior angles: cos = 0.6 at the apex
    (53.13 deg -> 53.13 / 90 * 63 + 0.5 = 37.69 -> bin 37) and 24 / sqrt(2880) = 0.447 at the base (63.43 deg -> 44.90 -> bin 44), twice.
    Voxels (63, 31, 31), (16, 55, 31), (16, 8, 31): a line of 47 cells meets two occupied cells at its start and one before its end
    (3 of 47: OUT), the triangle holds 9 <= 21 (OUT). So per sample, in sixths: A3 out 1 at bin 37 and 2 at bin 44; D3 out 3 at bin 63
    (every sample is the maximum, up to an ulp); D2 out 12 at bin 63 twice (the long sides are the maximum) and 12 at
    floor(48 / sqrt(2880) * 63 + 0.5) = floor(56.85) = 56. 1000 samples: 42 000 sixths."""
    s, a = scenes.scene("triangle"), scenes.answer("triangle")
    assert a["cnt"].tolist() == [3] and not a["nan"][0] and not a["whole"][0]
    assert a["scale"][0].tolist() == [0.0, 0.0, 0.0, 2.0]
    g = ref.scaled64(s["xyz"], a["scale"][0, :3], a["scale"][0, 3])
    assert g.v.tolist() == [[32, 0, 0], [-16, 24, 0], [-16, -24, 0]] and not g.e.any()
    assert ref.cells(g.v).tolist() == [[63, 31, 31], [16, 55, 31], [16, 8, 31]]
    want = np.zeros((10, B), np.int64)
    want[1, 37], want[1, 44] = 1000, 2000
    want[4, 63] = 3000
    want[7, 63], want[7, 56] = 24000, 12000
    assert np.array_equal(a["lo"][0], a["hi"][0]) and np.array_equal(_blocks(a["lo"][0]), want)
    t = scenes.transcript("triangle")[0]
    assert np.array_equal(_blocks(t["counts"]), want)
    row = (want.ravel().astype(F) / F(42000)).astype(F)
    assert row[64 + 37] == F(1000) / F(42000) and abs(float(row.astype(np.float64).sum()) - 1) < 640 * 2.0 ** -24


@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_margins_hold_and_few_keypoints_are_undecided(name):
    """the float32 transcription lies inside lo..hi on every keypoint the restatement decides, agrees on the NaN rows, and at most one
    keypoint in ten is undecided as a whole. The intervals stay narrow enough to mean something: under 3 % of the row's mass (a
    deposit of 12 sixths next to a bin edge already opens 24)."""
    s, a, tr = scenes.scene(name), scenes.answer(name), scenes.transcript(name)
    K = len(s["kp"])
    assert a["whole"].sum() * 10 <= K, a["whole"]
    for k in range(K):
        if tr[k] is None:
            assert a["nan"][k] and a["cnt"][k] < 3
            continue
        if a["whole"][k]:
            continue
        assert tr[k]["nan"] == a["nan"][k], k
        c = tr[k]["counts"]
        assert (a["lo"][k] <= c).all() and (c <= a["hi"][k]).all(), (k, np.nonzero((a["lo"][k] > c) | (c > a["hi"][k]))[0])
        if not a["nan"][k]:
            assert (a["hi"][k] - a["lo"][k]).sum() <= 0.03 * a["lo"][k].sum(), k
    print("%s: %d keypoints, %d undecided as a whole, %d maybe attempts, slack %d of %d sixths"
          % (name, K, a["whole"].sum(), a["maybes"].sum(), (a["hi"] - a["lo"]).sum(), a["lo"].sum()))


def _classes(name):
    tr = [t for t in scenes.transcript(name) if t is not None and not t["nan"]]
    tri = sum(np.bincount(t["tri"], minlength=3) for t in tr)
    line = sum(np.bincount(t["line"].ravel(), minlength=3) for t in tr)
    return tr, tri, line


def test_scenes_sit_where_they_claim():
    a = scenes.answer("generic")
    assert (a["cnt"] == 0).sum() == 2 and a["nan"].sum() == 2 and a["cnt"].max() > 150
    _, tri, line = _classes("generic")
    assert (line > 1000).all() and tri[ref.OUT] > 1000 and tri[ref.MIXED] > 1000            # every line class, two triangle classes
    a = scenes.answer("counts")
    assert a["cnt"].tolist() == scenes.COUNTS and a["nan"].tolist() == [n < 3 for n in scenes.COUNTS]
    assert scenes.CAP in scenes.COUNTS and scenes.CAP + 1 in scenes.COUNTS and max(scenes.COUNTS) > 2 * scenes.CAP
    # (d) collinear: every attempt is rejected by an exact zero, the cap is reached
    a = scenes.answer("collinear")
    assert a["cnt"].tolist() == [9, 5, 5] and a["nan"].all() and not a["whole"].any()
    assert all(t["nan"] for t in scenes.transcript("collinear"))
    # (e) the disc: every LINE is inside, so of the D2 blocks and of the ratio block only "in" fills. A triangle is OUT by the rule
    # sum inside <= 21 however full its cells are, so the few small triangles fill A3 out and D3 out; none is mixed.
    a = scenes.answer("disc")
    tr, tri, line = _classes("disc")
    assert a["cnt"].min() > 900 and line[ref.OUT] == 0 and line[ref.MIXED] == 0 and tri[ref.MIXED] == 0 and tri[ref.IN] > 20 * tri[ref.OUT]
    for k in range(4):
        blocks = _blocks(a["hi"][k])
        assert not blocks[[2, 5, 7, 8, 9]].any() and _blocks(a["lo"][k])[6].sum() <= 3 * 3 * 1000 <= blocks[6].sum()
    # (f) two clusters: all three line classes, the ratio block fills
    a = scenes.answer("two_clusters")
    _, tri, line = _classes("two_clusters")
    assert (line > 500).all() and (tri > 50).all()
    assert (_blocks(a["lo"].sum(0))[9].sum() > 6 * 500) and (a["lo"].reshape(-1, 10, B)[:, 9].sum(1) > 0).all()
    # (g) the copy: the same balls at other indices
    s, a = scenes.scene("copy"), scenes.answer("copy")
    assert np.array_equal(a["cnt"][:4], a["cnt"][4:]) and np.array_equal(a["lo"][:4], a["lo"][4:]) and np.array_equal(a["hi"][:4], a["hi"][4:])
    # the blob starts at index 25 of object 0 and at 115 + 140 of the batch in object 1
    assert all(np.array_equal(s["xyz"][a["balls"][k]], s["xyz"][a["balls"][k + 4]]) and np.array_equal(a["balls"][k] + 230, a["balls"][k + 4])
               for k in range(4))
    # (h) and the sample counts
    assert sorted({scenes.scene(n)["n_samples"] for n in scenes.SCENES}) == [1000, 2000, 20000]
    assert all(scenes.scene(n)["n_samples"] % 256 for n in scenes.SCENES) and len(scenes.scene("full")["kp"]) <= 4


def test_scale_bounds_contain_the_model():
    """the bound the device tests hold scale_out to contains the float32 model of step 3 on every scene"""
    for name in scenes.SCENES:
        s, a = scenes.scene(name), scenes.answer(name)
        for k in np.nonzero(a["cnt"] >= 3)[0]:
            P = s["xyz"][a["balls"][k]]
            c64, c_err, m64, m_err = ref.scale_bounds(P, s["kp"][k], s["radius"], a["scale"][k, :3])
            assert (np.abs(a["scale"][k, :3].astype(np.float64) - c64) <= c_err).all()
            assert abs(float(a["scale"][k, 3]) - m64) <= m_err


# ------------------------------------------------------------------------------------------------ host layer
def test_header_and_binding(pkg):
    h = open(os.path.join(ROOT, "include", "ismhip.h")).read()
    assert re.search(r"int\s+ismhip_esf_local\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, const uint32_t\* kp_offsets_h,", h)
    assert re.search(r"#define ISMHIP_ESF_DIM\s+640\b", h) and re.search(r"#define ISMHIP_ESF_SAMPLES\s+20000\b", h)
    assert re.search(r"#define ISMHIP_ESF_SEED\s+0x45534631u", h)
    assert '"esf_local"' in h and "features/features_esf_local.cpp" in h and "0x9E3779B1" in h and "0x7FEB352D" in h and "0x846CA68B" in h
    capi = pkg.capi
    assert "ismhip_esf_local" in capi.EXPORTS and callable(capi.esf_local)
    assert capi.ESF_DIM == ref.DIM == 640 and capi.ESF_SAMPLES == ref.SAMPLES and capi.ESF_SEED == ref.SEED
    assert hasattr(capi.lib(), "ismhip_esf_local")
    assert pkg.pipeline.IsmConfig(feature="ESF_LOCAL").dim == 640


def _cfg(features):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Children"]["Features"] = features
    return json.dumps(j)


def test_host_reads_esf_local_and_reports_its_length(tmp_path):
    """refused before this descriptor was built: this test fails on the parent commit"""
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "ESF_LOCAL", "Parameters": {"Radius": 0.35, "ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}))
    want = json.loads(m.config_to_json())
    out = want["Children"]["Features"]
    assert out["Type"] == "ESF_LOCAL" and out["Parameters"]["Radius"] == pytest.approx(0.35)
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m.h.value)) == 640
    path = str(tmp_path / "esf.ism")
    m.write(path)
    m2 = hb.Model()
    m2.read(path, training=True)
    assert json.loads(m2.config_to_json()) == want
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m2.h.value)) == 640
    m.close(); m2.close()


def test_host_default_radius():
    m = hb.Model()
    m.config_from_json(_cfg({"Type": "ESF_LOCAL", "Parameters": {"ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}}))
    assert json.loads(m.config_to_json())["Children"]["Features"]["Parameters"]["Radius"] == pytest.approx(0.1)
    m.close()


def test_shipped_esf_local_config_loads():
    m = hb.Model()
    m.read(os.path.join(ROOT, "config", "modelnet10_esf_local.ism"), training=True)
    out = json.loads(m.config_to_json())["Children"]
    assert out["Features"]["Type"] == "ESF_LOCAL" and out["Keypoints"]["Type"] == "VoxelGrid"
    assert out["Features"]["Parameters"]["Radius"] == pytest.approx(0.4)
    assert hb.lib().ism3d_descriptor_length(C.c_void_p(m.h.value)) == 640
    rsd = json.load(open(os.path.join(ROOT, "config", "modelnet10_rsd.ism")))["ObjectConfig"]
    esf = json.load(open(os.path.join(ROOT, "config", "modelnet10_esf_local.ism")))["ObjectConfig"]
    rsd["Children"]["Features"]["Parameters"].pop("UseFullRSDHistogram")
    rsd["Children"]["Features"]["Type"] = "ESF_LOCAL"
    assert rsd == esf                                                    # the value set of the RSD configuration, the feature replaced
    m.close()


def test_pfh_is_still_refused_and_the_message_names_esf_local():
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: SHOT, BSHOT, CSHOT, FPFH, SHORT_SHOT, SHORT_CSHOT, ESF_LOCAL, "
                                           r"CGF, RIFT, SpinImage, RSD, CoSPAIR\)"):
        m.config_from_json(_cfg({"Type": "PFH", "Parameters": {}}))
    with pytest.raises(hb.HostError, match="outside the MI355X hot path"):
        m.config_from_json(_cfg({"Type": "ESF", "Parameters": {}}))
    m.close()

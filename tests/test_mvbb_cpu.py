"""The MVBB definition without a GPU (-m "not gpu"): the float64 restatement mvbb_ref.py against the real libgdiam-1.3's answers
recorded in tests/golden/mvbb_gdiam.json, known answers, the scenes' share of undecided regions, and the host's configuration.

GDIAM_TOL: the restatement's largest relative deviation from the fixture, measured when the fixture was made, is 2.2e-8 (volume of box2;
extents 1.9e-8, centre 4.8e-9 of the scene's scale, axes 2e-8 rad); ten times that for the libm of another platform. It is libgdiam's
rectangle arithmetic (tan / atan2) that the deviation measures, not the restatement's."""
import json
import os

import numpy as np
import pytest

import host_binding as hb
import mvbb_ref as mr
import mvbb_scenes as ms

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GDIAM_TOL = 2.2e-7
OTHER_BOX = ms.FIXTURE_OTHER_BOX
_cache = {}


def golden():
    with open(os.path.join(HERE, "golden", "mvbb_gdiam.json")) as f:
        return json.load(f)


def fixture_boxes():
    if "boxes" not in _cache:
        _cache["boxes"] = {k: mr.box(p) for k, p in ms.fixture_scenes().items()}
    return _cache["boxes"]


def test_fixture_inputs_are_the_recorded_ones():
    g = golden()
    scenes = ms.fixture_scenes()
    assert sorted(g) == sorted(scenes)
    for k, p in scenes.items():
        assert g[k]["sha256"] == ms.checksum(p) and g[k]["n"] == len(p), k


@pytest.mark.parametrize("name", sorted(ms.fixture_scenes()))
def test_restatement_against_gdiam(name):
    e, b = golden()[name], fixture_boxes()[name]
    assert b["undecided_at"] == mr.TRACE, "a fixture scene must leave nothing undecided"
    scale = np.abs(ms.fixture_scenes()[name]).max()
    if name in OTHER_BOX:                                     # see mvbb_scenes.FIXTURE_OTHER_BOX: a smaller box, by libgdiam's own noise
        assert b["volume"] < e["volume"] * (1 - 1e-3)
        return
    assert abs(b["volume"] / e["volume"] - 1) <= GDIAM_TOL
    assert np.abs(np.sort(b["size"]) / np.sort(e["extents"]) - 1).max() <= GDIAM_TOL
    assert np.abs(np.asarray(b["center"]) - e["center"]).max() <= GDIAM_TOL * scale
    d = np.abs(np.asarray(b["axes"]) @ np.asarray(e["axes"]).T)                 # up to order and sign: each axis has its partner
    assert sorted(d.argmax(1).tolist()) == [0, 1, 2]
    assert np.sqrt(np.maximum(0.0, 1.0 - d.max(1) ** 2)).max() <= GDIAM_TOL     # sine of the angle between partners


def test_scenes_leave_few_regions_undecided():
    bt = ms.batch()
    und = [r[0] for r in bt["regions"] if mr.region_box(*ms.region_points(bt, r))["undecided_at"] < mr.TRACE]
    assert len(und) * 20 <= len(bt["regions"]), und
    assert not set(und) & set(ms.fixture_scenes())


def test_work_buffer_scenes_are_larger_than_the_lds_staging():
    o = ms.objects()
    assert all(len(o[k]) > ms.LDS_SURVIVORS for k in ms.WORK_BUFFER_SCENES)
    ring = mr.box(o["circle_1000"])
    assert max(ring["trace"][9::4]) == 1000                   # every point a hull vertex, hence a survivor of any pre-filter
    assert mr.box(o["ellipsoid_surface"])["undecided_at"] == mr.TRACE


def test_pair_search_in_blocks_of_rows():
    p = ms.ellipsoid_cloud(150, (1.0, 0.7, 0.4), 3).astype(np.float64)
    p[17] = p[140]                                             # a pair of distance 0 and many equal distances to both
    assert mr.farthest_pair(p, rows=7) == mr.farthest_pair(p, rows=256) == mr.farthest_pair(p, rows=1)
    i, j, d2, gap = mr.farthest_pair(p)
    d = np.linalg.norm(p[:, None] - p[None], axis=2)
    assert i < j and abs(d2 - d.max() ** 2) < 1e-12 and gap > 0


def test_known_box():
    b = mr.box(ms.known_box_corners())
    assert np.allclose(b["size"], ms.KNOWN_BOX_SIZE, rtol=0, atol=1e-6)
    assert abs(b["volume"] - 6.0) <= 1e-5
    want = ms.KNOWN_BOX_ROT.T                                  # rows: the box's axes, longest first
    for k in range(3):
        assert abs(abs(np.dot(b["axes"][k], want[k])) - 1.0) <= 1e-6
    assert np.allclose(b["center"], [0.5, -1.0, 2.0], atol=1e-6)
    a = np.asarray(b["axes"])
    assert np.linalg.det(a) > 0 and all(a[k][np.argmax(np.abs(a[k]))] > 0 for k in (0, 1))


def test_degenerate_inputs():
    one = mr.box(np.array([[0.25, -1.5, 3.0]], np.float32))
    assert one["axes"] == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]] and one["size"] == [0.0] * 3 and one["center"] == [0.25, -1.5, 3.0]
    assert one["trace"][6] == 1 and one["volume"] == 0.0
    same = mr.box(np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (5, 1)))
    assert same["size"] == [0.0] * 3 and same["center"] == [1.0, 2.0, 3.0] and same["trace"][6] == 1
    none = mr.box(np.zeros((0, 3), np.float32))
    assert np.isnan(none["center"]).all() and np.isnan(none["axes"]).all() and none["size"] == [0.0] * 3 and none["n"] == 0
    two = mr.box(np.array([[0, 0, 0], [1, 2, -0.5]], np.float32))
    assert two["trace"][:4] == [0, 1, 0, 1] and two["trace"][5] == 1 and abs(two["size"][0] - np.sqrt(5.25)) < 1e-12 and two["size"][1] < 1e-12
    line = mr.box(ms.objects()["collinear"])
    assert line["trace"][:2] == [0, 49] and line["trace"][5] == 1 and line["size"][1] < 1e-6


def test_ties_go_to_the_lowest_pair():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)       # a unit square: two equal diagonals, (0, 3) before (1, 2)
    assert mr.farthest_pair(p.astype(np.float64))[:2] == (0, 3)
    b = mr.box(p)
    # the box of the two diagonals; flat, so no round can make its volume strictly smaller and it stays
    assert b["trace"][:2] == [0, 3] and b["volume"] == 0.0 and np.allclose(b["size"], [2 ** 0.5, 2 ** 0.5, 0], atol=1e-12)


# ---- host -----------------------------------------------------------------------------------------------------------------------
def config(name):
    with open(os.path.join(ROOT, "config", name)) as f:
        return f.read()


def test_mvbb_config_loads_and_round_trips():
    text = config("modelnet10_shot_mvbb.ism")
    assert text.replace('"MVBB"', '"AABB"') == config("modelnet10_shot.ism")           # the one value changed
    m = hb.Model()
    m.read(os.path.join(ROOT, "config", "modelnet10_shot_mvbb.ism"), training=True)
    dumped = m.config_to_json()
    assert json.loads(dumped)["Parameters"]["BoundingBoxType"] == "MVBB"
    m2 = hb.Model()
    m2.config_from_json(dumped)
    assert m2.config_to_json() == dumped
    m.close(); m2.close()


def test_unknown_bounding_box_type_is_refused_at_train():
    m = hb.Model()
    j = json.loads(config("modelnet10_shot.ism"))["ObjectConfig"]
    j["Parameters"]["BoundingBoxType"] = "OBB"
    m.config_from_json(json.dumps(j))                          # read as any string, as the reference does
    p = ms.box_cloud(32, (1.0, 1.0, 1.0), 1)
    m.add_training(p, np.tile(np.float32([0, 0, 1]), (32, 1)), 0, 0)
    with pytest.raises(hb.HostError, match="invalid bounding box type: OBB"):
        m.train()
    m.close()


def test_exported_symbols():
    import __graft_entry__ as ge
    capi = ge.load_package().capi
    assert "ismhip_region_mvbb" in capi.EXPORTS and capi.MVBB_ROUNDS == mr.ROUNDS and capi.MVBB_TRACE == mr.TRACE
    assert hasattr(capi.lib(), "ismhip_region_mvbb")
    assert hasattr(hb.lib(), "ism3d_last_train_boxes") and hasattr(hb.lib(), "ism3d_last_global_boxes")
    with open(os.path.join(ROOT, "include", "ismhip.h")) as f:
        h = f.read()
    assert "#define ISMHIP_MVBB_ROUNDS 10" in h and "#define ISMHIP_MVBB_TRACE  48" in h

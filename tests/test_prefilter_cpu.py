"""Point-cloud pre-filters without a GPU: hand-derived answers for the restatement in tests/prefilter_ref.py (the checker of
tests/test_gpu_prefilter.py), and the host configuration (libism3d_amd.so): configs with the outlier removals and the z cut-off load
and round-trip, smoothing and voxel filtering are still refused."""
import json
import math
import os

import numpy as np
import pytest

import host_binding as hb
import prefilter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "modelnet10_shot.ism")


def test_sor_collinear_known_answer():
    # nine unit-spaced points on a line and one point 20 further on, MeanK = 2: the two nearest others of an interior point are at 1 and
    # 1 (mean 1), of an end point at 1 and 2 (mean 1.5), of the far point at 20 and 21 (mean 20.5)
    x = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 28], np.float32)
    xyz = np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)
    perm = np.random.default_rng(3).permutation(10)              # the answer may not depend on the point order
    keep, md, thr = ref.sor(xyz[perm], mean_k=2, stddev_mul=1.0)
    want = np.array([1.5, 1, 1, 1, 1, 1, 1, 1, 1.5, 20.5], np.float32)
    assert np.array_equal(md, want[perm])
    s, q, n = 2 * 1.5 + 7 * 1.0 + 20.5, 2 * 2.25 + 7 * 1.0 + 420.25, 10
    thr_want = s / n + 1.0 * math.sqrt((q - s * s / n) / (n - 1))   # 3.05 + sqrt(37.636...) = 9.1848...
    assert thr == pytest.approx(thr_want, rel=1e-14)
    assert 9.18 < thr < 9.19
    assert np.array_equal(keep, (want <= thr)[perm]) and keep.sum() == 9
    # a multiplier large enough keeps the far point too: 20.5 <= 3.05 + 3 * 6.1348
    assert ref.sor(xyz, 2, 3.0)[0].all()


def test_sor_duplicates_nan_and_small_objects():
    # duplicates count as neighbours at distance 0: three coincident points and one at distance 2, MeanK = 2
    xyz = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [2, 0, 0]], np.float32)
    _, md, _ = ref.sor(xyz, 2, 1.0)
    assert np.array_equal(md, np.array([0, 0, 0, 2], np.float32))
    # a non-finite point is never a neighbour and is dropped; the others are as without it
    x = np.arange(6, dtype=np.float32)
    line = np.stack([x, 0 * x, 0 * x], axis=1)
    with_nan = np.concatenate([line[:3], [[np.nan, 0, 0]], line[3:], [[1, np.inf, 0]]]).astype(np.float32)
    keep, md, thr = ref.sor(with_nan, 2, 5.0)
    k0, md0, thr0 = ref.sor(line, 2, 5.0)
    fin = np.array([1, 1, 1, 0, 1, 1, 1, 0], bool)
    assert np.array_equal(keep, fin) and np.isnan(md[~fin]).all() and np.array_equal(md[fin], md0) and thr == thr0
    # fewer than MeanK + 1 finite points: the object is kept whole (its finite points), no statistics
    keep, md, thr = ref.sor(with_nan, 6, 0.0)
    assert np.array_equal(keep, fin) and np.isnan(md).all() and thr == np.inf
    with pytest.raises(ValueError):
        ref.sor(line, 0, 1.0)


def test_ror_lattice_known_answer():
    # 4 x 4 x 4 unit lattice, 1 < r < sqrt(2): a point sees itself and its axis neighbours: 7 inside, 6 on a face, 5 on an edge, 4 at a corner
    g = np.arange(4, dtype=np.float32)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    border = ((xyz == 0) | (xyz == 3)).sum(axis=1)               # 0 inside, 1 face, 2 edge, 3 corner
    for r in (1.2, 1.4):
        keep, cnt = ref.ror(xyz * np.float32(0.5), r * 0.5, 5)
        assert np.array_equal(cnt, 7 - border)
        assert np.array_equal(keep, border < 2)                  # count > 5: inside and faces
    # the comparison is strict: at r = 1 exactly (r2 = 1, d2 = 1) only the point itself counts
    assert np.array_equal(ref.ror(xyz, 1.0, 0)[1], np.ones(64, np.int64))
    assert not ref.ror(xyz, 1.0, 1)[0].any() and ref.ror(xyz, 1.0, 0)[0].all()


def test_passthrough_limits_are_inclusive():
    z = np.array([0.0, 1.5, -1e-7, np.nextafter(np.float32(1.5), np.float32(2)), 0.7, np.nan, 0.7], np.float32)
    xyz = np.stack([np.zeros_like(z), np.zeros_like(z), z], axis=1)
    xyz[6, 0] = np.inf                                           # non-finite in x: dropped although z is inside
    assert np.array_equal(ref.passthrough_z(xyz, 0.0, 1.5), np.array([1, 1, 0, 0, 1, 0, 0], bool))


def test_prefilter_sequence_runs_each_filter_on_the_previous_output():
    rng = np.random.default_rng(5)
    xyz = np.concatenate([rng.normal(size=(400, 3)) * 0.1 + [0, 0, 1], rng.uniform(-3, 3, size=(20, 3))]).astype(np.float32)
    idx = ref.prefilter(xyz, use_sor=True, mean_k=8, stddev_mul=1.0, use_ror=True, radius=0.08, min_neighbors=3, cutoff_z=1.05)
    a = np.nonzero(ref.sor(xyz, 8, 1.0)[0])[0]
    b = a[ref.ror(xyz[a], 0.08, 3)[0]]
    c = b[ref.passthrough_z(xyz[b], 0.0, 1.05)]
    assert np.array_equal(idx, c) and 0 < len(c) < len(b) < len(a) < len(xyz)


def _cfg(**params):
    j = json.load(open(CFG))["ObjectConfig"]
    j["Parameters"].update(params)
    return json.dumps(j)


def test_host_config_with_outlier_removal_loads_and_round_trips():
    m = hb.Model()
    m.config_from_json(_cfg(UseStatisticalOutlierRemoval=True, OutlierRemovalMeanK=12, OutlierRemovalStddevMul=1.5, UseRadiusOutlierRemoval=True,
                            OutlierRemovalMinNeighbors=4, OutlierRemovalRadius=0.03, CutoffDistanceZAxis=1.25))
    p = json.loads(m.config_to_json())["Parameters"]
    assert p["UseStatisticalOutlierRemoval"] is True and p["UseRadiusOutlierRemoval"] is True
    assert p["OutlierRemovalMeanK"] == 12 and p["OutlierRemovalMinNeighbors"] == 4
    assert p["OutlierRemovalStddevMul"] == pytest.approx(1.5) and p["OutlierRemovalRadius"] == pytest.approx(0.03)
    assert p["CutoffDistanceZAxis"] == pytest.approx(1.25)
    assert p["UseSmoothing"] is False and p["UseVoxelFiltering"] is False
    m.close()
    m = hb.Model()                                               # the reference's defaults (implicit_shape_model.cpp:95-103)
    m.config_from_json(_cfg())
    p = json.loads(m.config_to_json())["Parameters"]
    assert p["UseStatisticalOutlierRemoval"] is False and p["UseRadiusOutlierRemoval"] is False
    assert p["OutlierRemovalMeanK"] == 20 and p["OutlierRemovalMinNeighbors"] == 10
    assert p["OutlierRemovalStddevMul"] == pytest.approx(2.0) and p["OutlierRemovalRadius"] == pytest.approx(0.005)
    assert p["CutoffDistanceZAxis"] == 0.0
    m.close()


def test_host_still_refuses_smoothing_and_voxel_filtering():
    for key in ("UseSmoothing", "UseVoxelFiltering"):
        m = hb.Model()
        with pytest.raises(hb.HostError) as e:
            m.config_from_json(_cfg(**{key: True, "UseStatisticalOutlierRemoval": True}))
        msg = str(e.value)
        assert "not built" in msg and "UseSmoothing" in msg and "UseVoxelFiltering" in msg and "outlier" not in msg.lower()
        m.close()
    # a MeanK the search kernel does not take is refused when the config is read, not in the middle of a detection
    for k in (0, 65):
        m = hb.Model()
        with pytest.raises(hb.HostError, match="OutlierRemovalMeanK"):
            m.config_from_json(_cfg(UseStatisticalOutlierRemoval=True, OutlierRemovalMeanK=k))
        m.close()
    m = hb.Model()
    m.config_from_json(_cfg(UseStatisticalOutlierRemoval=False, OutlierRemovalMeanK=65))    # unused: accepted, as in the reference
    m.close()

"""SHORT_SHOT without a GPU: the numpy restatement (short_shot_ref.py) against answers derived by hand from
features/features_short_shot.cpp:77-283, configureSphericalGrid, the host's config handling, and the proof that no neighbour of any
scene the GPU tests use sits within a libm difference of a hard bin decision."""
import json
import math

import numpy as np
import pytest

import host_binding as hb
import short_shot_ref as ssr
import short_shot_scenes as sss
from test_host_layer import _cfg

f32 = np.float32
I9 = sss.IDENTITY
KP0 = f32([0, 0, 0])


def one(points, bins=(2, 2, 8), radius=1.0, frame=I9, kp=KP0, **kw):
    """the restatement on a few points around one keypoint -> (row, count, frac_margin, switch_margin)"""
    return ssr.short_shot_keypoint(np.asarray(points, f32).reshape(-1, 3), kp, frame, radius, bins, **kw)


def row_of(deposits, dim=32):
    """{bin: increment} -> the L2-normalised float32 row, in double as the reference normalises"""
    h = np.zeros(dim)
    for b, v in deposits.items():
        h[b] += v
    return (h / math.sqrt(float((h * h).sum()))).astype(f32)


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_worked_example():
    """(2,2,8), Radius 1, r = 0.6, theta = 60 deg, phi = 30 deg: raw = (1.2, 2/3, 14/3). r: bin 1, decimals 0.2 -> share 0.7 towards
    bin 0. theta: bin 0, decimals 2/3 -> share 5/6 towards bin 1. phi: bin 4, decimals 2/3 -> share 5/6 towards bin 5. Bins
    r + 2 theta + 4 phi: primary 17, phi 21, theta 19, r 16. The float32 point is ~1e-8 off the stated angles and the rad2deg
    constant 8.5e-9 relative: the increments are compared to 1e-6, the bin pattern exactly."""
    th, ph = math.radians(60), math.radians(30)
    p = 0.6 * np.array([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)])
    row, cnt, frac, switch = one([p])
    want = row_of({17: 0.7 + 5 / 6 + 5 / 6, 21: 0.7 + 5 / 6 + 1 / 6, 19: 0.7 + 1 / 6 + 5 / 6, 16: 0.3 + 5 / 6 + 5 / 6})
    assert cnt == 1 and sorted(np.nonzero(row)[0]) == [16, 17, 19, 21]
    assert np.abs(row - want).max() < 1e-6
    assert abs(frac - 1 / 6) < 1e-6 and abs(switch - 1 / 6) < 1e-6


def test_exact_switch_on_the_radial_axis():
    """r = 0.75, Radius 1, two radial bins: raw_r = 1.5 without any libm call -> decimals == 0.5f, share 1.0, secondary towards -1 and
    carrying only the other two shares. The point lies on +x: theta = acos(0) -> raw_theta rounds to 1.0f (bin 1, share 0.5 towards
    bin 0), phi = 0 -> raw_phi = 4.0 (bin 4, share 0.5 towards bin 3)."""
    row, cnt, frac, switch = one([[0.75, 0, 0]])
    assert np.array_equal(row, row_of({1 + 2 + 16: 2.0, 1 + 2 + 12: 2.0, 1 + 0 + 16: 2.0, 0 + 2 + 16: 1.0}))
    assert frac == 0.0                      # ON the switch ...
    assert switch > 2e-8                    # ... and still half a float32 ulp of raw units from the next decision: robust


def test_clamps():
    """theta = 0: secondary clamps onto the primary, none. theta = 180 deg: raw_theta == e_bins, int beyond the last bin, decimals 0.
    phi = +180 deg: raw_phi == a_bins, clamped to bin 7, secondary 6. phi = -180 deg (y = -1e-30; a -0.0 does not survive the dot product's + 0): raw_phi a hair below 0, int 0,
    share just under 0.5, secondary WRAPS to bin 7. r just below Radius: secondary clamps onto the primary."""
    row, *_ = one([[0, 0, 0.5]])            # r bin 1 (raw 1.0) towards 0, theta bin 0, phi = atan2(0, 0) = 0: bin 4 towards 3
    assert np.array_equal(row, row_of({1 + 0 + 16: 1.5, 1 + 0 + 12: 1.5, 0 + 0 + 16: 1.5}))
    row, *_ = one([[0, 0, -0.5]])           # theta bin clamped to 1, secondary 0
    assert np.array_equal(row, row_of({1 + 2 + 16: 1.5, 1 + 2 + 12: 1.5, 1 + 0 + 16: 1.5, 0 + 2 + 16: 1.5}))
    row, *_ = one([[-0.5, 0.0, 0]])         # phi = +180: bin 7, secondary 6; theta = 90: bin 1 towards 0
    assert np.array_equal(row, row_of({1 + 2 + 28: 1.5, 1 + 2 + 24: 1.5, 1 + 0 + 28: 1.5, 0 + 2 + 28: 1.5}))
    row, *_ = one([[-0.5, -1e-30, 0]])      # phi = -180: bin 0, secondary wraps to 7
    raw_phi = f32((8 * (math.atan2(-1e-30, -0.5) * ssr.RAD2DEG + 180)) / 360)
    assert raw_phi < 0 and int(raw_phi) == 0
    fp = f32(float(raw_phi) + 0.5)
    assert fp < 0.5
    half = f32(0.5)
    want = row_of({1 + 2 + 0: f32(f32(half + half) + fp), 1 + 2 + 28: f32(f32(half + half) + f32(1 - fp)), 1 + 0 + 0: f32(f32(half + half) + fp),
                   0 + 2 + 0: f32(f32(half + half) + fp)})
    assert np.array_equal(row, want)
    x = np.nextafter(f32(1), f32(0))        # raw_r = 2 x: bin 1, decimals > 0.5 -> towards +1, clamped onto bin 1: no radial secondary
    row, cnt, *_ = one([[x, 0, 0]])
    fr = f32(f32(1 - f32(f32(2 * float(x)) - 1)) + 0.5)
    assert cnt == 1 and np.array_equal(row, row_of({1 + 2 + 16: f32(f32(fr + half) + half), 1 + 2 + 12: f32(f32(fr + half) + half),
                                                    1 + 0 + 16: f32(f32(fr + half) + half)}))
    assert one([[1.0, 0, 0]])[1] == 0       # d2 == Radius^2 is no neighbour


def test_single_bin_axes_have_no_secondary():
    """(1,1,8): whatever the radial and elevation decimals, only the azimuth has a second bin"""
    rng = np.random.default_rng(3)
    for p in rng.uniform(-0.5, 0.5, size=(20, 3)):
        row, cnt, *_ = one([p], bins=(1, 1, 8))
        assert cnt == 1 and np.count_nonzero(row) == 2
        b = np.nonzero(row)[0]
        assert (b[1] - b[0]) in (1, 7)      # neighbouring azimuth bins (7: the wrap)
    row, *_ = one([[0.3, 0, 0]], bins=(1, 1, 8))       # raw_r 0.3 -> f 0.8; raw_theta 0.5 -> f 1.0; raw_phi 4.0 -> f 0.5 towards 3
    fr, ft = f32(f32(0.3) + f32(0.5)), f32(1.0)
    assert f32((1 * (math.acos(0.0) * ssr.RAD2DEG)) / 180) == f32(0.5)              # raw_theta = 0.5000000042 rounds to 0.5f: share 1.0
    assert np.array_equal(row, row_of({4: f32(f32(fr + ft) + f32(0.5)), 3: f32(f32(fr + ft) + f32(0.5))}, 8))


def test_log_radius():
    """default minimum radius 0.1 Radius (the reference's float 0.1f), and an explicit one; a neighbour below it is skipped"""
    for kw, rmin in ((dict(), float(f32(0.1))), (dict(use_min_radius=True, min_radius_relative=0.25), 0.25)):
        mr = ssr.min_radius_of(1.0, log_radius=True, **kw)
        assert float(mr) == float(f32(rmin))
        row, cnt, *_ = one([[0.5, 0, 0], [0.01, 0, 0]], log_radius=True, min_radius=mr)
        raw_r = f32((2 - 1) * (math.log(0.5) - math.log(float(mr))) / math.log(1.0 / float(mr)) + 1)
        assert cnt == 2 and int(raw_r) == 1
        dec = f32(raw_r - f32(1))
        fr = f32(float(dec) + 0.5) if dec <= 0.5 else f32(float(f32(1 - dec)) + 0.5)
        dep = {1 + 2 + 16: f32(f32(fr + f32(0.5)) + f32(0.5)), 1 + 2 + 12: f32(f32(fr + f32(0.5)) + f32(0.5)), 1 + 0 + 16: f32(f32(fr + f32(0.5)) + f32(0.5))}
        if dec <= 0.5:
            dep[0 + 2 + 16] = f32(f32(f32(1 - fr) + f32(0.5)) + f32(0.5))
        assert np.array_equal(row, row_of(dep))
    assert ssr.min_radius_of(1.0) == 0 and ssr.min_radius_of(2.0, use_min_radius=True, min_radius_relative=0.5) == 1.0


def test_zero_norm_row_and_coincident_skip():
    row, cnt, frac, switch = one(np.zeros((0, 3)))
    assert cnt == 0 and np.isnan(row).all() and row.shape == (32,)
    row, cnt, *_ = one([[0, 0, 0], [1e-8, 0, 0]])                  # d2 = 0 and 1e-16 <= 1e-15: counted, both skipped -> 0 / 0
    assert cnt == 2 and np.isnan(row).all()
    a, ca, *_ = one([[0, 0, 0], [1e-8, 0, 0], [4e-8, 0, 0]])       # d2 = 1.6e-15 > 1e-15 contributes: one neighbour is enough
    b, cb, *_ = one([[4e-8, 0, 0]])
    assert ca == 3 and cb == 1 and np.isfinite(a).all() and np.array_equal(a, b)
    row, cnt, *_ = one([[0.5, 0, 0]], min_radius=0.6)
    assert cnt == 1 and np.isnan(row).all()                        # below the minimum radius: no contribution
    row, cnt, *_ = one([[0.5, 0, 0]], frame=sss.NAN_FRAME)
    assert cnt == 0 and np.isnan(row).all()


def test_rotated_frame_and_batch_wrapper():
    """local coordinates are taken in the frame: a point on the frame's x axis gives the row of test_exact_switch in any frame"""
    fr = f32([0, 1, 0, 0, 0, 1, 1, 0, 0])                          # x -> y
    row, *_ = one([[0, 0.75, 0]], frame=fr)
    assert np.array_equal(row, one([[0.75, 0, 0]])[0])
    pts = f32([[0.75, 0, 0], [np.nan, 0, 0], [5, 5.75, 5], [9, 9, 9]])
    desc, cnt, frac, switch = ssr.short_shot_ref(np.uint32([0, 2, 4]), pts, np.uint32([0, 1, 3]), f32([[0, 0, 0], [5, 5, 5], [20, 0, 0]]),
                                                 np.stack([I9, fr, I9]), 1.0, (2, 2, 8))
    assert cnt.tolist() == [1, 1, 0] and np.array_equal(desc[0], row) and np.array_equal(desc[1], row) and np.isnan(desc[2]).all()


# ------------------------------------------------------------------------------------------------ configureSphericalGrid
AUTO = {8: (1, 1, 8), 16: (2, 2, 4), 24: (2, 2, 6), 32: (2, 2, 8), 64: (2, 4, 8), 96: (3, 4, 8), 128: (4, 4, 8), 192: (6, 4, 8), 256: (8, 4, 8)}


def test_configure_spherical_grid(pkg):
    for grid in (ssr.configure_spherical_grid, pkg.capi.short_shot_grid):
        for dims, bins in AUTO.items():
            assert grid(dims) == (dims, bins) and bins[0] * bins[1] * bins[2] == dims
        assert grid(40) == (32, (2, 2, 8)) and grid(0) == (32, (2, 2, 8))                       # unknown size: the fallback
        assert grid(64, "manual", (1, 3, 5)) == (15, (1, 3, 5))                                 # manual: dims follow the bins
        assert grid(64, "spiral", (1, 3, 5)) == (32, (2, 2, 8))                                 # unknown bin type: the fallback
    cfg = pkg.pipeline.IsmConfig(feature="SHORT_SHOT", short_shot_dims=96)
    assert cfg.dim == 96 and cfg.short_shot_grid == (96, (3, 4, 8))
    assert pkg.pipeline.IsmConfig(feature="SHORT_SHOT").dim == 32 and pkg.pipeline.IsmConfig().dim == 352
    assert pkg.pipeline.IsmConfig(feature="SHORT_SHOT", short_shot_bin_type="manual", short_shot_r_bins=1, short_shot_e_bins=3, short_shot_a_bins=5).dim == 15
    for radius, kw in ((0.3, dict(log_radius=True)), (0.3, dict(use_min_radius=True, min_radius_relative=0.4)), (0.3, dict())):
        assert pkg.capi.short_shot_min_radius(radius, **kw) == float(ssr.min_radius_of(radius, **kw))


# ------------------------------------------------------------------------------------------------ host config
def _short_cfg(**params):
    p = {"Radius": 0.3, "ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}
    p.update(params)
    return _cfg(**{"Children/Features": {"Type": "SHORT_SHOT", "Parameters": p}})


def _features_after_roundtrip(cfg):
    m = hb.Model()
    m.config_from_json(cfg)
    out = json.loads(m.config_to_json())["Children"]["Features"]
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())                        # what we write, we read
    assert json.loads(m2.config_to_json())["Children"]["Features"] == out
    m.close(); m2.close()
    return out


def test_host_accepts_short_shot_and_round_trips_its_parameters():
    out = _features_after_roundtrip(_short_cfg())                  # only Radius given: the reference's defaults
    assert out["Type"] == "SHORT_SHOT"
    p = out["Parameters"]
    assert abs(p["Radius"] - 0.3) < 1e-6 and p["UseMinRadius"] is False and p["ShortShotMinRadius"] == 0 and p["ShortShotDims"] == 32
    assert p["ShortShotLogRadius"] is False and (p["ShortShotRBins"], p["ShortShotEBins"], p["ShortShotABins"]) == (2, 2, 8)
    assert p["ShortShotBinType"] == "auto" and p["ReferenceFrameType"] == "SHOT" and abs(p["ReferenceFrameRadius"] - 0.3) < 1e-6
    given = {"Radius": 0.25, "UseMinRadius": True, "ShortShotMinRadius": 0.125, "ShortShotDims": 7, "ShortShotLogRadius": True, "ShortShotRBins": 3,
             "ShortShotEBins": 2, "ShortShotABins": 5, "ShortShotBinType": "manual"}
    p = _features_after_roundtrip(_short_cfg(**given))["Parameters"]
    given["ShortShotDims"] = 30                                    # manual: the dimensions follow the bins
    for k, v in given.items():
        assert p[k] == v, k
    for dims, bins in AUTO.items():                                # auto: the bins follow the dimensions
        p = _features_after_roundtrip(_short_cfg(ShortShotDims=dims, ShortShotRBins=5, ShortShotEBins=5, ShortShotABins=5))["Parameters"]
        assert (p["ShortShotDims"], p["ShortShotRBins"], p["ShortShotEBins"], p["ShortShotABins"]) == (dims, *bins)
    for cfg in (_short_cfg(ShortShotDims=40), _short_cfg(ShortShotBinType="spiral", ShortShotDims=64, ShortShotABins=3)):
        p = _features_after_roundtrip(cfg)["Parameters"]           # the reference's fallback (with its LOG_ERROR)
        assert (p["ShortShotDims"], p["ShortShotRBins"], p["ShortShotEBins"], p["ShortShotABins"]) == (32, 2, 2, 8)


def test_host_reads_the_example_config():
    import os
    path = os.path.join(hb.ROOT, "config", "modelnet10_short_shot.ism")
    out = _features_after_roundtrip(json.dumps(json.load(open(path))["ObjectConfig"]))
    assert out["Type"] == "SHORT_SHOT" and out["Parameters"]["ShortShotDims"] == 32


@pytest.mark.parametrize("params,needle", [
    (dict(ShortShotLogRadius=True, UseMinRadius=True, ShortShotMinRadius=0.0), "ShortShotLogRadius"),
    (dict(ShortShotBinType="manual", ShortShotRBins=8, ShortShotEBins=8, ShortShotABins=8), "more than 256"),
    (dict(ShortShotBinType="manual", ShortShotRBins=0), "fewer than one bin"),
])
def test_host_refuses_what_the_device_does_not_compute(params, needle):
    m = hb.Model()
    with pytest.raises(hb.HostError, match=needle):
        m.config_from_json(_short_cfg(**params))
    m.close()


# ------------------------------------------------------------------------------------------------ switch margins of the GPU scenes
_lrf = {}


def _oracle_frames(ora, case):
    pt_off, p, _, kp_off, kp = case.soa()
    key = (id(case.objs), case.radius)
    if case.frames is None and key not in _lrf:
        _lrf[key] = ora.shot_lrf(pt_off, *[np.ascontiguousarray(p[:, i]) for i in range(3)], kp_off, *[np.ascontiguousarray(kp[:, i]) for i in range(3)], case.radius)
    return case.frames_from(_lrf.get(key))


@pytest.mark.parametrize("case", sss.all_cases(), ids=lambda c: c.name)
def test_gpu_scenes_keep_clear_of_the_switches(ora, case):
    """Device and host libm may differ by a few ulp of double, ~1e-13 in raw units. No raw value of any scene, before its cast to
    float32, lies within 1e-9 of a value where the cast changes int() or `decimals <= 0.5f` (switch_margin) -- so the GPU tests
    exempt no keypoint. A float32 fraction of EXACTLY 0.5 (frac_margin 0) is no danger by itself: such a value sits half a float32
    ulp from the next decision. The lattice places neighbours there on purpose (r and raw_r exact, no libm call); among the millions
    of raw values of the dense balls a few land there by rounding. Every other fraction is at least a float32 step from 0.5.
    The scenes also reach what they are there for."""
    frames = _oracle_frames(ora, case)
    desc, cnt, frac, switch = case.reference(frames)
    finite = np.isfinite(desc).all(1)
    assert np.array_equal(finite, ~np.isnan(desc).any(1))          # rows are NaN as a whole
    print(f"{case.name}: {finite.sum()} of {len(desc)} rows, neighbours {cnt.min()}..{cnt.max()}, switch margin {switch.min():.3g}, frac margin {frac.min():.3g}")
    assert switch.min() >= 1e-9
    assert ((frac == 0.0) | (frac >= 1e-9)).all()
    if case.name.startswith("lattice") and case.bins[0] == 2 and case.radius == 0.5:
        assert (frac == 0.0).all()                                 # r = 3/8 of radius 1/2 on two bins: raw_r = 1.5
    if case.name.startswith("thin"):
        assert len(case.objs) == 9 and cnt.max() > 4096 and finite.all()
    if case.name.startswith("mid") and not case.log_radius and not case.use_min_radius:
        assert cnt[sss.MID_EMPTY_BALL] == 0 and cnt[sss.MID_OFF_GRID] == 0 and cnt[sss.MID_NAN_FRAME] == 0 and cnt[sss.MID_ON_POINT] > 0
        assert finite.sum() == len(desc) - 3 and not finite[[sss.MID_EMPTY_BALL, sss.MID_OFF_GRID, sss.MID_NAN_FRAME]].any()
    if case.name.startswith("queue"):
        _, _, _, counts = sss._queue()
        assert cnt.tolist() == counts.tolist()
        assert finite.all() if case.min_radius_relative < 0.9 else not finite.any()

"""SHORT_CSHOT without a GPU: the numpy restatement (short_cshot_ref.py) against answers derived by hand from
features/features_short_cshot.cpp:103-507, the two grid functions, the colour edge list, the host's config handling, and the proof that
no neighbour of any scene the GPU tests use sits within a libm difference of a hard geometric bin decision of either grid."""
import json
import math
import os

import numpy as np
import pytest

import host_binding as hb
import short_cshot_ref as scr
import short_cshot_scenes as scs
import short_shot_ref as ssr
import short_shot_scenes as sss
from test_host_layer import _cfg

f32 = np.float32
I9 = sss.IDENTITY
KP0 = f32([0, 0, 0])
KP_LAB = f32([0.5, 0.0, 0.0])


def lab_at(cd):
    """a normalised CIELab triple at colour distance cd (as a real number) from KP_LAB: dL = 3 cd - 0.1, da = db = 0.1"""
    return f32([0.5 + (3 * cd - 0.1), 0.1, -0.1])


def one(points, labs, bins=(2, 2, 8), color_bins=(2, 2, 8), hist_size=15, radius=1.0, frame=I9, kp=KP0, kp_lab=KP_LAB, **kw):
    """the restatement on a few points around one keypoint -> (row, count, switch_margin)"""
    return scr.short_cshot_keypoint(np.asarray(points, f32).reshape(-1, 3), np.asarray(labs, f32).reshape(-1, 3), kp, kp_lab, frame, radius, bins,
                                    color_bins, hist_size, **kw)


def row_of(deposits, dim):
    """{bin: increment} -> the L2-normalised float32 row, in double as the reference normalises"""
    h = np.zeros(dim)
    for b, v in deposits.items():
        h[b] += v
    return (h / math.sqrt(float((h * h).sum()))).astype(f32)


def polar(r, theta_deg, phi_deg):
    th, ph = math.radians(theta_deg), math.radians(phi_deg)
    return r * np.array([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)])


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_worked_example():
    """Shape (2,2,8), colour grid (2,2,8), H = 15, Radius 1; one neighbour at r = 0.6, theta = 60 deg, phi = 30 deg with colour
    distance cd = 0.44 / 3. Both grids: raw = (1.2, 2/3, 14/3) -> r bin 1, share 0.7 towards 0; theta bin 0, share 5/6 towards 1; phi
    bin 4, share 5/6 towards 5. raw_c = 2.2 -> colour bin 2, share 0.7 towards 1.
    Shape bins r + 2 theta + 4 phi: primary 17, phi 21, theta 19, r 16 (the SHORT_SHOT worked example).
    Colour bins 32 + c + 15 (r + 2 (theta + 2 phi)): cell 17 -> primary 32 + 2 + 255 = 289; phi: cell 21 -> 349; theta: cell 19 -> 319;
    r: cell 16 -> 274; colour: 288. Increments c + r + theta + phi: 0.7 + 0.7 + 5/6 + 5/6, then with 1/6 for phi, with 1/6 for theta,
    with 0.3 for r, and for the secondary colour bin 0.3 + 0.3 + 5/6 + 5/6 -- (1 - f_r), bug-compatible: the consistent 0.3 + 0.7 + ...
    would be 0.4 larger (checked on a ratio of bins). Float32 inputs are ~1e-8 off the stated values: increments to 1e-6, the bin pattern exactly."""
    row, cnt, switch = one([polar(0.6, 60, 30)], [lab_at(0.44 / 3)])
    a, b = 5 / 6, 1 / 6
    want = {17: 0.7 + a + a, 21: 0.7 + a + b, 19: 0.7 + b + a, 16: 0.3 + a + a,
            289: 0.7 + 0.7 + a + a, 349: 0.7 + 0.7 + a + b, 319: 0.7 + 0.7 + b + a, 274: 0.7 + 0.3 + a + a, 288: 0.3 + 0.3 + a + a}
    assert cnt == 1 and row.shape == (512,) and sorted(np.nonzero(row)[0]) == sorted(want)
    assert np.abs(row - row_of(want, 512)).max() < 1e-6
    # the ratio of two bins of one row is free of the norm: as written (0.6 + 5/3) / (1.4 + 5/3) = 0.739; the consistent 1.0 + 5/3 gives 0.870
    assert abs(float(row[288]) / float(row[289]) - (0.6 + 2 * a) / (1.4 + 2 * a)) < 1e-6
    assert abs(switch - 1 / 6) < 1e-6


def test_colour_part_layout_with_distinct_bin_counts():
    """colour grid (3, 2, 5), H = 4 behind a (1, 1, 8) shape part: raw_r = 1.8 (bin 1 -> 2), raw_theta = 2/3 (0 -> 1), raw_phi =
    5 * 210 / 360 = 2.917 (2 -> 3), raw_c = 4 * 0.44 / 3 = 0.587 (0 -> 1); index 8 + c + 4 (r + 3 (theta + 2 phi))"""
    row, cnt, _ = one([polar(0.6, 60, 30)], [lab_at(0.44 / 3)], bins=(1, 1, 8), color_bins=(3, 2, 5), hist_size=4)
    assert row.shape == (8 + 30 * 4,)
    col = row[8:]
    cell = lambda r, t, p: 4 * (r + 3 * (t + 2 * p))
    assert sorted(np.nonzero(col)[0]) == sorted([cell(1, 0, 2), cell(1, 0, 2) + 1, cell(2, 0, 2), cell(1, 1, 2), cell(1, 0, 3)]) == [52, 53, 56, 64, 76]
    assert int(np.argmax(col)) == 52                                    # the primary bin carries the largest sum


def test_edge_values_of_the_colour_axis():
    p = [polar(0.6, 60, 30)]
    row, *_ = one(p, [lab_at(0.44 / 3)], hist_size=1)                   # H = 1: no secondary colour bin
    assert row.shape == (64,) and sorted(np.nonzero(row[32:])[0]) == [16, 17, 19, 21]
    row, *_ = one(p, [KP_LAB])                                          # cd = 0: raw_c = 0, bin 0, share 0.5; secondary clamps onto it
    a, b = 5 / 6, 1 / 6
    want = {17: 0.7 + a + a, 21: 0.7 + a + b, 19: 0.7 + b + a, 16: 0.3 + a + a,
            32 + 255: 0.5 + 0.7 + a + a, 32 + 315: 0.5 + 0.7 + a + b, 32 + 285: 0.5 + 0.7 + b + a, 32 + 240: 0.5 + 0.3 + a + a}
    assert sorted(np.nonzero(row)[0]) == sorted(want) and np.abs(row - row_of(want, 512)).max() < 1e-6
    row, *_ = one(p, [f32([1, 1, 1])], kp_lab=f32([0, -1, -1]))         # cd = (1 + 2) / 3 = 1 exactly: raw_c = 15 = H, bin clamped to 14,
    col = np.nonzero(row[32:])[0]                                       # decimals 0 -> share 0.5 towards 13
    assert sorted(col % 15) == [13, 14, 14, 14, 14] and sorted(col // 15) == [16, 17, 17, 19, 21]
    row, *_ = one(p, [f32([9, 9, 9])], kp_lab=f32([0, -1, -1]))         # cd beyond 1 is clamped to 1: the same bins
    assert np.array_equal(np.nonzero(row[32:])[0], col)
    row, cnt, _ = one(p, [lab_at(0.44 / 3)], bins=(2, 2, 8), color_bins=(1, 1, 8))    # a colour grid that is not the shape grid
    assert row.shape == (32 + 120,) and sorted(np.nonzero(row[:32])[0]) == [16, 17, 19, 21]
    assert sorted(np.nonzero(row[32:])[0]) == [15 * 4 + 1, 15 * 4 + 2, 15 * 5 + 2]    # colour: only phi and c have a second bin


def test_joint_normalisation_and_shape_part():
    """the two parts are normalised together; the shape part, renormalised, is the SHORT_SHOT row of the same neighbours"""
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.5, 0.5, size=(40, 3)).astype(f32)
    labs = np.stack([rng.uniform(0, 1, 40), rng.uniform(-1, 1, 40), rng.uniform(-1, 1, 40)], 1).astype(f32)
    for bins, cbins, H in scs.MID_CONFIGS:
        row, cnt, _ = one(pts, labs, bins=bins, color_bins=cbins, hist_size=H)
        Ds = bins[0] * bins[1] * bins[2]
        r64 = row.astype(np.float64)
        assert abs(np.linalg.norm(r64) - 1) < 1e-6 and 0.05 < np.linalg.norm(r64[:Ds]) < 0.95
        shape, scnt, *_ = ssr.short_shot_keypoint(pts, KP0, I9, 1.0, bins)
        assert cnt == scnt and np.abs(r64[:Ds] / np.linalg.norm(r64[:Ds]) - shape).max() < 2e-7
        assert (row[Ds:] >= 0).all() and np.count_nonzero(row[Ds:]) > 0


def test_empty_rows_are_nan_as_a_whole():
    row, cnt, switch = one(np.zeros((0, 3)), np.zeros((0, 3)))
    assert cnt == 0 and row.shape == (512,) and np.isnan(row).all() and switch == np.inf
    row, cnt, _ = one([[0, 0, 0], [1e-8, 0, 0]], [KP_LAB, KP_LAB])       # counted, both skipped (d2 <= 1e-15): 0 / 0
    assert cnt == 2 and np.isnan(row).all()
    row, cnt, _ = one([[0.5, 0, 0], [0, 0.3, 0]], [KP_LAB, KP_LAB], min_radius=0.6)      # all below the minimum radius, for both parts
    assert cnt == 2 and np.isnan(row).all()
    row, cnt, _ = one([[0.5, 0, 0], [0, 0.3, 0]], [KP_LAB, KP_LAB], min_radius=0.4)      # one left: enough
    assert cnt == 2 and np.isfinite(row).all() and np.count_nonzero(row[:32]) and np.count_nonzero(row[32:])
    row, cnt, _ = one([[0.5, 0, 0]], [KP_LAB], frame=sss.NAN_FRAME)
    assert cnt == 0 and np.isnan(row).all()


def test_batch_wrapper_takes_lab_once_per_colour(ora):
    calls = []

    def counting(c):
        calls.append(c)
        return ora.rgb2lab(c)

    pts = f32([[0.75, 0, 0], [np.nan, 0, 0], [5, 5.75, 5], [9, 9, 9]])
    rgba = np.uint32([0x102030, 0x102030, 0xFFFFFF, 0x102030])
    desc, cnt, _ = scr.short_cshot_ref(counting, np.uint32([0, 2, 4]), pts, rgba, np.uint32([0, 1, 3]), f32([[0, 0, 0], [5, 5, 5], [20, 0, 0]]),
                                       np.uint32([0x102030, 0xFFFFFF, 0]), np.stack([I9, f32([0, 1, 0, 0, 0, 1, 1, 0, 0]), I9]), 1.0, (2, 2, 8))
    assert sorted(calls) == [0, 0x102030, 0xFFFFFF]
    assert cnt.tolist() == [1, 1, 0] and np.isnan(desc[2]).all()
    assert np.array_equal(desc[0], desc[1])                             # the same local geometry, cd = 0 in both


# ------------------------------------------------------------------------------------------------ the two grid functions
def test_grid_functions(pkg):
    for dims, bins in scr.COLOR_BINS.items():
        assert pkg.capi.short_cshot_color_grid(dims) == scr.configure_spherical_color_grid(dims) == (dims, bins) and bins[0] * bins[1] * bins[2] == dims
    assert sorted(scr.COLOR_BINS) == [8, 16, 24, 32, 64, 96, 128]
    for dims in (0, 40, 192, 256):                                      # 192 and 256 are shape sizes only: the fallback
        assert pkg.capi.short_cshot_color_grid(dims) == scr.configure_spherical_color_grid(dims) == (32, (2, 2, 8))
    for args in ((32,), (256,), (40,), (64, "manual", (1, 3, 5)), (64, "spiral", (1, 3, 5))):
        assert pkg.capi.short_shot_grid(*args) == ssr.configure_spherical_grid(*args)
    C = pkg.pipeline.IsmConfig
    assert C(feature="SHORT_CSHOT").dim == 512
    assert C(feature="SHORT_CSHOT", short_shot_dims=256, short_color_shot_dims=64).dim == 256 + 64 * 15 == 1216
    assert C(feature="SHORT_CSHOT", short_color_shot_dims=8, short_color_shot_hist_size=7, short_shot_bin_type="manual", short_shot_r_bins=1,
             short_shot_e_bins=3, short_shot_a_bins=5).dim == 71
    assert C(feature="SHORT_CSHOT", short_color_shot_dims=40).dim == 512 and C(feature="SHORT_SHOT").dim == 32 and C().dim == 352
    lib = pkg.capi.lib()
    assert hasattr(lib, "ismhip_short_cshot") and "ismhip_short_cshot" in pkg.capi.EXPORTS


# ------------------------------------------------------------------------------------------------ the colour edge list
def test_edge_colour_list(ora):
    """every listed colour gives, through the oracle's rgb2lab, exactly the float32 raw_c its entry names; ordinary colours do not"""
    got = scs.edge_raw_c(ora.rgb2lab, [c for c, _, _ in scs.EDGE_COLORS])
    want = np.array([scs.edge_value(kind, n) for _, kind, n in scs.EDGE_COLORS], f32)
    assert np.array_equal(got, want)
    assert {k for _, k, _ in scs.EDGE_COLORS} == {"half", "half-below", "half-above", "int", "int-below"}
    assert all(n >= 1 for _, k, n in scs.EDGE_COLORS if k.startswith("int"))
    edges = {float(scs.edge_value(k, n)) for k in ("half", "half-below", "half-above", "int", "int-below") for n in range(16)}
    assert not set(scs.edge_raw_c(ora.rgb2lab, range(1000, 1200)).astype(float).tolist()) & edges
    case = scs.lattice_case()
    for (p, _), rgba in zip(case.geo.objs, case.rgba):
        inside = (p.astype(np.float64) ** 2).sum(1) < 0.25 ** 2
        assert {c for c, _, _ in scs.EDGE_COLORS} <= set(rgba[inside].tolist())        # all inside the smallest radius


# ------------------------------------------------------------------------------------------------ host config
ELEVEN = {"Radius": 0.1, "UseMinRadius": False, "ShortShotMinRadius": 0, "ShortShotDims": 32, "ShortColorShotDims": 32, "ShortColorShotHistSize": 15,
          "ShortShotLogRadius": False, "ShortShotRBins": 2, "ShortShotEBins": 2, "ShortShotABins": 8, "ShortShotBinType": "auto"}


def _short_cfg(**params):
    p = {"ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}
    p.update(params)
    return _cfg(**{"Children/Features": {"Type": "SHORT_CSHOT", "Parameters": p}})


def _features_after_roundtrip(cfg):
    m = hb.Model()
    m.config_from_json(cfg)
    out = json.loads(m.config_to_json())["Children"]["Features"]
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())                        # what we write, we read
    assert json.loads(m2.config_to_json())["Children"]["Features"] == out
    m.close(); m2.close()
    return out


def test_host_accepts_short_cshot_and_round_trips_its_parameters():
    out = _features_after_roundtrip(_short_cfg())                  # nothing given: the reference's eleven defaults (:23-33)
    assert out["Type"] == "SHORT_CSHOT"
    p = out["Parameters"]
    for k, v in ELEVEN.items():
        assert k in p and (abs(p[k] - v) < 1e-6 if isinstance(v, float) else p[k] == v), k
    given = {"Radius": 0.25, "UseMinRadius": True, "ShortShotMinRadius": 0.125, "ShortShotDims": 7, "ShortColorShotDims": 64, "ShortColorShotHistSize": 9,
             "ShortShotLogRadius": True, "ShortShotRBins": 3, "ShortShotEBins": 2, "ShortShotABins": 5, "ShortShotBinType": "manual"}
    p = _features_after_roundtrip(_short_cfg(**given))["Parameters"]
    given["ShortShotDims"] = 30                                    # manual: the shape dimensions follow the bins
    for k, v in given.items():
        assert p[k] == v, k
    for dims in (8, 16, 24, 32, 64):                               # all seven sizes are accepted; at H = 15 these fit the 1344 cap
        assert _features_after_roundtrip(_short_cfg(ShortColorShotDims=dims))["Parameters"]["ShortColorShotDims"] == dims
    for dims in (96, 128):
        assert _features_after_roundtrip(_short_cfg(ShortColorShotDims=dims, ShortColorShotHistSize=5))["Parameters"]["ShortColorShotDims"] == dims
    for dims in (40, 192, 0):                                      # the reference's fallback (with its LOG_ERROR); there is no manual colour grid
        assert _features_after_roundtrip(_short_cfg(ShortColorShotDims=dims, ShortShotBinType="manual"))["Parameters"]["ShortColorShotDims"] == 32
    p = _features_after_roundtrip(_short_cfg(ShortShotDims=40))["Parameters"]
    assert (p["ShortShotDims"], p["ShortShotRBins"], p["ShortShotEBins"], p["ShortShotABins"]) == (32, 2, 2, 8)


def test_host_reads_the_example_config():
    path = os.path.join(hb.ROOT, "config", "kinect_short_cshot.ism")
    src = json.load(open(path))["ObjectConfig"]
    out = _features_after_roundtrip(json.dumps(src))
    assert out["Type"] == "SHORT_CSHOT"
    for k, v in ELEVEN.items():
        if k != "Radius":
            assert out["Parameters"][k] == v, k
    assert abs(out["Parameters"]["Radius"] - 0.05) < 1e-7
    other = json.load(open(os.path.join(hb.ROOT, "config", "kinect_cshot.ism")))["ObjectConfig"]
    for j in (src, other):                                         # the value set of kinect_cshot.ism, the Features section apart
        del j["Children"]["Features"]
    assert src == other


@pytest.mark.parametrize("params,needle", [
    (dict(ShortShotDims=256, ShortColorShotDims=128), "longer than 1344"),                                       # 256 + 128 * 15 = 2176
    (dict(ShortColorShotDims=64, ShortColorShotHistSize=21), "longer than 1344"),                                # 32 + 64 * 21 = 1376
    (dict(ShortColorShotHistSize=0), "ShortColorShotHistSize"),
    (dict(ShortShotLogRadius=True, UseMinRadius=True, ShortShotMinRadius=0.0), "ShortShotLogRadius"),
    (dict(ShortShotLogRadius=True, UseMinRadius=True, ShortShotMinRadius=1.0), "ShortShotLogRadius"),
    (dict(ShortShotBinType="manual", ShortShotRBins=8, ShortShotEBins=8, ShortShotABins=8), "more than 256"),
    (dict(ShortShotBinType="manual", ShortShotRBins=0), "fewer than one bin"),
])
def test_host_refuses_what_the_device_does_not_compute(params, needle):
    m = hb.Model()
    with pytest.raises(hb.HostError, match=needle):
        m.config_from_json(_short_cfg(Radius=0.3, **params))
    m.close()


def test_host_accepts_exactly_1344():
    p = _features_after_roundtrip(_short_cfg(ShortShotDims=256, ShortColorShotDims=64, ShortColorShotHistSize=17))["Parameters"]     # 256 + 64 * 17
    assert (p["ShortShotDims"], p["ShortColorShotDims"], p["ShortColorShotHistSize"]) == (256, 64, 17)


def test_host_refuses_a_colourless_cloud_before_any_device_work():
    """on the host, so also on a machine without a GPU: training and detection throw for a cloud without colours"""
    rng = np.random.default_rng(9)
    xyz = rng.normal(size=(200, 3)).astype(f32)
    nrm = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(f32)
    m = hb.Model()
    m.config_from_json(_short_cfg(Radius=0.3))
    m.add_training(xyz, nrm, 0, 0)
    with pytest.raises(hb.HostError, match="SHORT_CSHOT needs coloured point clouds"):
        m.train()
    with pytest.raises(hb.HostError, match="SHORT_CSHOT needs coloured point clouds"):
        m.detect_batch(np.uint32([0, 200]), xyz, nrm, max_maxima=4)
    m.close()


# ------------------------------------------------------------------------------------------------ switch margins of the GPU scenes
_lrf = {}


def _oracle_frames(ora, geo):
    pt_off, p, _, kp_off, kp = geo.soa()
    key = (id(geo.objs), geo.radius)
    if geo.frames is None and key not in _lrf:
        _lrf[key] = ora.shot_lrf(pt_off, *[np.ascontiguousarray(p[:, i]) for i in range(3)], kp_off, *[np.ascontiguousarray(kp[:, i]) for i in range(3)], geo.radius)
    return geo.frames_from(_lrf.get(key))


@pytest.mark.parametrize("case", scs.parity_cases(), ids=lambda c: c.name)
def test_gpu_scenes_keep_clear_of_the_switches(ora, case):
    """Device and host libm may differ by a few ulp of double, ~1e-13 in raw units. No geometric raw value of any GPU case, on the
    shape grid or on the colour grid, lies before its cast to float32 within 1e-9 of a value where the cast changes int() or
    `decimals <= 0.5f` -- so the GPU tests exempt no keypoint. (raw_c takes no libm call: no margin is involved.) The scenes also reach
    what they are there for."""
    geo = case.geo
    desc, cnt, switch = case.reference(ora.rgb2lab, _oracle_frames(ora, geo))
    finite = np.isfinite(desc).all(1)
    assert np.array_equal(finite, ~np.isnan(desc).any(1))          # rows are NaN as a whole
    print(f"{case.name}: {finite.sum()} of {len(desc)} rows of {case.dim}, neighbours {cnt.min()}..{cnt.max()}, switch margin {switch.min():.3g}")
    assert desc.shape[1] == case.dim
    assert switch.min() >= 1e-9
    Ds = geo.bins[0] * geo.bins[1] * geo.bins[2]
    if finite.any():
        assert (np.abs(desc[finite][:, Ds:]).sum(1) > 0).all() and (np.abs(desc[finite][:, :Ds]).sum(1) > 0).all()     # both parts populated
    if geo.name.startswith("thin"):
        assert len(geo.objs) == 9 and cnt.max() > 4096 and finite.all()
    if geo.name.startswith("mid") and not geo.log_radius:
        assert cnt[sss.MID_EMPTY_BALL] == 0 and cnt[sss.MID_OFF_GRID] == 0 and cnt[sss.MID_NAN_FRAME] == 0 and cnt[sss.MID_ON_POINT] > 0
        assert finite.sum() == len(desc) - 3
    if geo.name.startswith("queue"):
        assert cnt.tolist() == sss._queue()[3].tolist()
        assert finite.all() if geo.min_radius_relative < 0.9 else not finite.any()
    if case.tag == "-palette":
        own = np.concatenate(case.rgba) == scs.EDGE_KP_COLOR
        assert 0.25 < own.mean() < 0.45 and set(np.concatenate(case.rgba).tolist()) == {scs.EDGE_KP_COLOR, scs.BLACK, scs.WHITE}
        col = desc[finite][:, Ds:].reshape(finite.sum(), -1, case.hist_size)
        assert (col[:, :, 0].sum(1) > 0).all()                      # colour bin 0 of some cell: the neighbours with cd = 0

"""RIFT on the host (no GPU): the float64 restatement rift_ref.py against answers worked out by hand, the caps on what the GPU tests may
leave undecided on the scenes of rift_scenes.py, the derived tolerances against the project's 1e-4, and the host layer (header, binding,
config, refusals)."""
import json
import os
import re

import numpy as np
import pytest

import host_binding as hb
import rift_ref as ref
import rift_scenes as scenes
from test_host_layer import _cfg

f32 = np.float32


def _pack(r, g, b):
    return ((np.asarray(r, np.int64) << 16) | (np.asarray(g, np.int64) << 8) | np.asarray(b, np.int64)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ hand-derived answers
def test_intensity_is_the_float_formula():
    got = ref.intensity(_pack([255, 0, 0, 10], [0, 255, 0, 20], [0, 0, 255, 30]))
    want = [f32(0.299) * f32(255), f32(0.587) * f32(255), f32(0.114) * f32(255), f32(f32(0.299) * f32(10) + f32(0.587) * f32(20)) + f32(0.114) * f32(30)]
    assert got.dtype == np.float32 and np.array_equal(got, np.asarray(want, f32))


def _grey_field(xyz, a, c):
    """grey levels R = G = B = a . p + c, exact integers: I = (0.299f + 0.587f + 0.114f) * level up to float rounding"""
    lv = xyz.astype(np.float64) @ a + c
    assert np.array_equal(lv, np.rint(lv)) and lv.min() >= 0 and lv.max() <= 255
    return _pack(lv, lv, lv), lv


def test_linear_field_on_a_curved_patch():
    """I = a . p + c on a paraboloid cap: least squares is exact, x = a whatever the ball, so g = (1 - n n^T) a. The grid is dyadic
    (multiples of 1/64, z = (x^2 + y^2) / 2 a multiple of 2^-13) and a = (128, 64, 0) makes every level an integer; the grey formula
    returns k * level with k = the float sum of the three weights, within 3 ulp of the level."""
    g = np.arange(-6, 7, dtype=np.float64) / 64.0
    x, y = np.meshgrid(g, g, indexing="ij")
    xyz = np.stack([x.ravel(), y.ravel(), (x.ravel() ** 2 + y.ravel() ** 2) / 2.0], 1).astype(f32)
    assert np.array_equal(xyz.astype(np.float64)[:, 2], (x.ravel() ** 2 + y.ravel() ** 2) / 2.0)
    a = np.array([128.0, 64.0, 0.0])
    rgba, lv = _grey_field(xyz, a, 100.0)
    nrm = np.stack([-x.ravel(), -y.ravel(), np.ones(x.size)], 1)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    out = ref.gradients(xyz, nrm, rgba, 4.5 / 64.0)
    inten = ref.intensity(rgba).astype(np.float64)
    assert np.abs(inten - lv).max() <= 3 * 2.0 ** -24 * 255
    n64 = nrm.astype(np.float64)
    want = a[None, :] - n64 * (n64 @ a)[:, None]
    assert (out["count"] >= 3).all() and not out["undecided"].any()
    # the float intensities are off the integer levels by up to 3 ulp of 255 (4.6e-5), amplified by the solve: |dx| <= |dI| sqrt(n / lambda_min)
    assert np.abs(out["grad"] - want).max() <= 0.05 and np.abs(want).max() > 100.0
    assert np.abs(out["x"] - a).max() <= 0.05


def test_linear_field_on_a_planar_lattice_takes_the_rank_2_pseudo_inverse():
    """the same field on the exact plane z = 0.25: A has an exactly zero eigenvalue, the pseudo-inverse leaves the normal direction out,
    x = (a_x, a_y, 0) = (1 - n n^T) a although a_z = 32 (which only shifts every level by the same 8)"""
    g = np.arange(0, 12, dtype=np.float64) / 64.0
    x, y = np.meshgrid(g, g, indexing="ij")
    xyz = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.25)], 1).astype(f32)
    a = np.array([128.0, 64.0, 32.0])
    rgba, _lv = _grey_field(xyz, a, 20.0)
    nrm = np.tile(f32([0, 0, 1]), (len(xyz), 1))
    out = ref.gradients(xyz, nrm, rgba, 3.5 / 64.0)
    assert not out["undecided"].any() and np.nanmax(np.abs(out["ratio"])) < 1e-14
    assert np.abs(out["grad"] - np.array([128.0, 64.0, 0.0])).max() <= 0.05
    assert np.abs(out["x"][:, 2]).max() <= 1e-9


def test_fewer_than_three_points_and_nan_normals_give_nan():
    xyz = f32([[0, 0, 0], [0.01, 0, 0], [5, 5, 5], [5.01, 5, 5], [5, 5.01, 5]])
    nrm = np.tile(f32([0, 0, 1]), (5, 1)); nrm[4, 0] = np.nan
    out = ref.gradients(xyz, nrm, _pack([1, 2, 3, 4, 5], [0] * 5, [0] * 5), 0.1)
    assert out["count"].tolist() == [2, 2, 3, 3, 3]
    assert np.isnan(out["grad"][[0, 1, 4]]).all() and np.isfinite(out["grad"][[2, 3]]).all()
    rows = ref.rift(xyz, out["grad"].astype(f32), f32([[0, 0, 0], [5, 5, 5], [9, 9, 9]]), 0.1)
    assert rows["count"].tolist() == [2, 3, 0]
    assert np.isnan(rows["rows"]).all()                   # NaN gradients in the ball, twice; an empty ball


def test_uniform_colour_gives_zero_gradients_and_zero_rows():
    xyz, nrm, _rgba, kp, radius = scenes.scene(0)
    out = ref.gradients(xyz, nrm, np.full(len(xyz), 0x00a0b0c0, np.int32), radius)
    assert (out["count"] >= 3).all() and not np.abs(out["grad"]).any()
    rows = ref.rift(xyz, out["grad"].astype(f32), kp, radius)
    assert not rows["rows"].any() and (rows["count"] > 0).all()


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_one_ball_point_at_half_the_radius(sign):
    """p0 at the origin, one cloud point at u = (R / 2, 0, 0) with gradient (sign * 3, 0, 0), R = 0.5, 8 x 16 bins.
    d = 8 * 0.25 / (R + eps) = 4 (1 - eps / R) up to rounding: distance bins 3 (weight 4 eps / R = 9.5e-7) and 4 (the rest).
    Along u the angle is 0: a = 0, gradient bin 0 alone (bins -1 -> 15 and 1 carry weight 0). Against u the angle is pi (as float64;
    a = 16 pi / ((float)pi + eps) = 16 - 16 (eps + (float)pi - pi) / pi: bins 15 and 16 -> 0, the cyclic wrap, the latter with weight
    a - 15 = 1 - 16 * 2.07e-7 / pi. The row is the deposit pattern over its L2 norm; mag 3 cancels."""
    R = 0.5
    xyz = f32([[R / 2, 0, 0]]); grad = f32([[sign * 3.0, 0, 0]])
    out = ref.rift(xyz, grad, f32([[0, 0, 0]]), R)
    assert out["count"].tolist() == [1]
    row = out["rows"][0].reshape(16, 8)                    # [gradient bin, distance bin]
    d = 8.0 * 0.25 / float(f32(f32(R) + ref.FLT_EPS))
    wd = {3: 4.0 - d, 4: d - 3.0}
    g_bins = {0: 1.0}
    if sign < 0:
        a = 16.0 * np.pi / float(f32(f32(np.pi) + ref.FLT_EPS))
        g_bins = {15: 16.0 - a, 0: a - 15.0}
    want = np.zeros((16, 8))
    for gb, wg in g_bins.items():
        for db, w in wd.items():
            want[gb, db] += wg * w
    want /= np.sqrt((want * want).sum())
    assert np.abs(row - want).max() <= 1e-12 and (row > 0).sum() == len(g_bins) * 2
    assert abs(wd[3] - 4 * float(ref.FLT_EPS) / R) <= 1e-9
    if sign < 0:
        assert row[0, 4] > 0.999 and 0 < row[15, 4] < 5e-6   # nearly everything wrapped into gradient bin 0


def test_coincident_keypoint_and_zero_gradient_deposit_into_bin_zero():
    """u = 0: dist 0, angle 0 (PCL's NaN case) -> the whole magnitude into bin (0, 0); a zero gradient deposits nothing"""
    xyz = f32([[1, 1, 1], [1.1, 1, 1]]); grad = f32([[0, 2, 0], [0, 0, 0]])
    out = ref.rift(xyz, grad, f32([[1, 1, 1]]), 0.5)
    want = np.zeros(128); want[0] = 1.0
    assert out["count"].tolist() == [2] and np.array_equal(out["rows"][0], want)


# ------------------------------------------------------------------------------------------------ the scenes
@pytest.mark.parametrize("k", range(len(scenes.SCENES)))
def test_scene_caps_and_tolerances(k):
    xyz, _nrm, _rgba, kp, radius = scenes.scene(k)
    ga = scenes.gradient_answer(k)
    mag = np.linalg.norm(ga["grad"], axis=1)
    assert ga["undecided"].sum() == 0 <= scenes.MAX_UNDECIDED_POINTS * len(xyz)          # the restatement alone stays at zero of both
    assert not ga["near"].any() and np.isfinite(mag).all() and np.nanmin(ga["ratio"]) > 1e-3
    assert 250 < np.median(mag) < 320 and 450 < mag.max() < 500
    # the gradient tolerance, relative to the scene's typical gradient, stays far inside the descriptor tolerance
    tol = ref.grad_tol(ga["x"], radius, len(xyz))
    assert ref.grad_rel(len(xyz)) <= 2e-7 and tol.max() / np.median(mag) <= 1e-5 <= ref.ROW_TOL_MAX
    for bins in scenes.BINS:
        ra = scenes.row_answer(k, bins)
        assert ra["undecided"].sum() == 0 <= scenes.MAX_UNDECIDED_KEYPOINTS * len(kp)
        assert np.isfinite(ra["rows"]).all() and (ra["rows"] >= 0).all() and np.allclose((ra["rows"] ** 2).sum(1), 1.0, atol=1e-12)
        assert ra["amp"].max() <= ref.ROW_TOL_MAX and ra["tol"].max() <= ref.ROW_TOL_MAX   # derived, and below the project's 1e-4 uncapped
    assert 40 <= np.median((scenes.row_answer(k)["rows"] > 0).sum(1)) <= 70
    # all-float32 inputs to the same arithmetic stay far inside the derived row tolerance: the gradients rounded to float32 against float64
    full = ref.rift(xyz, ga["grad"].astype(f32), kp, radius)
    assert np.array_equal(full["rows"], scenes.row_answer(k)["rows"])


# ------------------------------------------------------------------------------------------------ host layer
def test_header_and_binding(pkg):
    h = open(os.path.join(hb.ROOT, "include", "ismhip.h")).read()
    assert re.search(r"int\s+ismhip_intensity_gradients\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, float radius, float\* grad_out, uint32_t\* count_out\);", h)
    assert re.search(r"int\s+ismhip_rift\(ismhip_ctx\* ctx, const ismhip_cloud\* cloud, const uint32_t\* kp_offsets_h,", h)
    for name, v in (("DISTANCE_BINS", 8), ("GRADIENT_BINS", 16), ("DIM", 128)):
        assert re.search(rf"#define ISMHIP_RIFT_{name}\s+{v}\b", h)
    assert "ismhip_rift" in pkg.capi.EXPORTS and "ismhip_intensity_gradients" in pkg.capi.EXPORTS and pkg.capi.RIFT_DIM == 128
    assert pkg.pipeline.IsmConfig(n_classes=3, feature="RIFT").dim == 128


def _rift_cfg(**params):
    p = {"ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT"}
    p.update(params)
    return _cfg(**{"Children/Features": {"Type": "RIFT", "Parameters": p}})


def test_host_configures_rift_and_round_trips():
    """on the parent commit the factory refuses the type"""
    m = hb.Model()
    m.config_from_json(_rift_cfg(Radius=0.25))
    out = json.loads(m.config_to_json())["Children"]["Features"]
    assert out["Type"] == "RIFT" and out["Parameters"]["Radius"] == pytest.approx(0.25)
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())                        # what we write, we read
    assert json.loads(m2.config_to_json())["Children"]["Features"] == out
    m.close(); m2.close()
    m = hb.Model()
    m.config_from_json(_rift_cfg())                                # Radius not given: the reference's default 0.1
    assert json.loads(m.config_to_json())["Children"]["Features"]["Parameters"]["Radius"] == pytest.approx(0.1)
    m.close()


def test_host_reads_the_example_config():
    src = json.load(open(os.path.join(hb.ROOT, "config", "kinect_rift.ism")))["ObjectConfig"]
    m = hb.Model()
    m.config_from_json(json.dumps(src))
    out = json.loads(m.config_to_json())
    assert out["Children"]["Features"]["Type"] == "RIFT" and out["Children"]["Features"]["Parameters"]["Radius"] == pytest.approx(0.05)
    assert out["Parameters"]["DistanceType"] == "ChiSquared"
    m.close()
    other = json.load(open(os.path.join(hb.ROOT, "config", "kinect_cshot.ism")))["ObjectConfig"]
    for j in (src, other):                                         # the value set of kinect_cshot.ism, the feature type apart
        del j["Children"]["Features"]["Type"]
    assert src == other


def test_host_refuses_a_colourless_cloud_and_names_rift_in_the_factory_message():
    rng = np.random.default_rng(9)
    xyz = rng.normal(size=(200, 3)).astype(f32)
    nrm = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(f32)
    m = hb.Model()
    m.config_from_json(_rift_cfg(Radius=0.3))
    m.add_training(xyz, nrm, 0, 0)
    with pytest.raises(hb.HostError, match="RIFT needs coloured point clouds"):
        m.train()
    with pytest.raises(hb.HostError, match="RIFT needs coloured point clouds"):
        m.detect_batch(np.uint32([0, 200]), xyz, nrm, max_maxima=4)
    m.close()
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: .*RIFT, SpinImage, RSD, CoSPAIR\)"):
        m.config_from_json(_cfg(**{"Children/Features/Type": "PFH"}))
    m.close()

"""PCA normals of lrf.hip (k_pca_normals, k_normals_from_lrf, k_sorted_normals) against the float64 reference of normals_ref.py
(-m gpu) on the scenes of prepath_scenes.py. test_prepath_cpu.py proves the reference and the scenes first.

The device takes the neighbourhood in float32 (the reference reproduces that decision bit for bit), accumulates FP64 moments about
the query point and solves with Jacobi; so every normal whose direction is determined (eigenvalue gap >= 1e-3) must lie within
ANGLE_TOL = 2e-7 rad of the reference: double arithmetic contributes < 1e-9 at that gap, rounding a unit vector to float32 at most
sqrt(3) * 2^-25 = 5.2e-8. One missed or extra neighbour moves a normal by ~1e-3, so this bound proves the neighbour set. No quantiles."""
import numpy as np
import pytest

import frontend_scenes as fs
import normals_ref as nr
import prepath_scenes as ps

pytestmark = pytest.mark.gpu
TOL = 1e-4
_device = {}


def T(a, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def make_cloud(pkg, ctx, dev, s):
    import torch
    t = [T(c, dev) for c in fs.cols(s["P"])]
    zn = [torch.zeros(len(s["P"]), dtype=torch.float32, device=dev) for _ in range(3)]
    return pkg.capi.Cloud(ctx, s["off"], *t, *zn, s["cell"])


def pca_on(pkg, ctx, dev, s, orientation, cloud=None):
    """estimate_normals_pca of a scene -> [N, 3] float32"""
    import torch
    own = cloud is None
    cloud = make_cloud(pkg, ctx, dev, s) if own else cloud
    out = [torch.empty(len(s["P"]), dtype=torch.float32, device=dev) for _ in range(3)]
    pkg.capi.estimate_normals_pca(ctx, cloud, s["radius"], orientation, *out)
    got = np.stack([a.cpu().numpy() for a in out], 1)
    if own:
        cloud.close()
    return got


def device_normals(pkg, gpu, name, orientation):
    """on the shared default context, once per (scene, orientation)"""
    if (name, orientation) not in _device:
        ctx, dev = gpu
        _device[name, orientation] = pca_on(pkg, ctx, dev, ps.normal_scene(name), orientation)
    return _device[name, orientation]


def check_pca(label, got, want, cos, u, sign_rule=None):
    """NaN pattern, unit length, sign outside the |cos| exemption, angle <= ANGLE_TOL wherever the gap determines the direction.
    sign_rule(got64) -> per point (viewpoint - q) . n / |viewpoint - q| signed so that >= 0 is the rule the kernel follows: it must
    hold for the device's own vector at EVERY finite normal, also where the reference's direction is undetermined."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, int(np.isnan(got).any(1).sum()), int(np.isnan(want).any(1).sum()))
    ok = u.valid
    g = got[ok].astype(np.float64)
    assert np.abs(np.linalg.norm(g, axis=1) - 1).max() <= 1e-6
    determined = u.gap[ok] >= nr.GAP_MIN
    decided = determined & (cos[ok] >= nr.COS_MIN)
    dots = (g * want[ok]).sum(1)
    ang = nr.angle(g, want[ok])
    worst = float(ang[determined].max()) if determined.any() else 0.0
    print(f"{label}: {ok.sum()} normals, largest angle {worst:.3g} rad, angle-exempt {int((~determined).sum())}, "
          f"sign-exempt {int((determined & ~decided).sum())}, sign mismatches {int((dots[decided] <= 0).sum())}")
    assert (dots[decided] > 0).all(), (label, np.nonzero(dots[decided] <= 0)[0][:10])
    assert worst <= nr.ANGLE_TOL, (label, worst, int((ang[determined] > nr.ANGLE_TOL).sum()))
    if sign_rule is not None:
        assert (sign_rule(got.astype(np.float64))[ok] >= -nr.COS_MIN).all(), label
    return worst


def flip_rule(s, orientation):
    """orientation 0: the normal faces the origin; 1: it points away from the object's float32 centroid"""
    P64 = s["P"].astype(np.float64)
    vp = np.zeros_like(P64)
    if orientation == 1:
        for o in range(len(s["off"]) - 1):
            vp[s["off"][o]:s["off"][o + 1]] = nr.centroid32(s["P"][s["off"][o]:s["off"][o + 1]])

    def rule(n):
        with np.errstate(invalid="ignore", divide="ignore"):
            v = vp - P64
            c = (v * n).sum(1) / np.linalg.norm(v, axis=1)
        return -c if orientation == 1 else c
    return rule


@pytest.mark.parametrize("orientation", [0, 1])
@pytest.mark.parametrize("name", list(ps.NORMAL_SCENES))
def test_pca_normals_match_the_float64_reference(pkg, gpu, name, orientation):
    """generic, far from the origin, exactly on the radius (there the bound is what proves the '<' decision), on an inexact radius,
    minimal neighbourhoods, balls of more than one row batch, a wide ragged batch.
    Largest angle measured on the MI355X (the same at both orientations), no point exempt from either check except the minimal
    scene's 11 coincident / collinear points: generic 4.43e-8, far 4.18e-8, exact_radius 4.06e-8, inexact_radius 3.22e-8,
    minimal 7.8e-9, row_batches 4.85e-8, wide 4.28e-8 rad."""
    s = ps.normal_scene(name)
    got = device_normals(pkg, gpu, name, orientation)
    want, cos = nr.orient(s["off"], s["P"], s["ref"], orientation)
    check_pca(f"{name}, orientation {orientation}", got, want, cos, s["ref"], flip_rule(s, orientation))
    if name == "exact_radius":
        for pr in s["probes"]:                                     # the probes themselves are held to the bound
            assert s["ref"].gap[pr["q"]] >= nr.GAP_MIN
    if name == "minimal":
        (i2, _), (i3, _), _, (i5, n5), (i6, n6) = s["groups"]
        assert np.isnan(got[i2:i2 + 2]).all()
        # the plane through the three float32 points as stored (the group's offset rounds them): their own cross product
        p3 = s["P"][i3:i3 + 3].astype(np.float64)
        plane = np.cross(p3[1] - p3[0], p3[2] - p3[0])
        assert nr.angle(got[i3:i3 + 3].astype(np.float64), plane[None, :]).max() <= nr.ANGLE_TOL
        coincident = got[i5:i5 + n5].astype(np.float64)
        assert np.isfinite(coincident).all() and np.abs(np.linalg.norm(coincident, axis=1) - 1).max() <= 1e-6
        p6 = s["P"][i6:i6 + n6].astype(np.float64)
        direction = (p6[-1] - p6[0]) / np.linalg.norm(p6[-1] - p6[0])
        assert np.abs(got[i6:i6 + n6].astype(np.float64) @ direction).max() <= 1e-6


@pytest.mark.parametrize("orientation", [0, 1])
def test_sorted_normal_copy_feeds_shot(pkg, gpu, ora, orientation):
    """estimate_normals_pca also writes the cloud's cell-sorted normal copy (sn4), which only the descriptors read: SHOT-352 on the
    same Cloud must match the oracle fed with the device's normals (exact counts, 1e-4). 64 keypoints on the two surfaces."""
    ctx, dev = gpu
    s = ps.normal_scene("generic")
    rng = np.random.default_rng(70)
    off, P = s["off"], s["P"]
    fin = np.isfinite(P).all(1)
    picks = [rng.choice(np.nonzero(fin[off[o]:off[o + 1]])[0], 32, replace=False) + int(off[o]) for o in (0, 1)]
    kp = np.concatenate([P[picks[0]], (P[picks[1]].astype(np.float64) * 0.99 + 0.01 * np.array([0.1, 0.2, 2.5])).astype(np.float32)])
    ko = np.array([0, 32, 64, 64], np.uint32)
    tk = [T(c, dev) for c in fs.cols(kp)]
    cloud = make_cloud(pkg, ctx, dev, s)
    try:
        nrm = pca_on(pkg, ctx, dev, s, orientation, cloud)
        lrf = pkg.capi.shot_lrf(ctx, cloud, ko, *tk, 0.3)
        desc, cnt = pkg.capi.shot352(ctx, cloud, ko, *tk, lrf, 0.3, want_counts=True)
        lrf, desc, cnt = lrf.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)
    finally:
        ctx.sync(); cloud.close()
    assert nrm.tobytes() == device_normals(pkg, gpu, "generic", orientation).tobytes()
    want, wcnt = ora.shot352(off, *fs.cols(P), *fs.cols(nrm), ko, *fs.cols(kp), lrf, 0.3)
    assert np.array_equal(cnt, wcnt) and wcnt.min() > 50
    assert np.array_equal(np.isnan(desc), np.isnan(want)) and np.isfinite(want).all()
    err = np.abs(desc - want).max()
    print(f"SHOT-352 on the sorted normal copy, orientation {orientation}: max error {err:.3g}")
    assert err <= TOL, err


def test_block_order_leaves_the_normals_alone(pkg, gpu, monkeypatch):
    """11 objects, one empty, one all NaN, the largest of 898 points (no multiple of 4): the XCD-local block map and the plain
    object-major order give the same bytes"""
    _, dev = gpu
    s = ps.normal_scene("wide")
    monkeypatch.setenv("ISMHIP_XCD_MAP", "0")
    ctx = pkg.capi.Ctx(0)                                          # the switch is read when a context is created
    try:
        plain = [pca_on(pkg, ctx, dev, s, orientation) for orientation in (0, 1)]
    finally:
        ctx.sync(); ctx.close()
    for orientation in (0, 1):
        base = device_normals(pkg, gpu, "wide", orientation)
        assert np.isfinite(base).any() and plain[orientation].tobytes() == base.tobytes()


# ------------------------------------------------------------------------------------------------ method 2
def test_normals_from_shot_frames_cross_a_chunk(pkg, gpu, ora):
    """estimate_normals (ConsistentNormalsMethod 2) with k = 366 invalid frames in object 0: the reference's mis-indexed patch loop
    gives the first k FINITE points of the object pcl::eigen33's unflipped vector; the run crosses waves and 256-thread chunks and,
    with three NaN points in front, rank != index. Object 1: k = 0. Object 2: k = n = 3. Expectation assembled here: frames from
    the oracle; rank < k -> raw_sign of the float64 reference normal; else a valid frame -> its inverted z axis (1e-4 for 99.9 %, the
    existing frame criterion); else the origin-flipped reference normal. PCA-derived entries: 2e-7 rad and exact sign.
    Measured on the MI355X: 369 first-k normals within 3.77e-8 rad (4 sign-exempt by the component margin), 319 kept fall-backs
    within 3.54e-8 rad. This test found k_pca_normals forming eigen33's sign from the matrix eigen_sym3 had already diagonalised
    in place: 5 of the first 366 points of object 0 came out negated (the 95 % of the older test hid them)."""
    ctx, dev = gpu
    s = ps.normal_scene("method2")
    off, P, u = s["off"], s["P"], s["ref"]
    zeros = [T(np.zeros(len(P), np.float32), dev) for _ in range(3)]
    cloud = make_cloud(pkg, ctx, dev, s)
    try:
        got = np.stack([a.cpu().numpy() for a in pkg.capi.estimate_normals(ctx, cloud, s["radius"], *zeros)], 1)
    finally:
        ctx.sync(); cloud.close()
    frames = ora.shot_lrf(off, *fs.cols(P), off, *fs.cols(P), s["radius"])
    fin = np.isfinite(P).all(1)
    bad = fin & ~np.isfinite(frames[:, 0])
    flipped, cos = nr.orient(off, P, u, 0)
    raw = nr.raw_sign(u.n)
    first_k = np.zeros(len(P), bool)
    k = []
    for o in range(3):
        a, b = int(off[o]), int(off[o + 1])
        k.append(int(bad[a:b].sum()))
        rank = np.cumsum(fin[a:b]) - 1
        first_k[a:b] = fin[a:b] & (rank < k[o])
    assert k[0] >= 300 and k[1] == 0 and k[2] == 3
    from_frame = fin & ~bad & ~first_k
    want = np.where(first_k[:, None], raw, np.where(from_frame[:, None], -frames[:, 6:9].astype(np.float64), flipped))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err = np.abs(got[from_frame] - want[from_frame]).max(1)
    assert (err < TOL).mean() > 0.999, int((err > TOL).sum())
    assert from_frame[off[1]:off[2]].all() and first_k[off[2]:off[3]].all()                       # k = 0 and k = n
    # PCA-derived: the unflipped first k (sign from the component margin) and the kept fall-backs (sign from the viewpoint)
    valid = ~np.isnan(want).any(1)
    g = got.astype(np.float64)
    for label, sel, clear in (("first k, eigen33 sign", first_k & valid, u.margin >= nr.MARGIN_MIN),
                              ("kept fall-backs, flipped to the origin", bad & ~first_k & valid, cos >= nr.COS_MIN)):
        determined = sel & (u.gap >= nr.GAP_MIN)
        ang = nr.angle(g[determined], want[determined])
        dots = (g * want).sum(1)[determined & clear]
        print(f"method 2, {label}: {int(sel.sum())} normals, largest angle {ang.max():.3g} rad, angle-exempt {int((sel & ~determined).sum())}, "
              f"sign-exempt {int((determined & ~clear).sum())}, sign mismatches {int((dots <= 0).sum())}")
        assert sel.sum() >= 3 and ang.max() <= nr.ANGLE_TOL and (dots > 0).all()
    assert (bad & ~first_k & valid)[:off[1]].sum() >= 200                                        # groups behind the first k keep the flipped normal

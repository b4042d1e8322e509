"""RIFT on the MI355X (ismhip_intensity_gradients, ismhip_rift) against the restatement tests/rift_ref.py.

Gradients: within ref.grad_tol (derived in rift_ref.py from the quantum of the integer sums and the float store) on every decided point,
neighbour counts and the NaN pattern exact. Rows: the restatement reads the DEVICE's gradients (as test_gpu_global.py feeds the device's
frame to its restatement), so a row is held to the per-bin bound that rift_ref.py derives from float rounding and the fixed-point scale,
never above 1e-4; counts and the NaN pattern exact. One leg runs the restatement end to end on its own gradients, with the gradient
tolerance carried into the row bound. At most 1 % of a scene's points and 5 % of its keypoints may be undecided.

Figures printed by these tests on an MI355X when they were written: see DESIGN.md section 4.19."""
import numpy as np
import pytest

import iss3d_scenes
import rift_ref as ref
import rift_scenes as scenes

pytestmark = pytest.mark.gpu
f32 = np.float32


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


class Batch:
    """objs: list of (xyz [n, 3], normals [n, 3], rgba [n] or None), kps: list of float32 [k, 3] -> a Cloud and the keypoint arrays"""

    def __init__(self, pkg, ctx, dev, objs, kps, cell, color=True):
        self.objs, self.kps = objs, kps
        self.pt_off = np.concatenate([[0], np.cumsum([len(o[0]) for o in objs])]).astype(np.uint32)
        self.kp_off = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.uint32)
        cat = lambda parts, width, dt: np.concatenate([np.asarray(p, dt).reshape(-1, width) for p in parts]) if parts else np.zeros((0, width), dt)
        xyz, nrm, kp = cat([o[0] for o in objs], 3, f32), cat([o[1] for o in objs], 3, f32), cat(kps, 3, f32)
        col = lambda a, i: _dev(a[:, i] if len(a) else np.zeros(1, f32), dev)      # an empty batch still hands over valid pointers
        self.t = [col(xyz, i) for i in range(3)] + [col(nrm, i) for i in range(3)]
        self.tk = [col(kp, i) for i in range(3)]
        rgba = np.concatenate([np.asarray(o[2], np.int32) for o in objs] + [np.zeros(0, np.int32)])
        self.rgba = _dev(rgba if len(rgba) else np.zeros(1, np.int32), dev) if color else None
        self.cloud = pkg.capi.Cloud(ctx, self.pt_off, *self.t, cell, rgba=self.rgba)

    def run(self, pkg, ctx, radius, bins=scenes.BINS[0], grad=None):
        """-> (gradients [n, 3], point counts [n], rows [k, D], keypoint counts [k]) as numpy"""
        g, gc = pkg.capi.intensity_gradients(ctx, self.cloud, radius, want_counts=True)
        rows, rc = pkg.capi.rift(ctx, self.cloud, self.kp_off, *self.tk, radius, g if grad is None else grad, bins[0], bins[1], want_counts=True)
        ctx.sync()
        return g.cpu().numpy(), gc.cpu().numpy(), rows.cpu().numpy(), rc.cpu().numpy()

    def close(self):
        self.cloud.close()


def _check_gradients(got, cnt, want, radius, tag):
    """device gradients of one object against the restatement; returns (undecided points, largest error over its tolerance, largest error)"""
    dec = ~want["undecided"]
    assert np.array_equal(cnt, want["count"]), tag
    assert np.array_equal(np.isnan(got), np.isnan(want["grad"])), tag
    ok = dec & np.isfinite(want["grad"]).all(1)
    if not ok.any():
        return int((~dec).sum()), 0.0, 0.0
    err = np.abs(got[ok].astype(np.float64) - want["grad"][ok]).max(1)
    tol = ref.grad_tol(want["x"][ok], radius, len(got))
    print("%s: %d points, %d undecided, largest gradient error %.3g (%.3g of its tolerance, %.3g of |x|)"
          % (tag, len(got), (~dec).sum(), err.max(), (err / tol).max(), (err / np.maximum(np.linalg.norm(want["x"][ok], axis=1), 1e-30)).max()))
    assert (err <= tol).all(), tag
    return int((~dec).sum()), float((err / tol).max()), float(err.max())


def _check_rows(rows, cnt, want, tag):
    dec = ~want["undecided"]
    assert np.array_equal(cnt, want["count"]), tag
    assert np.array_equal(np.isnan(rows), np.isnan(want["rows"])), tag
    ok = dec & np.isfinite(want["rows"]).all(1)
    if not ok.any():
        return int((~dec).sum()), 0.0
    err = np.abs(rows[ok].astype(np.float64) - want["rows"][ok])
    print("%s: %d keypoints, %d undecided, largest row error %.3g (%.3g of its tolerance; largest tolerance %.3g)"
          % (tag, len(rows), (~dec).sum(), err.max(), (err / np.maximum(want["tol"][ok], 1e-300)).max(), want["tol"][ok].max()))
    assert (err <= want["tol"][ok]).all() and want["tol"].max() <= ref.ROW_TOL_MAX, tag
    return int((~dec).sum()), float(err.max())


@pytest.fixture(scope="module")
def scene_runs(pkg, gpu):
    """both scenes at both bin shapes, run once: {(k, bins): (gradients, point counts, rows, keypoint counts)}"""
    ctx, dev = gpu
    out = {}
    for k in range(len(scenes.SCENES)):
        xyz, nrm, rgba, kp, radius = scenes.scene(k)
        b = Batch(pkg, ctx, dev, [(xyz, nrm, rgba)], [kp], 0.4 * radius)
        for bins in scenes.BINS:
            out[(k, bins)] = b.run(pkg, ctx, radius, bins)
        b.close()
    return out


@pytest.mark.parametrize("k", range(len(scenes.SCENES)))
def test_gradients_match_restatement(scene_runs, k):
    xyz, _nrm, _rgba, _kp, radius = scenes.scene(k)
    g, gc, _rows, _rc = scene_runs[(k, scenes.BINS[0])]
    n_und, _rel, _err = _check_gradients(g, gc, scenes.gradient_answer(k), radius, "scene %d" % k)
    assert n_und <= scenes.MAX_UNDECIDED_POINTS * len(xyz)
    assert np.isfinite(g).all() and np.median(np.linalg.norm(g, axis=1)) > 100.0          # a gradient field, not an empty answer


@pytest.mark.parametrize("bins", scenes.BINS)
@pytest.mark.parametrize("k", range(len(scenes.SCENES)))
def test_rows_match_restatement_on_the_device_gradients(scene_runs, k, bins):
    xyz, _nrm, _rgba, kp, radius = scenes.scene(k)
    g, _gc, rows, rc = scene_runs[(k, bins)]
    want = ref.rift(xyz, g, kp, radius, bins[0], bins[1], undecided_points=scenes.gradient_answer(k)["undecided"])
    n_und, _err = _check_rows(rows, rc, want, "scene %d, %d x %d bins" % (k, bins[0], bins[1]))
    assert n_und <= scenes.MAX_UNDECIDED_KEYPOINTS * len(kp)
    assert rows.shape == (len(kp), bins[0] * bins[1]) and np.allclose((rows.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-6)


@pytest.mark.parametrize("k", range(len(scenes.SCENES)))
def test_end_to_end_against_the_restatements_own_gradients(scene_runs, k):
    """the restatement's rows from ITS gradients against the device's rows from the device's: the row bound then carries, per ball
    point, the gradient tolerance and the float rounding of the stored gradient"""
    xyz, _nrm, _rgba, kp, radius = scenes.scene(k)
    ga = scenes.gradient_answer(k)
    gerr = ref.grad_tol(ga["x"], radius, len(xyz)) + 2.0 ** -24 * np.abs(ga["grad"]).max(1)
    want = ref.rift(xyz, ga["grad"].astype(f32), kp, radius, undecided_points=ga["undecided"], gerr=gerr)
    _g, _gc, rows, rc = scene_runs[(k, scenes.BINS[0])]
    n_und, _err = _check_rows(rows, rc, want, "scene %d end to end" % k)
    assert n_und <= scenes.MAX_UNDECIDED_KEYPOINTS * len(kp)
    assert np.array_equal(want["rows"], scenes.row_answer(k)["rows"])


def _object(xyz, radius):
    xyz = np.asarray(xyz, f32)
    return xyz, scenes.pca_normals(xyz, radius) if len(xyz) else np.zeros((0, 3), f32), scenes.texture(xyz)


FAR = f32([[10.0, 10.0, 10.0]])


def test_small_and_empty_objects_in_one_batch(pkg, gpu):
    """objects of 0, 1, 2, 3, 63, 64, 65 and 257 points, then [700, 0, 700]: an empty object between two full ones. Every object but one
    gets its first point as a keypoint (u = 0) and a keypoint far away (an empty ball, a NaN row); the 63-point object gets none."""
    ctx, dev = gpu
    p = iss3d_scenes.scene(2)
    radius = 0.3                                                           # sparse cuts: wide balls
    cuts = [p[:0], p[:1], p[:2], p[10:13], p[100:163], p[200:264], p[300:365], p[400:657], p, p[:0], p[::-1].copy()]
    objs = [_object(c, radius) for c in cuts]
    kps = [np.concatenate([c[:1], FAR, c[5:40:7]]) for c in cuts]
    kps[4] = np.zeros((0, 3), f32)
    b = Batch(pkg, ctx, dev, objs, kps, 0.1)
    g, gc, rows, rc = b.run(pkg, ctx, radius)
    b.close()
    for o, (xyz, nrm, rgba) in enumerate(objs):
        pb, pe, kb, ke = int(b.pt_off[o]), int(b.pt_off[o + 1]), int(b.kp_off[o]), int(b.kp_off[o + 1])
        ga = ref.gradients(xyz, nrm, rgba, radius)
        _check_gradients(g[pb:pe], gc[pb:pe], ga, radius, "object %d" % o)
        want = ref.rift(xyz, g[pb:pe], kps[o], radius, undecided_points=ga["undecided"])
        _check_rows(rows[kb:ke], rc[kb:ke], want, "object %d" % o)
        if len(xyz) in (1, 2):
            assert np.isnan(g[pb:pe]).all() and np.isnan(rows[kb:ke]).all()               # cp < 3: NaN gradients, NaN rows
        if len(kps[o]):
            far = kb + min(len(xyz), 1)
            assert np.isnan(rows[far]).all() and rc[far] == 0                             # the far keypoint: an empty ball
        if len(xyz) >= 63 and len(kps[o]):
            assert np.isfinite(rows[kb]).all() and rc[kb] >= 3                            # the coincident keypoint


def test_lattice_counts_are_exact_in_both_passes(pkg, gpu):
    ctx, dev = gpu
    xyz = iss3d_scenes.lattice()
    nrm = np.tile(f32([0, 0, 1]), (len(xyz), 1))
    b = Batch(pkg, ctx, dev, [(xyz, nrm, scenes.texture(xyz))], [xyz], 1.0 / 64.0)
    _g, gc, _rows, rc = b.run(pkg, ctx, iss3d_scenes.LATTICE_RADIUS)
    b.close()
    assert np.array_equal(gc, iss3d_scenes.lattice_counts()) and np.array_equal(rc, iss3d_scenes.lattice_counts())


def test_non_finite_points_and_nan_normals(pkg, gpu):
    """points that are not finite are neither queries nor neighbours; a point with a NaN normal has a NaN gradient and every row whose
    ball touches it is NaN"""
    ctx, dev = gpu
    xyz0, nrm0, rgba, kp, radius = scenes.scene(0)
    xyz, nrm = xyz0.copy(), nrm0.copy()
    bad = np.arange(3, len(xyz), 9)
    xyz[bad[0::3], 0] = np.nan; xyz[bad[1::3], 1] = np.inf; xyz[bad[2::3]] = -np.inf
    nan_n = np.array([100, 350])
    nrm[nan_n, 1] = np.nan
    assert not np.isin(nan_n, bad).any()
    b = Batch(pkg, ctx, dev, [(xyz, nrm, rgba)], [kp], 0.05)
    g, gc, rows, rc = b.run(pkg, ctx, radius)
    b.close()
    ga = ref.gradients(xyz, nrm, rgba, radius)
    assert _check_gradients(g, gc, ga, radius, "NaN points")[0] <= 7
    assert np.isnan(g[bad]).all() and not gc[bad].any() and np.isnan(g[nan_n]).all() and (gc[nan_n] >= 3).all()
    want = ref.rift(xyz, g, kp, radius, undecided_points=ga["undecided"])
    _check_rows(rows, rc, want, "NaN points")
    touched = np.isnan(want["rows"]).all(1)
    assert 0 < touched.sum() < len(kp) and np.array_equal(np.isnan(rows).all(1), touched)


def test_radius_larger_than_the_object(pkg, gpu):
    """every point is in every ball: 700 candidates per wave, more than one block of the candidate sweep"""
    ctx, dev = gpu
    xyz, nrm, rgba, kp, _radius = scenes.scene(0)
    b = Batch(pkg, ctx, dev, [(xyz, nrm, rgba)], [kp], 0.05)
    g, gc, rows, rc = b.run(pkg, ctx, 2.0)
    b.close()
    assert (gc == len(xyz)).all() and (rc == len(xyz)).all()
    ga = ref.gradients(xyz, nrm, rgba, 2.0)
    _check_gradients(g, gc, ga, 2.0, "radius 2")
    assert not ga["undecided"].all()
    _check_rows(rows, rc, ref.rift(xyz, g, kp, 2.0, undecided_points=ga["undecided"]), "radius 2")


def test_results_do_not_depend_on_the_cell_size_or_the_run(pkg, gpu):
    ctx, dev = gpu
    xyz, nrm, rgba, kp, radius = scenes.scene(1)
    runs = []
    for cell in (0.25 * radius, 0.25 * radius, 4.0 * radius):             # the same call twice, then a cloud with cells of four radii
        b = Batch(pkg, ctx, dev, [(xyz, nrm, rgba)], [kp], cell)
        runs.append(b.run(pkg, ctx, radius))
        b.close()
    for other in runs[1:]:
        for a, c in zip(runs[0], other):
            assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    assert np.isfinite(runs[0][2]).all()


def test_refusals(pkg, gpu):
    ctx, dev = gpu
    xyz, nrm, rgba, kp, radius = scenes.scene(0)
    capi = pkg.capi
    b = Batch(pkg, ctx, dev, [(xyz, nrm, rgba)], [kp], 0.05)
    grad = capi.intensity_gradients(ctx, b.cloud, radius)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(capi.IsmHipError, match=r"\(-1\).*intensity_gradients: bad argument"):
            capi.intensity_gradients(ctx, b.cloud, r)
        with pytest.raises(capi.IsmHipError, match=r"\(-1\).*rift: bad argument"):
            capi.rift(ctx, b.cloud, b.kp_off, *b.tk, r, grad)
    for nd, ng in ((0, 16), (8, 0), (-1, 16)):
        with pytest.raises(capi.IsmHipError, match=r"\(-1\).*rift: bad argument"):
            capi.rift(ctx, b.cloud, b.kp_off, *b.tk, radius, grad, nd, ng)
    with pytest.raises(capi.IsmHipError, match=r"\(-4\).*more than 256 bins"):
        capi.rift(ctx, b.cloud, b.kp_off, *b.tk, radius, grad, 17, 16)
    assert capi.rift(ctx, b.cloud, b.kp_off, *b.tk, radius, grad, 16, 16).shape == (len(kp), 256)      # exactly 256 is built
    with pytest.raises(capi.IsmHipError, match=r"\(-1\).*rift: .*NULL"):
        capi.rift(ctx, b.cloud, b.kp_off, *b.tk, radius, None)
    bad_off = b.kp_off[::-1].copy()
    with pytest.raises(capi.IsmHipError, match=r"\(-1\).*rift: offsets not monotone"):
        capi.rift(ctx, b.cloud, bad_off, *b.tk, radius, grad)
    plain = Batch(pkg, ctx, dev, [(xyz, nrm, rgba)], [kp], 0.05, color=False)
    with pytest.raises(capi.IsmHipError, match=r"\(-1\).*intensity_gradients: colour arrays missing"):
        capi.intensity_gradients(ctx, plain.cloud, radius)
    with pytest.raises(capi.IsmHipError, match=r"\(-1\).*rift: colour arrays missing"):
        capi.rift(ctx, plain.cloud, b.kp_off, *b.tk, radius, grad)
    plain.close(); b.close()


def test_timers_report_one_launch_each(pkg, gpu):
    ctx, dev = gpu
    xyz, nrm, rgba, kp, radius = scenes.scene(0)
    b = Batch(pkg, ctx, dev, [(xyz, nrm, rgba)], [kp], 0.05)
    ctx.timers_enable(True); ctx.timers_reset()
    b.run(pkg, ctx, radius)
    for key in ("intensity_gradients", "rift"):
        ms, launches = ctx.timer(key)
        assert launches == 1 and ms > 0.0
    ctx.timers_enable(False)
    b.close()

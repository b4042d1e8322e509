"""SHOT-352, CSHOT-1344 and SHOT_GLOBAL of the device (-m gpu) against the float64 restatement shot_ref.py on the scenes of
shot_ref_scenes.py, each bin of each row within the bound shot_ref derives for it from the kernels' arithmetic (v_sqrt_f32, v_rcp_f32,
shot_acos on a float zl * rcp(dist), shot_atan2, the float weights, the CIELab bound on the colour offset, 2^-29 per fixed-point
deposit, the final divide) -- no global tolerance. The existing 1e-4 comparisons with the float oracle stay where they are
(test_gpu_parity.py, test_gpu_frontend.py); this gate is 10 to 200 times tighter and sees, for example, PST_RAD_45f off by 1e-4
relative, which moves rows by a few 1e-5 and passes every 1e-4 comparison.

Per scene: equal counts and NaN patterns; |device - reference| <= bound on every finite SHOT-352 row and every colour-decided
CSHOT-1344 row (at most 10 % of the finite keypoints may be colour-undecided; their shape half, renormalised, is still compared);
the sector-sum identity between the two channels on every finite CSHOT row (shot_ref_scenes.sector_sum_bound). Frames: the device's
own estimate unless the scene supplies them.

Measured on the MI355X, largest |error| / bound . largest error . largest bound (every test prints its own, -s):
    sphere          SHOT 0.21 . 4.2e-7 . 2.8e-6    CSHOT 0.32 . 3.7e-7 . 4.5e-6    (21 of 21 finite keypoints colour-decided)
    pole_and_seams  SHOT 0.36 . 1.7e-6 . 1.1e-5    CSHOT 0.36 . 1.2e-6 . 1.1e-5
    palette_white   SHOT 0.22 . 1.5e-8 . 4.4e-7    CSHOT 0.21 . 3.0e-8 . 3.5e-6
    palette_black   SHOT 0.22 . 1.5e-8 . 4.4e-7    CSHOT 0.19 . 3.7e-8 . 2.4e-6
    palette_uniform SHOT 0.22 . 1.5e-8 . 4.4e-7    CSHOT 0.21 . 1.5e-8 . 6.7e-7
    dense           SHOT 0.08 . 7.5e-9 . 2.9e-7    CSHOT 0.02 . 4.1e-8 . 4.0e-6
    SHOT_GLOBAL     0.28 . 1.5e-8 . 4.4e-7
    sector sums     largest difference 4e-8 (bound there 2.4e-7)
One run with PST_RAD_45f off by 1e-4 relative: test_shot352_matches_oracle and test_cshot1344_matches_oracle (1e-4) pass, the sphere
case fails: largest row error 9.95e-5 against the float64 reference, 289 times the bound of its bin."""
import numpy as np
import pytest

import shot_ref
import shot_ref_scenes as srs
import test_gpu_frontend as gf

pytestmark = pytest.mark.gpu
U = shot_ref.U
_runs = {}


def run(pkg, gpu, name):
    """device rows of a scene on the shared context and the reference on the same frames, computed once"""
    if name in _runs:
        return _runs[name]
    ctx, dev = gpu
    s = srs.scene(name)
    b = gf.Batch(pkg, ctx, dev, [(s.points, s.normals)], [s.keypoints], s.cell, [s.rgba], [s.kp_rgba])
    try:
        est = None if s.frames is not None else pkg.capi.shot_lrf(ctx, b.cloud, b.kp_off, *b.tk, s.radius).cpu().numpy()
        fr = srs.with_fixed_frames(s, est)
        t_fr = gf.T(fr, dev)
        shot, cnt = pkg.capi.shot352(ctx, b.cloud, b.kp_off, *b.tk, t_fr, s.radius, want_counts=True)
        cshot, ccnt = pkg.capi.cshot1344(ctx, b.cloud, b.kp_off, *b.tk, b.t_kp_rgba, t_fr, s.radius, want_counts=True)
        out = dict(scene=s, frames=fr, shot=shot.cpu().numpy(), cnt=cnt.cpu().numpy(), cshot=cshot.cpu().numpy(), ccnt=ccnt.cpu().numpy())
        ctx.sync()
    finally:
        b.close()
    out["ref"] = srs.reference(s, fr)
    _runs[name] = out
    return out


def check(name, got, want, bound):
    """|got - want| <= bound per bin -> the largest ratio; prints the figures the docstrings quote"""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):             # a bin nothing can reach has bound 0 and must hold exactly 0
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s: largest |error| / bound %.3f (error %.3g, bound %.3g, bin %s); largest error %.3g; bound: largest %.3g, median of the rows' largest %.3g"
          % (name, ratio[i], err[i], bound[i], i, err.max(), bound.max(), np.median(bound.max(-1))))
    assert (err <= bound).all(), (name, i, float(err[i]), float(bound[i]))
    return float(ratio[i])


@pytest.mark.parametrize("name", list(srs.BUILDERS))
def test_device_rows_lie_within_the_derived_bound(pkg, gpu, name):
    r = run(pkg, gpu, name)
    ref = r["ref"]
    want_cnt = np.array([x.count for x in ref])
    assert np.array_equal(r["cnt"], want_cnt) and np.array_equal(r["ccnt"], want_cnt)
    want_s, want_c = np.array([x.shape for x in ref]), np.array([x.desc for x in ref])
    assert np.array_equal(np.isnan(r["shot"]), np.isnan(want_s)) and np.array_equal(np.isnan(r["cshot"]), np.isnan(want_c))
    fin = ~np.isnan(want_c[:, 0])
    assert fin.any()
    check(name + " SHOT-352", r["shot"][fin], want_s[fin], np.array([x.shape_bound for x in ref])[fin])
    dec = fin & np.array([x.decided for x in ref])
    print("%s: %d of %d finite keypoints colour-decided" % (name, dec.sum(), fin.sum()))
    assert (fin & ~dec).sum() <= 0.1 * fin.sum()
    check(name + " CSHOT-1344", r["cshot"][dec], want_c[dec], np.array([x.bound for x in ref])[dec])
    und = fin & ~dec
    if und.any():                                                    # the shape half of an undecided row, rescaled: two more roundings per value
        half = r["cshot"][und][:, :352].astype(np.float64)
        half /= np.sqrt((half * half).sum(1, keepdims=True))
        check(name + " CSHOT-1344 shape half of undecided rows", half, want_s[und], np.array([x.shape_bound for x in ref])[und] + 4 * U * np.abs(half))
    a, c = srs.sector_sums(r["cshot"][fin])
    diff, sb = np.abs(a - c), srs.sector_sum_bound(a, c)
    print("%s: largest sector-sum difference %.3g (bound there %.3g) at sector sums up to %.3g" % (name, diff.max(), sb.flat[np.argmax(diff)], a.max()))
    assert (diff <= sb).all()
    if name == "palette_uniform":                                    # cd = 0: every colour bin but step 0 receives exactly 0
        assert (r["cshot"][0, 352:].reshape(32, 31)[:, 1:] == 0).all()
    if name == "sphere":
        assert want_cnt[srs.SPHERE_FOUR] == 4 and not fin[[srs.SPHERE_FAR, srs.SPHERE_NAN, srs.SPHERE_FOUR]].any() and fin[:21].all()
    if name == "dense":
        assert want_cnt[0] == srs.DENSE_POINTS


def test_shot_global_row_lies_within_the_derived_bound(pkg, gpu):
    """SHOT_GLOBAL shares the per-neighbour code (shot_neighbour): one whole-object region of the sphere, held to shot352 at the device's
    own centroid, radius and frame"""
    ctx, dev = gpu
    s = srs.scene("sphere")
    b = gf.Batch(pkg, ctx, dev, [(s.points, s.normals)], [s.keypoints], s.cell)
    try:
        out = {k: v.cpu().numpy() for k, v in pkg.capi.global_shot352(ctx, b.cloud, dev, [0]).items()}
        ctx.sync()
    finally:
        b.close()
    assert out["n_sel"][0] == len(s.points) and np.isfinite(out["lrf"]).all() and np.isfinite(out["desc"]).all()
    want, cnt, bound = shot_ref.shot352(s.points, s.normals, out["centroid"][0], out["lrf"][0], out["radius"][0])
    assert cnt >= len(s.points) - 1                                  # the farthest point defines the radius and may lie ON it
    check("SHOT_GLOBAL sphere", out["desc"], want[None], bound[None])

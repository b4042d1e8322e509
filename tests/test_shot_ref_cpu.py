"""Runs without a GPU: the float CPU oracle's SHOT-352 and CSHOT-1344 against the float64 restatement shot_ref.py on the scenes of
shot_ref_scenes.py (the scenes test_gpu_shot_ref.py holds the device to), and the properties those scenes are built for.

The oracle accumulates its bins in float like the reference, the restatement in float64: they agree to 2.5e-7 at worst (dense scene,
20 000 neighbours; 9e-8 on the sphere). The gate is 1e-6 -- the spread between two readings of the specification, not the device's
arithmetic, so the number may be fixed. Frames: the oracle's (the GPU test takes the device's)."""
import numpy as np
import pytest

import frontend_scenes as fs
import lab_ref
import shot_ref
import shot_ref_scenes as srs

TOL = 1e-6
_runs = {}


def run(ora, name):
    """(scene, frames, oracle SHOT rows, oracle CSHOT rows, oracle counts, reference rows) of a scene, computed once"""
    if name not in _runs:
        s = srs.scene(name)
        po, ko = np.array([0, len(s.points)], np.uint32), np.array([0, len(s.keypoints)], np.uint32)
        est = ora.shot_lrf(po, *fs.cols(s.points), ko, *fs.cols(s.keypoints), s.radius)
        fr = srs.with_fixed_frames(s, est)
        shot, cnt = ora.shot352(po, *fs.cols(s.points), *fs.cols(s.normals), ko, *fs.cols(s.keypoints), fr, s.radius)
        cshot, ccnt = ora.cshot1344(po, *fs.cols(s.points), *fs.cols(s.normals), s.rgba, ko, *fs.cols(s.keypoints), s.kp_rgba, fr, s.radius)
        assert np.array_equal(cnt, ccnt)
        _runs[name] = (s, fr, shot, cshot, cnt, srs.reference(s, fr))
    return _runs[name]


@pytest.mark.parametrize("name", list(srs.BUILDERS))
def test_oracle_matches_the_restatement(ora, name):
    s, fr, shot, cshot, cnt, ref = run(ora, name)
    assert [r.count for r in ref] == cnt.tolist()
    want_c, want_s = np.array([r.desc for r in ref]), np.array([r.shape for r in ref])
    assert np.array_equal(np.isnan(cshot), np.isnan(want_c)) and np.array_equal(np.isnan(shot), np.isnan(want_s))
    fin = ~np.isnan(want_c[:, 0])
    assert fin.any()
    e_s, e_c = float(np.abs(shot[fin] - want_s[fin]).max()), float(np.abs(cshot[fin] - want_c[fin]).max())
    decided = np.array([r.decided for r in ref])[fin]
    print("%s: oracle vs restatement SHOT %.3g CSHOT %.3g; colour-decided %d of %d finite keypoints; largest bound SHOT %.3g CSHOT %.3g"
          % (name, e_s, e_c, decided.sum(), fin.sum(), max(r.shape_bound.max() for r, f in zip(ref, fin) if f), max(r.bound.max() for r, f in zip(ref, fin) if f)))
    assert e_s <= TOL and e_c <= TOL
    assert (~decided).sum() <= 0.1 * fin.sum()                                  # the cap the GPU test relies on
    # shot352 on its own is the shape half of the CSHOT reference
    k = int(np.nonzero(fin)[0][0])
    d, c, b = shot_ref.shot352(s.points, s.normals, s.keypoints[k], fr[k], s.radius)
    assert c == ref[k].count and np.array_equal(d, ref[k].shape) and np.array_equal(b, ref[k].shape_bound)


@pytest.mark.parametrize("name", list(srs.BUILDERS))
def test_sector_sums_of_the_oracle_agree_between_the_channels(ora, name):
    """both channels of a sector receive 1 + winc per home neighbour and the same side deposits"""
    s, fr, shot, cshot, cnt, ref = run(ora, name)
    fin = ~np.isnan(cshot[:, 0])
    a, b = srs.sector_sums(cshot[fin])
    bound = srs.oracle_sector_sum_bound(a, b, cnt[fin])
    print("%s: largest sector-sum difference %.3g at sector sums up to %.3g" % (name, np.abs(a - b).max(), a.max()))
    assert (np.abs(a - b) <= bound).all()
    ra, rb = srs.sector_sums(np.array([r.desc for r in ref])[fin].astype(np.float64))
    assert np.abs(ra - rb).max() <= 42 * 2 * shot_ref.U                          # the restatement: float64 sums, 42 float32 casts of values <= 1


def test_sphere_keypoints_are_what_they_are_named(ora):
    s, fr, shot, cshot, cnt, ref = run(ora, "sphere")
    assert len(s.points) == 3000 and len(s.keypoints) == 24 and lab_ref.convert(s.rgba).decided.all() and lab_ref.convert(s.kp_rgba).decided.all()
    assert cnt[srs.SPHERE_FOUR] == 4 and np.isnan(cshot[srs.SPHERE_FOUR]).all() and np.isfinite(fr[srs.SPHERE_FOUR]).all()
    assert cnt[srs.SPHERE_FAR] == 0 and cnt[srs.SPHERE_NAN] == 0 and np.isnan(cshot[[srs.SPHERE_FAR, srs.SPHERE_NAN]]).all()
    assert (s.keypoints[srs.SPHERE_ON_POINT] == s.points[7]).all() and np.isfinite(cshot[:21]).all() and cnt[:21].min() >= 30


def test_pole_and_seam_neighbours_sit_beside_the_hard_decisions(ora):
    s = srs.scene("pole_and_seams")
    p = s.points.astype(np.float64)
    d = np.linalg.norm(p, axis=1)
    inc = np.arccos(p[:, 2] / d)
    pole, equator, seam = slice(0, 200), slice(200, 400), slice(400, 600)
    off = np.minimum(inc[pole], np.pi - inc[pole])
    assert 0.9e-4 < off.min() and off.max() < 1.1e-2 and (inc[pole] < 1).sum() == 100
    assert 0.9e-4 < np.abs(inc[equator] - np.pi / 2).min() and np.abs(inc[equator] - np.pi / 2).max() < 1.1e-2
    x, y = s.points[seam, 0], s.points[seam, 1]                                 # the float32 values the kernel decides on
    assert (x != 0).all() and (y != 0).all() and (np.abs(x) != np.abs(y)).all()
    az = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    to_seam = np.abs(az / (np.pi / 4) - np.rint(az / (np.pi / 4))) * (np.pi / 4)
    assert 1e-7 < to_seam.min() and to_seam.max() < 1.2e-6 and len(set(np.rint(az / (np.pi / 4)).astype(int) % 8)) == 8
    r = s.radius
    for part in (pole, equator, seam):                                           # every radial case in every group
        assert all(m.sum() >= 30 for m in (d[part] < r / 4, (d[part] > r / 4) & (d[part] < r / 2), (d[part] > r / 2) & (d[part] < 3 * r / 4),
                                           (d[part] > 3 * r / 4) & (d[part] < r)))
    assert d.max() < r


@pytest.mark.parametrize("name,colour", [("palette_white", srs.WHITE), ("palette_black", srs.BLACK)])
def test_palette_hits_every_colour_step(name, colour):
    s = srs.scene(name)
    step, dec = srs.colour_steps(colour, s.rgba)
    top = srs.palette_max_step(colour)
    print("%s: colour steps 0..%d" % (name, top))
    assert dec.all() and sorted(set(step.tolist())) == list(range(top + 1)) and top >= 15
    assert np.bincount(step, minlength=top + 1).min() >= 4 and int(s.kp_rgba[0]) == colour


def test_uniform_palette_puts_all_colour_weight_into_step_0(ora):
    s, fr, shot, cshot, cnt, ref = run(ora, "palette_uniform")
    assert (s.rgba == s.kp_rgba[0]).all()
    for row in (cshot[0], ref[0].desc):
        col = row[352:].reshape(32, 31)
        assert (col[:, 1:] == 0).all() and (col[:, 0] > 0).sum() >= 16
    assert (ref[0].bound[352:].reshape(32, 31)[:, 1:] <= 400 * 2 * shot_ref.FIX / np.sqrt((cshot[0] ** 2).sum())).all()


def test_dense_scene_is_dense():
    s = srs.scene("dense")
    assert len(set(s.rgba.tolist())) == 4 and int(s.kp_rgba[0]) in s.rgba and np.bincount(np.unique(s.rgba, return_inverse=True)[1]).min() > 4500
    assert (np.linalg.norm(s.points.astype(np.float64), axis=1) < s.radius).all() and len(s.points) == 20000

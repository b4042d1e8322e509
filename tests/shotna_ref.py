"""Restatement of the SHOTNA reference frame (third_party/pcl_shot_na_lrf/shot_na_lrf.hpp:48-178 of the reference) in numpy float64,
with the neighbour decision in float32 exactly as the library states it. Brute-force neighbours, one keypoint at a time.

  1. neighbours: finite surface points with float32 d2 < r2, d2 = ((dx*dx + dy*dy) + dz*dz) on the float32 differences, r2 =
     float32(float64(radius)^2); `valid` = those whose coordinates differ from the keypoint's; valid < 5 -> all NaN
  2. float64 covariance of the valid neighbours, weighted by radius - sqrt(d2), normalised by the weight sum; v1 / v3 = eigenvectors
     of the largest / smallest eigenvalue (numpy.linalg.eigh: their signs are arbitrary, the votes below fix them)
  3. x sign: plusT = 2 #(vij . v1 >= 0) - valid over the valid neighbours; < 0 flips; == 0: the five neighbours of rank
     valid/2 - 2 .. valid/2 + 2 by (d2, index) decide, v1 is flipped when fewer than three have vij . v1 > 0
  4. z sign: normal_votes=True (SHOTNA): plusN = 2 #(float64(normal) . v3 >= 0) - valid over ALL points inside the ball, a point on
     the keypoint included, a NaN normal never counting; normal_votes=False (SHOT): the positions of the valid neighbours, as for x.
     < 0 flips; == 0: the same five median neighbours decide BY POSITION
  5. x = float32(v1), z = float32(v3), y = z cross x in float32

One deviation from the reference's text: its x loop runs over every point in the ball and so reads rows of vij that were never written
when a point coincides with the keypoint; here, as in upstream PCL and in the library, the written rows are counted.

A vote with |dot| < SMALL may fall either way on another machine. A keypoint's x (z) sign is *decided* unless such votes could change
whether its sum is below 0, at 0 or above 0 (and, in a tie, whether three of the five medians are positive).

The normal votes have one more source of indecision, which is the reference's own: with c points ON the keypoint the sum runs over
valid + c votes but subtracts `valid`, so it is not antisymmetric in v3: for -v3 it is 2 c - plusN. The sign an eigen-solver gives its
eigenvector is arbitrary, and for 0 <= plusN <= 2 c the two signs end in opposite z axes. Such a keypoint is not decided either;
`v3_hint` orients the solver's v3 along a given direction first, for known answers."""
import numpy as np

f32, f64 = np.float32, np.float64
SMALL = 1e-7


def _cross_f32(z, x):
    return np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]], f32)


def _sign_of(plus, small, med_dots, coincident=0):
    """(flip, decided, tie) of one axis from its vote sum, the number of near-zero votes, the five median dot products and, for the
    normal votes, the number of voting points that lie on the keypoint"""
    if plus != 0:
        return plus < 0, plus - 2 * small > 2 * coincident or plus + 2 * small < 0, False
    pos = int((med_dots > 0).sum())
    med_small = int((np.abs(med_dots) < SMALL).sum())
    sure = int((med_dots >= SMALL).sum())                     # positives that stay positive
    decided = small == 0 and coincident == 0 and ((sure >= 3) == (sure + med_small >= 3))
    return pos < 3, decided, True


def frame_of_keypoint(points, normals, kp, radius, normal_votes=True, v3_hint=None):
    """one keypoint on one object's points / normals [n, 3] float32 (non-finite points are skipped) -> dict"""
    nan = dict(frame=np.full(9, np.nan, f32), valid=0, in_ball=0, plusT=0, plusN=0, gap=np.nan, small_x=0, small_z=0,
               decided_x=True, decided_z=True, tie_x=False, tie_z=False)
    kp = np.asarray(kp, f32)
    if not np.isfinite(kp).all() or len(points) == 0:
        return nan
    idx = np.nonzero(np.isfinite(points).all(1))[0]
    p, nrm = points[idx], normals[idx]
    d = (p - kp[None, :]).astype(f32)
    d2 = ((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32)
    d2 = (d2 + (d[:, 2] * d[:, 2]).astype(f32)).astype(f32)
    r2 = f32(f64(f32(radius)) * f64(f32(radius)))
    ball = d2 < r2
    val = ball & ~(p == kp[None, :]).all(1)
    valid, in_ball = int(val.sum()), int(ball.sum())
    nan.update(valid=valid, in_ball=in_ball)
    if valid < 5:
        return nan
    vij = d[val].astype(f64)
    w = f64(f32(radius)) - np.sqrt(d2[val].astype(f64))
    cov = (vij * w[:, None]).T @ vij / w.sum()
    ev, V = np.linalg.eigh(cov)
    if not np.isfinite(ev).all():
        return nan
    v1, v3 = V[:, 2].copy(), V[:, 0].copy()
    if v3_hint is not None and v3 @ np.asarray(v3_hint, f64) < 0:
        v3 = -v3
    gap = float(min(ev[2] - ev[1], ev[1] - ev[0]) / ev[2])
    order = np.lexsort((idx[val], d2[val]))                   # by distance, then by the point's index
    med = order[valid // 2 - 2: valid // 2 + 3]
    dx = vij @ v1
    plusT = int(2 * (dx >= 0).sum() - valid)
    small_x = int((np.abs(dx) < SMALL).sum())
    if normal_votes:
        dz = nrm[ball].astype(f64) @ v3
    else:
        dz = vij @ v3
    with np.errstate(invalid="ignore"):
        plusN = int(2 * (dz >= 0).sum() - valid)
        small_z = int((np.abs(dz) < SMALL).sum())
    flip_x, dec_x, tie_x = _sign_of(plusT, small_x, vij[med] @ v1)
    flip_z, dec_z, tie_z = _sign_of(plusN, small_z, vij[med] @ v3, in_ball - valid if normal_votes else 0)
    if flip_x:
        v1 = -v1
    if flip_z:
        v3 = -v3
    x, z = v1.astype(f32), v3.astype(f32)
    return dict(frame=np.concatenate([x, _cross_f32(z, x), z]).astype(f32), valid=valid, in_ball=in_ball, plusT=plusT, plusN=plusN, gap=gap,
                small_x=small_x, small_z=small_z, decided_x=dec_x, decided_z=dec_z, tie_x=tie_x, tie_z=tie_z)


def frames(pt_off, points, normals, kp_off, kps, radius, normal_votes=True):
    """ragged batch (offsets as the C ABI takes them) -> dict of arrays, one entry per keypoint"""
    rows = []
    for o in range(len(pt_off) - 1):
        p, n = points[pt_off[o]:pt_off[o + 1]], normals[pt_off[o]:pt_off[o + 1]]
        for k in range(kp_off[o], kp_off[o + 1]):
            rows.append(frame_of_keypoint(p, n, kps[k], radius, normal_votes))
    if not rows:
        return dict(frame=np.zeros((0, 9), f32))
    out = {key: np.asarray([r[key] for r in rows]) for key in rows[0]}
    out["decided"] = out["decided_x"] & out["decided_z"]
    return out

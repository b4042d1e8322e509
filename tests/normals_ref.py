"""PCA normals in float64, brute force (numpy only): the operation k_pca_normals / k_normals_from_lrf compute, stated once more
without a grid, without float sums and without an analytic eigen solver.

Neighbourhood: the DEVICE's decision, bit for bit in float32 (common.h's sqdist3): d = p - q per axis, d2 = (dx*dx + dy*dy) + dz*dz,
every operation rounded to float32, no FMA; neighbour iff d2 < r2 with r2 = float32(float64(r) * float64(r)); finite points of the
same object only, the point itself included; ORIGINAL coordinates for both orientations (method 1 of the reference shifts the cloud
by its centroid first and searches there: a stated difference).
Normal: fewer than 3 neighbours -> NaN; else the eigenvector of the smallest eigenvalue (numpy.linalg.eigh) of the float64 covariance
of the float64 differences p - q.
Orientation 0: flip when (0 - q) . n < 0.  Orientation 1: viewpoint c = float32(float64 mean of the object's finite points), then negate."""
import numpy as np

f32 = np.float32
GAP_MIN = 1e-3        # below this relative eigenvalue gap the direction is not determined well enough for the angle bound
COS_MIN = 1e-5        # below this |cos| of the flip decision float32 and float64 may decide differently
MARGIN_MIN = 1e-2     # raw_sign: margin between the two largest |components| below which PCL's float cross products may pick another
ANGLE_TOL = 2e-7      # rad: double arithmetic < 1e-9 at GAP_MIN, rounding a unit vector to float32 <= sqrt(3) * 2^-25 = 5.2e-8; ~4x that


def r2_of(radius):
    return f32(np.float64(f32(radius)) * np.float64(f32(radius)))


def sqdist3(p, q):
    """float32 squared distances of the rows of p [m, 3] to q [3] (or [m, 3]), in the device's operation order"""
    p, q = np.asarray(p, f32), np.asarray(q, f32)
    d = (p - q).astype(f32)
    xx, yy, zz = (d[..., 0] * d[..., 0]).astype(f32), (d[..., 1] * d[..., 1]).astype(f32), (d[..., 2] * d[..., 2]).astype(f32)
    return ((xx + yy).astype(f32) + zz).astype(f32)


def neighbour_mask(P, Q, radius, flip_equal=False):
    """[len(Q), len(P)] bool: P[j] is a neighbour of Q[i]; non-finite points are nobody's neighbour. flip_equal: d2 <= r2 instead
    (only to prove that a scene sits on the decision)"""
    P, Q = np.asarray(P, f32), np.asarray(Q, f32)
    fin = np.isfinite(P).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = sqdist3(P[None, :, :], Q[:, None, :])
        m = (d2 <= r2_of(radius)) if flip_equal else (d2 < r2_of(radius))
    return m & fin[None, :]


def angle(a, b):
    """unsigned angle between directions (rows), atan2(|a x b|, |a . b|) in float64: accurate near 0 where arccos is not"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(-1)))


def centroid32(P):
    """pcl::compute3DCentroid as grid.hip forms it: float64 mean of the finite points, rounded to float32"""
    P = np.asarray(P, f32)
    fin = np.isfinite(P).all(1)
    return P[fin].astype(np.float64).mean(0).astype(f32) if fin.any() else np.zeros(3, f32)


class Unoriented:
    """per point: eigenvector n [N, 3] float64 (sign as eigh left it; NaN rows below 3 neighbours or at non-finite points),
    count, gap = (l1 - l0) / l2 (0 where l2 == 0), margin between the two largest |components| of n"""

    def __init__(self, n, count, gap):
        self.n, self.count, self.gap = n, count, gap
        a = np.sort(np.abs(n), axis=1)
        self.margin = a[:, 2] - a[:, 1]
        self.valid = ~np.isnan(n).any(1)


def unoriented(pt_off, P, radius, flip_equal=False, chunk=128):
    P = np.asarray(P, f32)
    N = len(P)
    n = np.full((N, 3), np.nan)
    count = np.zeros(N, np.int64)
    gap = np.zeros(N)
    for o in range(len(pt_off) - 1):
        s, e = int(pt_off[o]), int(pt_off[o + 1])
        X = P[s:e]
        fin = np.isfinite(X).all(1)
        X64 = np.where(fin[:, None], X, 0).astype(np.float64)
        for a in range(0, e - s, chunk):
            b = min(a + chunk, e - s)
            m = neighbour_mask(X, np.where(fin[a:b, None], X[a:b], 0), radius, flip_equal) & fin[a:b, None]
            c = m.sum(1)
            d = (X64[None, :, :] - X64[a:b, None, :]) * m[:, :, None]
            cc = np.maximum(c, 1)[:, None]
            mean = d.sum(1) / cc
            d = (d - mean[:, None, :]) * m[:, :, None]
            cov = np.einsum("qpi,qpj->qij", d, d) / cc[:, :, None]
            w, v = np.linalg.eigh(cov)
            ok = c >= 3
            count[s + a:s + b] = c
            with np.errstate(invalid="ignore", divide="ignore"):
                gap[s + a:s + b] = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
            n[s + a:s + b] = np.where(ok[:, None], v[:, :, 0], np.nan)
    gap[np.isnan(n).any(1)] = 0.0
    return Unoriented(n, count, gap)


def orient(pt_off, P, u, orientation):
    """-> (normals [N, 3] float64, |cos| [N]): |cos| = |(viewpoint - q) . n| / |viewpoint - q| of the flip decision"""
    P64 = np.asarray(P, f32).astype(np.float64)
    vp = np.zeros_like(P64)
    if orientation == 1:
        for o in range(len(pt_off) - 1):
            s, e = int(pt_off[o]), int(pt_off[o + 1])
            vp[s:e] = centroid32(P[s:e]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = vp - P64
        dot = (v * u.n).sum(1)
        dist = np.linalg.norm(v, axis=1)
        cos = np.where(dist > 0, np.abs(dot) / dist, 0.0)
        out = np.where((dot < 0)[:, None], -u.n, u.n)
    if orientation == 1:
        out = -out
    cos[~u.valid] = 0.0
    return out, cos


def raw_sign(n):
    """n with the sign pcl::eigen33 gives its eigenvector before any viewpoint flip. B = A - l0 I is symmetric with null vector v, so
    the cross products of its rows are r0 x r1 = mu v2 v, r0 x r2 = -mu v1 v, r1 x r2 = mu v0 v with mu = (l1 - l0)(l2 - l0) > 0, and
    eigen33 normalises the longest: the component of largest magnitude comes out positive when it is x or z, negative when it is y."""
    n = np.asarray(n, np.float64)
    out = n.copy()
    ok = ~np.isnan(n).any(1)
    k = np.argmax(np.abs(n[ok]), axis=1)
    big = n[ok][np.arange(ok.sum()), k]
    want_pos = k != 1
    out[ok] = np.where(((big > 0) == want_pos)[:, None], n[ok], -n[ok])
    return out

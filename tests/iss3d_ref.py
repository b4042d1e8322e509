"""numpy / scipy restatement of the ISS3D keypoint detector (include/ismhip.h: ismhip_iss3d_saliency,
ismhip_iss3d_keypoints), one object at a time. It is the checker of tests/test_gpu_iss3d.py and is itself checked against hand-derived
answers in tests/test_iss3d_cpu.py.

Neighbours are decided on the float32 values in the library's order, d2 = (dx*dx + dy*dy) + dz*dz without fused multiply-adds, strictly
below (float)((double)r * r), the query included; scipy's kd-tree (double) only shortlists. The scatter matrix (about the query, not
divided by the count) and its eigenvalues are float64.

Besides the answer the restatement returns an `undecided` mask: the points whose outcome another correct float64 evaluation could turn.
The margin is derived, not tuned: a fixed-order float64 sum of a few hundred outer products followed by a Jacobi solve to 1e-22
off-diagonal is good to about 1e-13 * e1 (forward against reversed summation order differs by at most 5e-13 relative), so MARGIN = 1e-9
leaves four orders of headroom."""
import numpy as np
from scipy.spatial import cKDTree

from prefilter_ref import finite, sqd32

MARGIN = 1e-9


def r2_of(radius):
    return np.float32(np.float64(np.float32(radius)) * np.float64(np.float32(radius)))


def neighbours(p, radius):
    """per point of p (finite float32 [n, 3]) the indices with d2 < r2, ascending, the point itself included"""
    r2 = r2_of(radius)
    if not len(p):
        return []
    p64 = p.astype(np.float64)
    lists = cKDTree(p64).query_ball_point(p64, float(np.float32(radius)) * 1.001 + 1e-12)
    out = []
    for i, l in enumerate(lists):
        l = np.sort(np.asarray(l, np.int64))
        out.append(l[sqd32(p[i][None, :], p[l]) < r2])
    return out


def scatter(p, i, nb):
    d = p[nb].astype(np.float64) - p[i].astype(np.float64)
    return d.T @ d


def iss3d(xyz, salient_radius=0.1, non_max_radius=0.05, gamma21=0.975, gamma32=0.975, min_neighbors=5):
    """-> dict: saliency float64[n], eig float64[n, 3] (e1 >= e2 >= e3), count int64[n] (salient-radius neighbours), keep bool[n],
    undecided bool[n]; non-finite points: zeros / False"""
    xyz = np.asarray(xyz, np.float32)
    n_all = len(xyz)
    fin = finite(xyz) if n_all else np.zeros(0, bool)
    p = xyz[fin]
    n = len(p)
    sal = np.zeros(n, np.float64); eig = np.zeros((n, 3), np.float64); cnt = np.zeros(n, np.int64)
    open_s = np.zeros(n, bool)                              # the ratio tests (or e3 >= 0) lie inside the margin
    ns = neighbours(p, salient_radius)
    for i in range(n):
        cnt[i] = len(ns[i])
        if cnt[i] < min_neighbors:
            continue                                        # zero matrix: eigenvalues 0, 0 / 0 fails the tests, never salient
        w = np.linalg.eigvalsh(scatter(p, i, ns[i]))        # ascending
        e1, e2, e3 = w[2], w[1], w[0]
        eig[i] = (e1, e2, e3)
        m = MARGIN * e1
        open_s[i] = abs(e3) <= m or abs(e2 - gamma21 * e1) <= m or abs(e3 - gamma32 * e2) <= m
        if not np.isfinite(w).all() or e3 < 0:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            if e2 / e1 < gamma21 and e3 / e2 < gamma32:
                sal[i] = e3
    keep = np.zeros(n, bool); open_n = open_s.copy()
    nn = neighbours(p, non_max_radius)
    for i in range(n):
        if open_s[i] or not sal[i] > 0:
            continue
        nb = nn[i]
        others = nb[nb != i]
        if open_s[others].any():
            open_n[i] = True
        close = np.abs(sal[others] - sal[i]) <= MARGIN * np.maximum(eig[others, 0], eig[i, 0])
        if (close & (sal[others] > 0)).any():
            open_n[i] = True
        keep[i] = len(nb) >= min_neighbors and not (sal[nb] > sal[i]).any()
    out = dict(saliency=np.zeros(n_all), eig=np.zeros((n_all, 3)), count=np.zeros(n_all, np.int64), keep=np.zeros(n_all, bool),
               undecided=np.zeros(n_all, bool))
    out["saliency"][fin] = sal; out["eig"][fin] = eig; out["count"][fin] = cnt; out["keep"][fin] = keep; out["undecided"][fin] = open_n
    out["undecided_saliency"] = np.zeros(n_all, bool); out["undecided_saliency"][fin] = open_s
    return out

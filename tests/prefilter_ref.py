"""numpy / scipy restatement of the point-cloud pre-filters (include/ismhip.h): statistical outlier removal,
radius outlier removal and the z pass-through, one object at a time. It is the checker of tests/test_gpu_prefilter.py and is itself
checked against hand-derived answers in tests/test_prefilter_cpu.py.

The deciding arithmetic is float32 in the library's order: d2 = (dx*dx + dy*dy) + dz*dz without fused multiply-adds. scipy's kd-tree
(double) only shortlists candidates; which of them count is decided on the float32 values."""
import numpy as np
from scipy.spatial import cKDTree


def sqd32(a, b):
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float32)
    return ((d[..., 0] * d[..., 0]).astype(np.float32) + (d[..., 1] * d[..., 1]).astype(np.float32)).astype(np.float32) + \
        (d[..., 2] * d[..., 2]).astype(np.float32)


def finite(xyz):
    return np.isfinite(np.asarray(xyz, np.float32)).all(axis=1)


def sor_mean_dist(xyz, mean_k):
    """mean distance to the mean_k nearest other points, float32 [n]; NaN for non-finite points. None when the object holds fewer
    than mean_k + 1 finite points (it is kept whole)."""
    xyz = np.asarray(xyz, np.float32)
    fin = finite(xyz)
    p = xyz[fin]
    n = len(p)
    if n < mean_k + 1:
        return None
    kk = min(n, mean_k + 9)
    tree = cKDTree(p.astype(np.float64))
    _, idx = tree.query(p.astype(np.float64), k=kk)
    idx = idx.reshape(n, kk)
    d2 = np.sort(sqd32(p[:, None, :], p[idx]), axis=1)
    if kk < n:
        # the shortlist is complete where its (mean_k + 1)-th float distance lies strictly below its farthest candidate; the few
        # other rows are decided over all points
        for i in np.nonzero(~(d2[:, mean_k] < d2[:, -1]))[0]:
            d2[i, :mean_k + 1] = np.sort(sqd32(p[i][None, :], p))[:mean_k + 1]
    s = np.zeros(n, np.float64)
    for j in range(1, mean_k + 1):                       # the smallest (the point itself) is dropped; ascending, in double
        s += np.sqrt(d2[:, j].astype(np.float64))
    md = np.full(len(xyz), np.nan, np.float32)
    md[fin] = (s / mean_k).astype(np.float32)
    return md


def sor_threshold(mean_dist, stddev_mul):
    """the closed formula on the finite entries of mean_dist, in double"""
    d = np.asarray(mean_dist)[np.isfinite(mean_dist)].astype(np.float64)
    n = len(d)
    s, q = d.sum(), (d * d).sum()
    mean = s / n
    var = (q - s * s / n) / (n - 1)
    return mean + float(stddev_mul) * np.sqrt(var)


def sor(xyz, mean_k=20, stddev_mul=2.0):
    """-> keep bool[n], mean_dist float32[n] (NaN: non-finite point or small object), threshold (inf for a small object)"""
    if mean_k < 1:
        raise ValueError("MeanK < 1")
    fin = finite(xyz)
    md = sor_mean_dist(xyz, mean_k)
    if md is None:
        return fin.copy(), np.full(len(xyz), np.nan, np.float32), np.inf
    thr = sor_threshold(md, stddev_mul)
    return fin & ~(md.astype(np.float64) > thr), md, thr


def ror_counts(xyz, radius):
    """finite points with d2 < r2 (float32, strict), the point itself included; 0 for non-finite points"""
    xyz = np.asarray(xyz, np.float32)
    fin = finite(xyz)
    p = xyz[fin]
    r2 = np.float32(np.float64(np.float32(radius)) * np.float64(np.float32(radius)))
    cnt = np.zeros(len(p), np.int64)
    if len(p):
        tree = cKDTree(p.astype(np.float64))
        lists = tree.query_ball_point(p.astype(np.float64), float(radius) * 1.001 + 1e-12)
        for i, l in enumerate(lists):
            cnt[i] = int((sqd32(p[i][None, :], p[np.asarray(l, np.int64)]) < r2).sum())
    out = np.zeros(len(xyz), np.int64)
    out[fin] = cnt
    return out


def ror(xyz, radius=0.005, min_neighbors=10):
    cnt = ror_counts(xyz, radius)
    return finite(xyz) & (cnt > min_neighbors), cnt


def passthrough_z(xyz, z_min, z_max):
    xyz = np.asarray(xyz, np.float32)
    z = xyz[:, 2]
    return finite(xyz) & ~((z < np.float32(z_min)) | (z > np.float32(z_max)))


def prefilter(xyz, use_sor=False, mean_k=20, stddev_mul=2.0, use_ror=False, radius=0.005, min_neighbors=10, cutoff_z=0.0):
    """the host's filter stage on one object: SOR, ROR on its output, z cut-off on that; returns the indices of the survivors"""
    idx = np.arange(len(xyz))
    if use_sor:
        idx = idx[sor(xyz[idx], mean_k, stddev_mul)[0]]
    if use_ror:
        idx = idx[ror(xyz[idx], radius, min_neighbors)[0]]
    if cutoff_z > 0:
        idx = idx[passthrough_z(xyz[idx], 0.0, cutoff_z)]
    return idx


def per_object(pt_off, fn):
    """applies fn(begin, end) to every object of a batch"""
    return [fn(int(pt_off[o]), int(pt_off[o + 1])) for o in range(len(pt_off) - 1)]

"""numpy restatement of the SIFT3D keypoint detector's stages (include/ismhip.h: ismhip_sift3d_scale_space,
ismhip_sift3d_extrema, ismhip_voxel_downsample_xyzi), one object at a time. It is the checker of tests/test_gpu_sift3d.py and is itself
checked against known answers in tests/test_sift3d_cpu.py.

Squared distances are the library's float32 values, d2 = (dx*dx + dy*dy) + dz*dz without fused multiply-adds (prefilter_ref.sqd32); which
neighbours enter a sum (d2 <= 9.0f * s2, s2 = fl32(s * s)) and the order of the 25 nearest ((d2, index) ascending) are decided on them, so
they are exact and always decided. Every `dog` value is float64, and comes with a bound on |kernel - float64| derived from the kernel's
own arithmetic:

  a   = (-0.5f * d2) / s2        the product is exact; one float division, |da| <= 2^-23 |a| (one ulp allowed, correctly rounded is half)
  w   = expf(a)                  OCML's exp is good to 1 ulp, ulp(w) <= 2^-23 w; the error of a enters as w |da|:
                                 |dw| <= w (|a| + 1) 2^-23,  |a| <= 4.5
  w I                            one float product, 2^-24 relative, then rounded to the numerator's grid q_n = 2^(ei - bits), 2^ei the power
                                 of two above the object's largest finite |I|: q_n / 2 per term
  w                              rounded to the denominator's grid q_d = 2^(1 - bits): q_d / 2 per term
  E_n = sum |I| w ((|a| + 1) 2^-23 + 2^-24) + n q_n / 2,   E_d = sum w (|a| + 1) 2^-23 + n q_d / 2
  response = (float)(num / den)  |d response| <= (E_n + |response| E_d) / (den - E_d) + 2^-24 |response|  (the double quotient adds 2^-52)
  dog = response_i - response_{i-1} in float: the two bounds and 2^-24 |dog|

bits = 48 for objects below 2^14 points, one fewer per doubling (grid_bits). An extremum test is DECIDED when a comparison it rests on fails
by more than the two bounds involved, or when all of them hold by more than that; the rest is undecided and is not compared."""
import math

import numpy as np
from scipy.spatial import cKDTree

from culling_ref import grid_bits
from prefilter_ref import finite, sqd32

F = np.float32
MIN_POINTS = 25                      # ISMHIP_SIFT3D_MIN_POINTS
U23, U24 = 2.0 ** -23, 2.0 ** -24


def scales(base_scale, nr_scales):
    """scales[i] = base_scale * powf(2.0f, (i - 1.0f) / nr_scales), i = 0 .. nr_scales + 2, every step in float; powf as the correctly
    rounded float of the double power"""
    out = []
    for i in range(nr_scales + 3):
        e = F(F(F(i) - F(1.0)) / F(nr_scales))
        out.append(F(F(base_scale) * F(math.pow(2.0, float(e)))))
    return np.array(out, np.float32)


def knn(p, k):
    """per point of p (finite float32 [n, 3]) its k nearest by (d2, index) ascending, itself included: int32 [n, k], -1 behind"""
    n = len(p)
    out = np.full((n, k), -1, np.int32)
    idx = np.arange(n)
    for i in range(n):
        d2 = sqd32(p[i][None, :], p)
        order = np.lexsort((idx, d2))[:k]
        out[i, :len(order)] = order
    return out


def dog(xyz, intensity, sc):
    """-> (dog float64 [n, len(sc) - 1], bound float64 [n, len(sc) - 1], count int64 [n]) in the order of xyz; rows of points whose position
    or intensity is not finite: NaN, NaN, 0. count: the points with d2 <= 9 max(s2) and a finite intensity"""
    xyz = np.asarray(xyz, np.float32); inten = np.asarray(intensity, np.float32); sc = np.asarray(sc, np.float32)
    n_all, ns = len(xyz), len(sc)
    D = np.full((n_all, ns - 1), np.nan); B = np.full((n_all, ns - 1), np.nan); cnt = np.zeros(n_all, np.int64)
    fin = finite(xyz) if n_all else np.zeros(0, bool)
    use = fin & np.isfinite(inten)
    if not use.any():
        return D, B, cnt
    rows = np.nonzero(use)[0]
    p = xyz[use]; I = inten[use].astype(np.float64)
    s2 = (sc * sc).astype(np.float32); lim = (F(9.0) * s2).astype(np.float32)
    bits = grid_bits(int(fin.sum()))
    ei = math.frexp(float(np.abs(inten[use]).max()))[1]
    qn, qd = 2.0 ** (ei - bits), 2.0 ** (1 - bits)
    p64 = p.astype(np.float64)
    lists = cKDTree(p64).query_ball_point(p64, 3.0 * float(sc.max()) * 1.001 + 1e-12)
    for i, l in enumerate(lists):
        l = np.asarray(l, np.int64)
        d2 = sqd32(p[i][None, :], p[l])
        cnt[rows[i]] = int((d2 <= lim.max()).sum())
        resp = np.zeros(ns); rb = np.zeros(ns)
        for s in range(ns):
            m = d2 <= lim[s]
            a = -0.5 * d2[m].astype(np.float64) / float(s2[s])
            w = np.exp(a)
            relw = (np.abs(a) + 1.0) * U23
            num, den = float((w * I[l[m]]).sum()), float(w.sum())
            En = float((np.abs(I[l[m]]) * w * (relw + U24)).sum()) + m.sum() * qn / 2
            Ed = float((w * relw).sum()) + m.sum() * qd / 2
            resp[s] = num / den
            rb[s] = (En + abs(resp[s]) * Ed) / (den - Ed) + (U24 + 2.0 ** -50) * abs(resp[s])
        d = resp[1:] - resp[:-1]
        D[rows[i]] = d
        B[rows[i]] = rb[1:] + rb[:-1] + U24 * np.abs(d)
    return D, B, cnt


def extrema(xyz, D, B, k=MIN_POINTS, min_contrast=0.0, nn=None):
    """-> (flags uint8 [n, n_cols]: 0 none, 1 minimum, 2 maximum; undecided bool [n, n_cols]; nn int32 [n, k]) by the float64 columns D
    and their bounds B (B = None: exact values, everything decided). Strict comparisons; rows of non-finite points stay 0 / -1"""
    xyz = np.asarray(xyz, np.float32)
    n_all, nc = D.shape
    flags = np.zeros((n_all, nc), np.uint8); und = np.zeros((n_all, nc), bool)
    nn_all = np.full((n_all, k), -1, np.int32)
    fin = finite(xyz) if n_all else np.zeros(0, bool)
    rows = np.nonzero(fin)[0]
    if not len(rows):
        return flags, und, nn_all
    if nn is None:
        nn = knn(xyz[fin], k)
    nn_all[rows] = np.where(nn >= 0, rows[np.maximum(nn, 0)], -1)
    if B is None:
        B = np.zeros_like(D)
    for r, i in enumerate(rows):
        nb = [rows[j] for j in nn[r] if j >= 0 and rows[j] != i]
        for c in range(1, nc - 1):
            v, bv = D[i, c], B[i, c]
            if not (abs(v) >= min_contrast):              # a NaN never passes
                und[i, c] = min_contrast > 0 and abs(abs(v) - min_contrast) <= bv
                continue
            contrast_open = min_contrast > 0 and abs(abs(v) - min_contrast) <= bv
            others = [(D[i, c - 1], B[i, c - 1]), (D[i, c + 1], B[i, c + 1])]
            for q in nb:
                others += [(D[q, c - 1], B[q, c - 1]), (D[q, c], B[q, c]), (D[q, c + 1], B[q, c + 1])]
            u = np.array([o[0] for o in others]); bu = np.array([o[1] for o in others]) + bv
            for flag, holds, fails in ((2, v > u, ~(v > u)), (1, v < u, ~(v < u))):
                close = (np.abs(v - u) <= bu) & (bu > 0)   # exact columns (bound 0) are always decided, a tie fails; so does a NaN
                if (fails & ~close).any():
                    continue                               # decisively not this kind of extremum
                if close.any() or contrast_open:
                    und[i, c] = True
                elif holds.all():
                    flags[i, c] = flag
    return flags, und, nn_all


def voxel_mean_bound(mean64, max_abs):
    """|kernel - float64 mean| of a voxel's intensity: every term rounded to 2^-40 of the power of two above the object's largest |I|
    (half a quantum each, so half a quantum on the mean), the sum rounded to float (2^-24) and the float division (2^-24)"""
    ei = math.frexp(float(max_abs))[1]
    return 0.5 * 2.0 ** (ei - 40) + 2.0 ** -23 * np.abs(mean64) * (1.0 + 2.0 ** -20)


def voxel_means(xyz, intensity, leaf):
    """float64 mean intensity per occupied voxel in ascending voxel index, and the voxels' point counts, by the index rule of
    ismhip_voxel_keypoints (floor(p * (1 / leaf)) in float32 about the bounding box's first cell); finite points only"""
    xyz = np.asarray(xyz, np.float32); inten = np.asarray(intensity, np.float32)
    use = finite(xyz) & np.isfinite(inten)
    p, I = xyz[use], inten[use].astype(np.float64)
    inv = F(1.0) / F(leaf)
    cell = np.floor((p * inv).astype(np.float32)).astype(np.int64)
    lo = np.floor((p.min(0) * inv).astype(np.float32)).astype(np.int64); hi = np.floor((p.max(0) * inv).astype(np.float32)).astype(np.int64)
    div = hi - lo + 1
    v = (cell[:, 0] - lo[0]) + (cell[:, 1] - lo[1]) * div[0] + (cell[:, 2] - lo[2]) * div[0] * div[1]
    ids, inv_idx, counts = np.unique(v, return_inverse=True, return_counts=True)
    sums = np.zeros(len(ids)); np.add.at(sums, inv_idx, I)
    return sums / counts, counts

"""numpy restatement of the VoxelGridCulling keypoint detector (include/ismhip.h: ismhip_principal_curvatures,
ismhip_culling_scores, ismhip_culling_select), one object at a time. It is the checker of tests/test_gpu_culling.py and is itself checked
against hand-derived answers in tests/test_culling_cpu.py.

PCL is external. Where PCL decides the arithmetic (the curvature of pcl::NormalEstimation, pcl::PrincipalCurvaturesEstimation) the
definition below is this library's own, written from knowledge of PCL 1.10; parity with PCL is unpinned. Where the reference's own source
decides it (keypoints/keypoints_voxel_grid_culling.cpp: computeKPQ :441-471, computeColorScore :474-506, the combined score :331-340,
computeThresholds :346-432, acceptance :204-272) the text is followed as written, oddities included.

Surface, keypoints, ball. The surface is the batch's search surface with its finite points; keypoints are what ismhip_voxel_keypoints
gives at LeafSize; every ball has radius LeafSize: d2 = (dx*dx + dy*dy) + dz*dz in unfused float32, a neighbour iff d2 <
float32(float64(r) * r); non-finite points are never neighbours.

curvature     n = ball count; n < 3: NaN; else C = sum (p - m)(p - m)^T / n about the neighbours' mean m, e3 its smallest eigenvalue,
              score = float32(|e3 / trace(C)|), 0 when the trace is 0.
pc1, pc2      per surface point i with normal n, over its ball N (i included; neighbours with a non-finite normal skipped, not counted):
              v_j = n_j - n (n . n_j) in float64 from the float32 normals, c = mean v_j, S = sum (v_j - c)(v_j - c)^T (NOT divided),
              eigenvalues l0 <= l1 <= l2; pc1 = float32(l2 / |N|), pc2 = float32(l1 / |N|); NaN for a point whose own normal or position
              is not finite.
kpq           over the keypoint's ball, K = pc1 * pc2 in float32; max_k1, max_K start at FLT_MIN, min_k2, min_K at FLT_MAX and move by the
              comparisons as written (a NaN never moves them); float32, left to right:
              (1000 / num * num) * sum K + 100 * max_K + |100 * min_K| + 10 * max_k1 + |10 * min_k2|   (the precedence of 1000 / num * num is
              the source's); sum K exact (math.fsum), rounded once to float32, NaN if any K is NaN; empty ball: NaN.
colordistance the keypoint's averaged colour through RGB -> normalised CIELab is the reference; per ball point the distance
              (|dL| + (|da| + |db|) / 2) / 3 in float64 from the float32 differences, clamped to [0, 1], as float32;
              score = float32(count(distance > MaxSimilarColorDistance)) / float32(n); empty ball: NaN (0 / 0).
combined      (g - gmin) / gmax + (c - cmin) / cmax in float32 -- the division is by the maximum, not by the range; min and max are the
              first smallest / largest of the object's non-NaN scores (none: +inf / -inf).
thresholds    cutoff: the element at index min(unsigned(ratio * float32(size)), size - 1) of the ascending list, NaN behind +inf, ties
              by index; threshold: the configured value; the combined threshold exists only when both methods are on and both types are
              cutoff; whatever is not set stays FLT_MIN, as written.
acceptance    a test passes iff not (score < threshold), so a NaN score passes; both methods on: RequireOne / RequireBoth /
              RequireCombinedList; otherwise geo_passed and color_passed. Kept keypoints: the voxel keypoints themselves, in their order.

Bounds (derived, not tuned). The device sums on an integer grid of 2^-47 or finer of the terms' bound and solves the same Jacobi
iteration as ISS3D, whose eigenvalues section 4.14 holds to MARGIN = 1e-9 of the largest eigenvalue against a float64 evaluation (the
true error is near 1e-13). Carried through:
  curvature = |e3 / t|, t the trace >= e1: |d(e3 / t)| <= |de3| / t + (e3 / t) |dt| / t <= MARGIN (1 + 3 * score) <= 2 MARGIN as score <= 1 / 3;
              plus one float32 rounding 2^-24 |score|                                      -> curvature_bound
  pc        = l / |N|: |d pc| <= MARGIN * l2 / |N| + 2^-24 |pc|                             -> pc_bound
  kpq         two float32 values that round float64 values within MARGIN * pc1 of each other differ by at most dk = MARGIN * pc1 +
              2^-23 |k|; K = k1 * k2 then differs by dK = |k1| dk2 + |k2| dk1 + dk1 dk2 + 2^-23 |K|; with A = 1000 / num * num the
              expression differs by A * sum dK + 100 * max dK (max_K) + 100 * max dK (min_K) + 10 * max dk1 + 10 * max dk2, plus the eight
              float32 operations of the expression and the single rounding of sum K, each 2^-23 of the terms' absolute sum -> kpq_bound
The grid adds a floor that does not shrink with the eigenvalues (format precision, not tuning). bits = grid_bits(points of the object):
48 up to 2^14 - 2 points, one fewer per doubling. A product is rounded to q2 = 2^(e2 - bits) <= 2 W 2^-bits, W the bound of the terms, a
component to q1 <= 2 sqrt(W) 2^-bits. Per entry of the centred matrix divided by the count: q2 / 2 from the products plus |c| q1 <= 2 W 2^-bits
from the mean, together below 3 W 2^-bits; an eigenvalue moves by at most the Frobenius norm, 3 entries' worth: 9 W 2^-bits, taken as
FLOOR = 16 W 2^-bits. W = B (1 + B)^2 for the projected normals (B the object's largest squared normal length): pc_bound += FLOOR. W = r2
for the curvature, whose quotient divides by the trace: curvature_bound += 2 * FLOOR(r2) / trace(C) (e3 and the trace each move). sum K sits
on the grid of the object's largest finite |K|: kpq_bound += A * n * 2 * Kmax * 2^-bits.
An `undecided` keypoint is one whose outcome another correct evaluation could turn: a ball point within the float32 summation margin
(4 * 2^-24 * r2) of d2 == r2, or eigenvalues of C within MARGIN * e1 of a tie."""
import math

import numpy as np

from iss3d_ref import neighbours, r2_of
from prefilter_ref import finite, sqd32

f32 = np.float32
MARGIN = 1e-9
FLT_MIN = np.finfo(f32).tiny
FLT_MAX = np.finfo(f32).max
NAN32 = f32(np.nan)


# ---- balls -------------------------------------------------------------------------------------------------------------------------
def ball(p, q, radius):
    """indices of the finite float32 points p [n, 3] inside the ball of float32 q [3], ascending"""
    if not len(p) or not np.isfinite(q).all():
        return np.zeros(0, np.int64)
    return np.nonzero(sqd32(np.asarray(q, f32)[None, :], p) < r2_of(radius))[0]


def near_boundary(p, q, radius):
    """a point of p within the float32 summation margin of d2 == r2"""
    if not len(p):
        return False
    d = p.astype(np.float64) - np.asarray(q, np.float64)
    r2 = float(r2_of(radius))
    return bool((np.abs((d * d).sum(1) - r2) <= 4 * 2.0 ** -24 * r2).any())


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def curvature(p, q, radius):
    """-> (score float32, count, undecided) of keypoint q on the finite points p"""
    nb = ball(p, q, radius)
    und = near_boundary(p, q, radius)
    if len(nb) < 3:
        return NAN32, len(nb), und
    pts = p[nb].astype(np.float64)
    d = pts - pts.mean(0)
    C = d.T @ d / len(nb)
    w = np.linalg.eigvalsh(C)
    tr = np.trace(C)
    und = und or bool(w[1] - w[0] <= MARGIN * w[2])
    return (f32(0) if tr == 0 else f32(abs(w[0] / tr))), len(nb), und


def curvature64(p, q, radius):
    nb = ball(p, q, radius)
    pts = p[nb].astype(np.float64)
    d = pts - pts.mean(0)
    C = d.T @ d / len(nb)
    tr = np.trace(C)
    return 0.0 if tr == 0 else abs(np.linalg.eigvalsh(C)[0] / tr)


def grid_bits(n_points):
    bits = 48
    while bits > 24 and n_points + 1 >= 1 << (62 - bits):
        bits -= 1
    return bits


def grid_floor(w, n_points):
    return 16.0 * w * 2.0 ** -grid_bits(n_points)


def curvature_trace(p, q, radius):
    pts = p[ball(p, q, radius)].astype(np.float64)
    d = pts - pts.mean(0)
    return float((d * d).sum() / len(pts))


def curvature_bound(score64, trace, radius, n_points):
    with np.errstate(all="ignore"):
        return 2 * MARGIN + 2.0 ** -24 * abs(score64) + (2 * grid_floor(float(r2_of(radius)), n_points) / trace if trace > 0 else 0.0)


def principal_curvatures(xyz, normals, radius):
    """-> dict pc1, pc2 float32 [n], count int64 [n], pc1_64, pc2_64 float64 [n] (before the rounding) in the order of xyz"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3); normals = np.asarray(normals, f32).reshape(-1, 3)
    n_all = len(xyz)
    out = dict(pc1=np.full(n_all, np.nan, f32), pc2=np.full(n_all, np.nan, f32), count=np.zeros(n_all, np.int64),
               pc1_64=np.full(n_all, np.nan), pc2_64=np.full(n_all, np.nan), floor=0.0, bits=grid_bits(0))
    fin = finite(xyz) if n_all else np.zeros(0, bool)
    where = np.nonzero(fin)[0]
    p, nrm = xyz[fin], normals[fin].astype(np.float64)
    ok = np.isfinite(nrm).all(1)
    B = float((nrm[ok] ** 2).sum(1).max()) if ok.any() else 0.0
    out["bits"] = grid_bits(len(p))
    out["floor"] = grid_floor(B * (1.0 + B) ** 2, len(p))
    for i, nb in enumerate(neighbours(p, radius)):
        if not ok[i]:
            continue
        nb = nb[ok[nb]]
        n = nrm[i]
        v = nrm[nb] - n[None, :] * (nrm[nb] @ n)[:, None]
        d = v - v.mean(0)
        w = np.linalg.eigvalsh(d.T @ d)
        k = where[i]
        out["count"][k] = len(nb)
        out["pc1_64"][k], out["pc2_64"][k] = w[2] / len(nb), w[1] / len(nb)
        out["pc1"][k], out["pc2"][k] = f32(w[2] / len(nb)), f32(w[1] / len(nb))
    return out


def pc_bound(pc1_64, pc_64, floor):
    return MARGIN * np.abs(pc1_64) + 2.0 ** -24 * np.abs(pc_64) + floor


def kpq(pc1, pc2, idx):
    """computeKPQ over the ball's point indices idx (in any order: only sum K depends on it and it is exact here)"""
    if len(idx) == 0:
        return NAN32
    max_k1, min_k2, max_K, min_K = f32(FLT_MIN), f32(FLT_MAX), f32(FLT_MIN), f32(FLT_MAX)
    Ks = []
    with np.errstate(all="ignore"):
        for i in idx:
            k_1, k_2 = f32(pc1[i]), f32(pc2[i])
            K = f32(k_1 * k_2)
            if k_1 > max_k1:
                max_k1 = k_1
            if k_2 < min_k2:
                min_k2 = k_2
            if K > max_K:
                max_K = K
            if K < min_K:
                min_K = K
            Ks.append(float(K))
        total = f32(np.nan) if np.isnan(Ks).any() else f32(sum(Ks) if np.isinf(Ks).any() else math.fsum(Ks))
        num = f32(len(idx))
        r = f32(f32(f32(1000.0) / num) * num) * total
        r = f32(r + f32(f32(100.0) * max_K))
        r = f32(r + np.abs(f32(f32(100.0) * min_K)))
        r = f32(r + f32(f32(10.0) * max_k1))
        r = f32(r + np.abs(f32(f32(10.0) * min_k2)))
    return r


def kpq_bound(pc1, pc2, pc1_64, idx, floor=0.0, bits=48):
    """how far two evaluations of kpq may lie apart whose pc inputs each hold pc_bound (see the head of the file)"""
    if len(idx) == 0:
        return 0.0
    k1, k2 = np.abs(pc1[idx].astype(np.float64)), np.abs(pc2[idx].astype(np.float64))
    lead = MARGIN * np.abs(np.asarray(pc1_64, np.float64)[idx]) + floor
    with np.errstate(all="ignore"):
        every = np.abs(np.asarray(pc1, f32) * np.asarray(pc2, f32)).astype(np.float64)
    kmax = float(every[np.isfinite(every)].max()) if np.isfinite(every).any() else 0.0
    dk1, dk2 = lead + 2.0 ** -23 * k1, lead + 2.0 ** -23 * k2
    K = k1 * k2
    dK = k1 * dk2 + k2 * dk1 + dk1 * dk2 + 2.0 ** -23 * K
    A = 1000.0
    terms = A * K.sum() + 100.0 * K.max() + 100.0 * K.max() + 10.0 * k1.max() + 10.0 * k2.max()
    return A * dK.sum() + 200.0 * dK.max() + 10.0 * dk1.max() + 10.0 * dk2.max() + 9 * 2.0 ** -23 * terms + A * len(idx) * 2.0 * (kmax + K.max()) * 2.0 ** -bits


# ---- colour ------------------------------------------------------------------------------------------------------------------------
def color_distance(lab_ref, lab):
    """getColorDistance on normalised CIELab: float32 [3] against float32 [n, 3] -> float32 [n]"""
    lab_ref = np.asarray(lab_ref, f32); lab = np.asarray(lab, f32).reshape(-1, 3)
    dl = np.abs((lab_ref[0] - lab[:, 0]).astype(f32)).astype(np.float64)
    da = np.abs((lab_ref[1] - lab[:, 1]).astype(f32)).astype(np.float64)
    db = np.abs((lab_ref[2] - lab[:, 2]).astype(f32)).astype(np.float64)
    return np.clip((dl + (da + db) / 2.0) / 3.0, 0.0, 1.0).astype(f32)


def color_score(lab_ref, lab_ball, max_similar_color_distance):
    """-> (score float32, distant count)"""
    n = len(lab_ball)
    distant = int((color_distance(lab_ref, lab_ball) > f32(max_similar_color_distance)).sum()) if n else 0
    with np.errstate(all="ignore"):
        return f32(f32(distant) / f32(n)), distant


def lab_table(rgb2lab, colors):
    """normalised CIELab of packed 0x00RRGGBB colours -> float32 [n, 3]; rgb2lab (the oracle's) runs once per distinct colour"""
    colors = np.asarray(colors, np.uint32).reshape(-1)
    uniq, inv = np.unique(colors, return_inverse=True)
    raw = np.array([rgb2lab(int(c)) for c in uniq], f32).reshape(-1, 3)
    norm = np.stack([raw[:, 0] / f32(100), raw[:, 1] / f32(120), raw[:, 2] / f32(120)], 1).astype(f32)
    return norm[inv.reshape(-1)]


# ---- one object's scores -----------------------------------------------------------------------------------------------------------
def scores(xyz, kp, leaf, geometry="none", color="none", max_similar_color_distance=0.01, pc=None, lab=None, kp_lab=None):
    """-> dict geo, color float32 [m], count int64 [m], distant int64 [m], undecided bool [m], geo64 / bound float64 [m] (curvature and kpq)
    xyz [n, 3] surface, kp [m, 3] keypoints (float32), pc: principal_curvatures(...) for kpq, lab [n, 3] / kp_lab [m, 3] for colordistance"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3); kp = np.asarray(kp, f32).reshape(-1, 3)
    fin = finite(xyz) if len(xyz) else np.zeros(0, bool)
    where = np.nonzero(fin)[0]
    p = xyz[fin]
    m = len(kp)
    out = dict(geo=np.zeros(m, f32), color=np.zeros(m, f32), count=np.zeros(m, np.int64), distant=np.zeros(m, np.int64),
               undecided=np.zeros(m, bool), geo64=np.zeros(m), bound=np.zeros(m))
    for k in range(m):
        nb = ball(p, kp[k], leaf)
        out["count"][k] = len(nb)
        out["undecided"][k] = near_boundary(p, kp[k], leaf) if np.isfinite(kp[k]).all() else False
        if geometry == "curvature":
            out["geo"][k], _, und = curvature(p, kp[k], leaf) if np.isfinite(kp[k]).all() else (NAN32, 0, False)
            out["undecided"][k] |= und
            if len(nb) >= 3:
                out["geo64"][k] = curvature64(p, kp[k], leaf)
                out["bound"][k] = curvature_bound(out["geo64"][k], curvature_trace(p, kp[k], leaf), leaf, len(p))
        elif geometry == "kpq":
            idx = where[nb]
            out["geo"][k] = kpq(pc["pc1"], pc["pc2"], idx)
            out["geo64"][k] = float(out["geo"][k])
            out["bound"][k] = kpq_bound(pc["pc1"], pc["pc2"], pc["pc1_64"], idx, pc["floor"], pc["bits"]) if not np.isnan(out["geo"][k]) else 0.0
        if color == "colordistance":
            out["color"][k], out["distant"][k] = color_score(kp_lab[k], lab[where[nb]], max_similar_color_distance)
    return out


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def ascending(v):
    """std::sort's order with NaN behind +inf and ties by index -> permutation"""
    v = np.asarray(v, f32)
    nan = np.isnan(v)
    return np.lexsort((np.arange(len(v)), nan, np.where(nan, np.inf, v.astype(np.float64))))


def cutoff_index(ratio, size):
    return min(int(f32(ratio) * f32(size)), size - 1)


def minmax(v):
    """first smallest / first largest of the non-NaN entries (std::min_element / max_element); none: +inf / -inf"""
    v = np.asarray(v, f32)
    ok = np.nonzero(~np.isnan(v))[0]
    if not len(ok):
        return f32(np.inf), f32(-np.inf)
    return v[ok[np.argmin(v[ok])]], v[ok[np.argmax(v[ok])]]


def combined(g, c):
    g, c = np.asarray(g, f32), np.asarray(c, f32)
    gmin, gmax = minmax(g); cmin, cmax = minmax(c)
    with np.errstate(all="ignore"):
        return (((g - gmin).astype(f32) / gmax).astype(f32) + ((c - cmin).astype(f32) / cmax).astype(f32)).astype(f32)


def select(g, c, geo_on=True, color_on=True, geo_type="cutoff", color_type="cutoff", geo_threshold=0.005, color_threshold=0.02, ratio=0.5,
           combine="RequireCombinedList"):
    """one object -> dict keep bool [n], thresholds float32 [3] (geometry, colour, combined), combined float32 [n]"""
    g, c = np.asarray(g, f32).reshape(-1), np.asarray(c, f32).reshape(-1)
    n = len(g)
    thr = np.full(3, FLT_MIN, f32)
    x = combined(g, c) if n else np.zeros(0, f32)
    if n:
        idx = cutoff_index(ratio, n)
        if geo_on and geo_type == "cutoff":
            thr[0] = g[ascending(g)[idx]]
        if color_on and color_type == "cutoff":
            thr[1] = c[ascending(c)[idx]]
        if geo_on and color_on and geo_type == "cutoff" and color_type == "cutoff":
            thr[2] = x[ascending(x)[idx]]
    if geo_on and geo_type == "threshold":
        thr[0] = f32(geo_threshold)
    if color_on and color_type == "threshold":
        thr[1] = f32(color_threshold)
    with np.errstate(invalid="ignore"):
        geo_passed = ~(g < thr[0]) if geo_on else np.ones(n, bool)
        color_passed = ~(c < thr[1]) if color_on else np.ones(n, bool)
        combined_passed = ~(x < thr[2])
    if geo_on and color_on:
        keep = {"RequireOne": geo_passed | color_passed, "RequireBoth": geo_passed & color_passed, "RequireCombinedList": combined_passed}[combine]
    else:
        keep = geo_passed & color_passed
    return dict(keep=keep, thresholds=thr, combined=x)

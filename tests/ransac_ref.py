"""CPU restatement (numpy, float64) of the RANSAC vote filter, DESIGN.md §4.6: what ismhip_ransac_filter and the RANSAC variants of the
maxima kernels compute for ONE cluster of votes. PCL is external, so the draws, the three-point model and the scoring are this
library's own definitions; the sequential loop of pcl::SampleConsensus is the contract. The model here goes through numpy.linalg.svd
(the library: a one-sided Jacobi SVD), everything else is written in the library's order of operations."""
import math

import numpy as np

M64 = (1 << 64) - 1
MAX_SAMPLE_CHECKS = 1000
DBL_EPS = float(np.finfo(np.float64).eps)


def splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(seed, i, t, n):
    """the three distinct indices of attempt t of hypothesis i: a pure function of (seed, i, t, n)"""
    base = (i << 20) | (t << 2)
    r0, r1, r2 = (splitmix(seed ^ splitmix(base | j)) for j in range(3))
    a = r0 % n; b = r1 % (n - 1); c = r2 % (n - 2)
    if b >= a:
        b += 1
    lo, hi = (a, b) if a < b else (b, a)
    if c >= lo:
        c += 1
    if c >= hi:
        c += 1
    return a, b, c


def sample_distance_threshold(S):
    """PCL computeSampleDistanceThreshold: ((sqrt l0 + sqrt l1 + sqrt l2) / 3)^2 of the covariance of S (about its centroid, / n)"""
    d = S - S.mean(0)
    ev = np.clip(np.linalg.eigvalsh(d.T @ d / len(S)), 0.0, None)
    q = np.sqrt(ev).sum() / 3.0
    return q * q


def rigid3(S3, T3):
    """least-squares rigid motion of three pairs (Umeyama without scale) -> (R, t) or None for a degenerate sample
    (second singular value of the cross-covariance <= 1e-12 of the first: collinear points or images)"""
    cs = ((S3[0] + S3[1]) + S3[2]) / 3.0
    ct = ((T3[0] + T3[1]) + T3[2]) / 3.0
    Sc, Tc = S3 - cs, T3 - ct
    H = (np.outer(Tc[0], Sc[0]) + np.outer(Tc[1], Sc[1])) + np.outer(Tc[2], Sc[2])
    U, D, Vt = np.linalg.svd(H)
    if not D[1] > 1e-12 * D[0]:
        return None
    s = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        s[2] = -1.0
    R = U @ np.diag(s) @ Vt
    t = ct - ((R[:, 0] * cs[0] + R[:, 1] * cs[1]) + R[:, 2] * cs[2])
    return R, t


def residuals2(R, t, S, T):
    """d^2 of every vote in the library's order: ((R0.S + R1.S) + R2.S + t) - T, then (dx^2 + dy^2) + dz^2"""
    d = [(((R[r, 0] * S[:, 0] + R[r, 1] * S[:, 1]) + R[r, 2] * S[:, 2]) + t[r]) - T[:, r] for r in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def find_sample(S, seed, i, sdt, fragile=None, beta=0.0):
    n = len(S)
    for t in range(MAX_SAMPLE_CHECKS):
        a, b, c = draw(seed, i, t, n)
        dd = [float(((S[q] - S[p]) ** 2).sum()) for p, q in ((a, b), (a, c), (b, c))]
        if fragile is not None and any(abs(v - sdt) <= beta * max(sdt, 1e-300) for v in dd):
            fragile[0] = True
        if all(v > sdt for v in dd):
            return [a, b, c]
    return None


def hypothesis(S, T, thr, seed, i):
    """one hypothesis, as ismhip_ransac_hypothesis reports it: dict(valid, R, t, d2, mask) (valid False: no good sample)"""
    S = np.asarray(S, np.float64); T = np.asarray(T, np.float64)
    sel = find_sample(S, seed, i, sample_distance_threshold(S))
    if sel is None:
        return dict(valid=False)
    m = rigid3(S[sel], T[sel])
    if m is None:
        return dict(valid=True, degenerate=True, d2=None, mask=np.zeros(len(S), bool))
    thr2 = float(np.float32(thr)) * float(np.float32(thr))
    d2 = residuals2(m[0], m[1], S, T)
    return dict(valid=True, degenerate=False, R=m[0], t=m[1], d2=d2, mask=d2 < thr2, sample=sel)


def stopping_k(count, n):
    """k of PCL's loop after a new best count"""
    w = count / n
    p = min(max(1.0 - w * w * w, DBL_EPS), 1.0 - DBL_EPS)
    return math.log(1.0 - 0.99) / math.log(p)


def sequential_stop(counts, n, max_iterations):
    """PCL's loop over a given sequence of inlier counts (None = no good sample) -> (best, best_i, iterations)"""
    k, best, best_i, i = 1.0, -1, -1, 0
    while i < k and i <= max_iterations:
        c = counts[i]
        if c is None:
            break
        if c > best:
            best, best_i = c, i
            k = stopping_k(c, n)
        i += 1
    return best, best_i, i


def is_identity(R, t, prec=1e-4):
    """Eigen isIdentity(prec) on the float-rounded 4x4"""
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = R.astype(np.float32); M[:3, 3] = t.astype(np.float32)
    prec = np.float32(prec)
    for r in range(4):
        for c in range(4):
            m = M[r, c]
            if r == c:
                if not abs(m - np.float32(1)) <= prec * min(abs(m), np.float32(1)):
                    return False
            elif not abs(m) <= prec:
                return False
    return True


def ransac(S, T, thr, seed=12345, max_iterations=10000, beta=0.0):
    """-> dict(kept, mask [n] bool, n_inliers, best_i, iterations, R, t, fragile, evaluated). fragile: some evaluated hypothesis had a
    d^2 within relative beta of thr^2 (or a sample distance within beta of its threshold): one rounding could change the result."""
    S = np.asarray(S, np.float64); T = np.asarray(T, np.float64)
    n = len(S)
    out = dict(kept=False, mask=np.zeros(n, bool), n_inliers=0, best_i=-1, iterations=0, R=np.eye(3), t=np.zeros(3), fragile=False, evaluated=0)
    thr = float(np.float32(thr))
    if n < 3 or not thr > 0 or max_iterations < 0:
        return out
    thr2 = thr * thr
    sdt = sample_distance_threshold(S)
    k, best, best_i, i = 1.0, -1, -1, 0
    frag = [False]
    best_model = None
    while i < k and i <= max_iterations:
        sel = find_sample(S, seed, i, sdt, frag, beta)
        if sel is None:
            break
        m = rigid3(S[sel], T[sel])
        if m is None:
            c = 0; d2 = None
        else:
            d2 = residuals2(m[0], m[1], S, T)
            if (np.abs(d2 - thr2) <= beta * thr2).any():
                frag[0] = True
            c = int((d2 < thr2).sum())
        out["evaluated"] += 1
        if c > best:
            best, best_i, best_model = c, i, (m, d2)
            k = stopping_k(c, n)
        i += 1
    out.update(best_i=best_i, iterations=i, fragile=frag[0])
    if best_i < 0 or best < 3:
        return out
    (R, t), d2 = best_model
    out.update(R=R, t=t)
    if is_identity(R, t):
        return out
    out.update(kept=True, mask=d2 < thr2, n_inliers=best)
    return out

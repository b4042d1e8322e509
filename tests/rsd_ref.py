"""The RSD descriptor (ismhip_rsd) restated in numpy, brute force, one object at a time. float32 exactly where the
definition says float32 (the neighbour predicate, the dot product c of two normals, the squared distance d2 of two points, a = min(|c|, 1));
float64 elsewhere (acos, sqrt, the bin coordinates, the radii fit).

A pair is UNDECIDED when a bin coordinate, 5 * dist / D or 5 * theta / (pi / 2), lies within EDGE_EPS = 1e-9 of an integer edge: the
edges 1..4 of the angle, the edges 1..4 of the distance and 5, the boundary dist > D beyond which the pair is neglected. The double acos
and sqrt of two libraries differ by a few 1e-16 relative and the coordinates are below 5, so 1e-9 is a derived margin, far outside what
the libraries can disagree on, not a measured one. Undecided pairs widen the counts of the bins they may fall into to intervals [lo, hi];
every other count is decided and is compared bit for bit. In radii mode a keypoint with an undecided pair is left out (`radii_ok`)."""
import numpy as np

import normals_ref as nr

f32, f64 = np.float32, np.float64
SUB = 5
DIM, RADII_DIM = 25, 2
EDGE_EPS = 1e-9
NORM = f32(300.0)            # features.cpp:282-297 divides by the sum of the indices 0..24


def pair_terms(P, N, idx):
    """all unordered pairs of the cloud indices idx -> (a float32, d2 float32, finite mask)"""
    i, j = np.triu_indices(len(idx), 1)
    pi, pj, ni, nj = P[idx[i]], P[idx[j]], N[idx[i]], N[idx[j]]
    with np.errstate(invalid="ignore", over="ignore"):
        c = ((ni[:, 0] * nj[:, 0]).astype(f32) + (ni[:, 1] * nj[:, 1]).astype(f32)).astype(f32)
        c = (c + (ni[:, 2] * nj[:, 2]).astype(f32)).astype(f32)
        d2 = nr.sqdist3(pi, pj) if len(i) else np.zeros(0, f32)
        a = np.minimum(np.abs(c), f32(1.0)).astype(f32)
    return a, d2, np.isfinite(c) & np.isfinite(d2)


def bin_coordinates(a, d2, radius):
    """-> (ta, td) float64: 5 * theta / (pi / 2) and 5 * dist / D"""
    D = f64(f32(radius))
    theta = np.arccos(a.astype(f64))
    dist = np.sqrt(d2.astype(f64))
    return 5.0 * theta / (np.pi / 2), 5.0 * dist / D, dist, D


def _near(t, edges):
    r = np.rint(t)
    return (np.abs(t - r) <= EDGE_EPS) & np.isin(r, edges)


def radii_of(amin, amax, present, radius):
    """the two radii from the extremal a of every distance bin (float32 [5] each; present [5] bool: the bin has a pair)"""
    D = f64(f32(radius))
    amin, amax, present = amin.copy(), amax.copy(), present.copy()
    # bin 0 starts at theta_min = theta_max = 0: a = 1 takes part in its extremes
    amin[0] = min(amin[0], f32(1.0)) if present[0] else f32(1.0)
    amax[0] = max(amax[0], f32(1.0)) if present[0] else f32(1.0)
    present[0] = True
    Amin2 = Amind = Amax2 = Amaxd = f64(0.0)
    for d in range(SUB):
        if not present[d]:
            continue
        tmin, tmax = np.arccos(f64(amax[d])), np.arccos(f64(amin[d]))
        f = (f64(d) + 0.5) * D / 5.0
        Amin2 += tmin * tmin; Amind += tmin * f
        Amax2 += tmax * tmax; Amaxd += tmax * f
    r0 = f32(D) if Amin2 == 0 else f32(min(Amind / Amin2, D))
    r1 = f32(D) if Amax2 == 0 else f32(min(Amaxd / Amax2, D))
    r0, r1 = f32(r0 * f32(1.1)), f32(r1 * f32(1.1))
    return np.array([min(r0, r1), max(r0, r1)], f32)


def rsd_keypoint(P, N, q, radius):
    """one keypoint q on the object (P, N) -> dict(n, pairs, skipped, neglected (decided), undecided, lo [25], hi [25] (counts),
    neg_hi (neglected at most), radii [2] float32, radii_ok)"""
    P, N, q = np.asarray(P, f32), np.asarray(N, f32), np.asarray(q, f32)
    out = dict(n=0, pairs=0, skipped=0, neglected=0, neg_hi=0, undecided=0, lo=np.zeros(DIM, np.int64), hi=np.zeros(DIM, np.int64),
               radii=np.full(2, np.nan, f32), radii_ok=True, valid=False)
    if not np.isfinite(q).all() or len(P) == 0:
        return out
    idx = np.flatnonzero(nr.neighbour_mask(P, q[None, :], radius)[0])
    n = len(idx)
    out["n"] = n
    if n == 0:
        return out
    out["valid"] = True
    if n == 1:
        out["radii"] = np.zeros(2, f32)
        return out
    a, d2, fin = pair_terms(P, N, idx)
    out["pairs"] = len(a)
    out["skipped"] = int((~fin).sum())
    a, d2 = a[fin], d2[fin]
    ta, td, dist, D = bin_coordinates(a, d2, radius)
    ua, ud = _near(ta, [1, 2, 3, 4]), _near(td, [1, 2, 3, 4, 5])
    und = ua | ud
    ba = np.minimum(SUB - 1, np.floor(ta)).astype(np.int64)
    bd = np.where(dist > D, SUB, np.minimum(SUB - 1, np.floor(td))).astype(np.int64)
    dec = ~und
    keep = dec & (bd < SUB)
    lo = np.bincount((ba + SUB * bd)[keep], minlength=DIM).astype(np.int64)
    hi = lo.copy()
    neg_hi = int((dec & (bd == SUB)).sum())
    out["neglected"] = neg_hi
    for k in np.flatnonzero(und):
        r_a, r_d = int(np.rint(ta[k])), int(np.rint(td[k]))
        cand_a = {min(SUB - 1, r_a - 1), min(SUB - 1, r_a)} if ua[k] else {int(ba[k])}
        cand_d = {r_d - 1, r_d if r_d < SUB else SUB} if ud[k] else {int(bd[k])}      # at the edge 5: bin 4 or neglected
        if SUB in cand_d:
            neg_hi += 1
        for x in cand_a:
            for y in cand_d:
                if y < SUB:
                    hi[x + SUB * y] += 1
    out.update(lo=lo, hi=hi, neg_hi=neg_hi, undecided=int(und.sum()))
    out["radii_ok"] = not und.any()
    if out["radii_ok"]:
        amin, amax, present = np.ones(SUB, f32), np.zeros(SUB, f32), np.zeros(SUB, bool)
        for d in range(SUB):
            m = bd == d
            if m.any():
                amin[d], amax[d], present[d] = a[m].min(), a[m].max(), True
        out["radii"] = radii_of(amin, amax, present, radius)
    return out


def rsd(pt_off, xyz, normals, kp_off, kp, radius):
    """the batch -> dict of arrays over the keypoints: cnt [K], pairs, skipped, neglected, neg_hi, undecided [K]; lo, hi [K, 25] counts;
    row_lo, row_hi [K, 25] float32 (the histogram rows at the two ends; NaN rows where the definition says NaN); radii [K, 2] float32;
    radii_ok [K] bool"""
    K = int(kp_off[-1])
    res = dict(cnt=np.zeros(K, np.int64), pairs=np.zeros(K, np.int64), skipped=np.zeros(K, np.int64), neglected=np.zeros(K, np.int64),
               neg_hi=np.zeros(K, np.int64), undecided=np.zeros(K, np.int64), lo=np.zeros((K, DIM), np.int64), hi=np.zeros((K, DIM), np.int64),
               radii=np.full((K, 2), np.nan, f32), radii_ok=np.ones(K, bool), valid=np.zeros(K, bool))
    for o in range(len(pt_off) - 1):
        P, N = xyz[int(pt_off[o]):int(pt_off[o + 1])], normals[int(pt_off[o]):int(pt_off[o + 1])]
        for k in range(int(kp_off[o]), int(kp_off[o + 1])):
            r = rsd_keypoint(P, N, kp[k], radius)
            res["cnt"][k] = r["n"]
            for key in ("pairs", "skipped", "neglected", "neg_hi", "undecided", "lo", "hi", "radii", "radii_ok", "valid"):
                res[key][k] = r[key]
    res["row_lo"] = (res["lo"].astype(f32) / NORM).astype(f32)
    res["row_hi"] = (res["hi"].astype(f32) / NORM).astype(f32)
    res["row_lo"][~res["valid"]] = np.nan
    res["row_hi"][~res["valid"]] = np.nan
    return res

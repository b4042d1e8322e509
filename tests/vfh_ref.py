"""The VFH region descriptor (ismhip_global_vfh, include/ismhip.h) restated in float64, numpy only, from the header's text: the pair
(centroid c, normal centroid nc) against every selected point p with a finite normal n by pcl::computePairFeatures, four 45-bin blocks
(f1, f2, f3, distance) and a 128-bin viewpoint block of INTEGER counts, then one product per bin.

Inputs are the selected points and normals and the DEVICE's c, nc and viewpoint (c and nc are outputs of the same call, held to their own
checks). The device evaluates each pair in float32 (pair_features.h); float32 in another libm, or here in float64, may land in another
bin when a raw bin coordinate is close to an integer. So the counts come as an INTERVAL: a deposit is UNDECIDED, and counts in `upper`
only, in every bin it could reach, when
  edge      a raw bin coordinate t lies within its margin of an integer at which the bin changes (1 .. 44; 1 .. 127 for the viewpoint);
  swap      the role swap of computePairFeatures is inside pair_features.h's own band, ||a1| - |a2|| <= SWAP: both role assignments'
            bins are candidates;
  pole      (x, y) of the arctangent is too short for its size: all 45 bins of f1;
  degenerate  f4 is within the margin of 0 (in raw units, hundredths) or the cross product d x u is within DEG of 0 relative to
            |d| |u|: the pair may or may not be rejected, and if it is kept f1 and f2 are noise.
MARGIN = 1e-4 raw bin units: a numpy float32 transcription (pairs32 below, pair_features.h's written order) against float64 differs by at
most 2.4e-5 in t1 and 1.2e-5 in the others on blobs and shells of 1 000 and 16 384 points; test_vfh_cpu.py measures it on every scene
of vfh_scenes.py and requires that the two never disagree outside the margin.
The margins of t1 and t2 GROW where the pair is ill conditioned (reasoned as in fpfh_ref.py, ERR = 4 * 2^-24 the absolute error of a
sum of three float32 products of magnitude <= 1): the direction of v = d x u moves by ERR / sin, sin = |d x u| / (|d| |u|), which is
45 / 2 of that in t2 and 45 / 2 pi in t1; the direction of (x, y) moves by ERR * |u| |n_t| / |(x, y)|, 45 / 2 pi of that in t1. Where
those exceed MARGIN they take its place; below |(x, y)| = POLE * |u| |n_t| f1 is undecided altogether."""
import numpy as np

f32, f64 = np.float32, np.float64
DIM, SHAPE_BINS, VP_BINS = 308, 45, 128
MARGIN = 1e-4
SWAP = 1.2e-5                 # pair_features.h's band of 1e-5 plus the float32 error of the two cosines
ERR = 4 * 2.0 ** -24
POLE = 2.0 ** -6
DEG = 2.0 ** -10
ALL45 = (1 << SHAPE_BINS) - 1
D_PI = f64(f32(1.0) / (f32(2.0) * f32(np.pi)))


def _dot(a, b):
    return (a * b).sum(-1)


def view_direction(c, viewpoint):
    """d = viewpoint - c in float32, divided by its float32 norm; a zero norm leaves d = 0"""
    d = (np.asarray(viewpoint, f32) - np.asarray(c, f32)).astype(f32)
    n = f32(np.sqrt(f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
    return d if n == 0 else (d / n).astype(f32)


def _bit(t):
    return np.left_shift(np.int64(1), np.clip(np.floor(t), 0, SHAPE_BINS - 1).astype(np.int64))


def _edge_mask(t, margin):
    """candidate bins of a raw coordinate: its own, and the neighbour across an integer 1 .. 44 closer than the margin"""
    r = np.rint(t)
    near = (np.abs(t - r) <= margin) & (r >= 1) & (r <= SHAPE_BINS - 1)
    ri = np.clip(r, 1, SHAPE_BINS - 1).astype(np.int64)
    both = np.left_shift(np.int64(1), ri) | np.left_shift(np.int64(1), ri - 1)
    return np.where(near, both, _bit(t))


def _role(d, dn, u, nt, margin):
    """one role assignment (source normal u at the source, target normal nt, d from source to target) in float64
    -> dict(t [k, 3], masks [k, 3], deg [k], pole [k])"""
    with np.errstate(invalid="ignore", divide="ignore"):
        cr = np.cross(d, u)
        crn = np.linalg.norm(cr, axis=-1)
        v = cr / crn[:, None]
        w = np.cross(u, v)
        x, y = _dot(u, nt), _dot(w, nt)
        f1, f2, f3 = np.arctan2(y, x), _dot(v, nt), _dot(u, d) / dn
        un, ntn = np.linalg.norm(u, axis=-1), np.linalg.norm(nt, axis=-1)
        sin = crn / (dn * un)
        hyp = np.hypot(x, y) / (un * ntn)
    deg = ~(sin >= DEG)
    pole = ~deg & ~(hyp >= POLE)
    t = np.stack([SHAPE_BINS * ((f1 + np.pi) * D_PI), SHAPE_BINS * ((f2 + 1.0) * 0.5), SHAPE_BINS * ((f3 + 1.0) * 0.5)], 1)
    t = np.where(np.isfinite(t), t, 0.0)
    s = np.maximum(sin, DEG)
    m2 = np.maximum(margin, (SHAPE_BINS / 2.0) * ERR / s)
    m1 = np.maximum(margin, (SHAPE_BINS / (2 * np.pi)) * ERR * (1.0 / s + 1.0 / np.maximum(hyp, POLE)))
    masks = np.stack([_edge_mask(t[:, 0], m1), _edge_mask(t[:, 1], m2), _edge_mask(t[:, 2], np.full_like(m1, margin))], 1)
    masks[:, 0] = np.where(pole, ALL45, masks[:, 0])
    masks[deg, :2] = ALL45
    return dict(t=t, masks=masks, deg=deg, pole=pole)


def pairs64(P, N, c, nc, margin=MARGIN):
    """computePairFeatures(c, nc, p, n) for every row of P / N in float64 from the float32 inputs -> dict of per-point arrays:
    reject (f4 == 0: decided), maybe (the pair may or may not be rejected), swap, tie, gap, t [k, 4] (face-value raw coordinates),
    masks [k, 4] (candidate bins of the four shape blocks as bit masks)"""
    P64, N64 = np.asarray(P, f32).astype(f64).reshape(-1, 3), np.asarray(N, f32).astype(f64).reshape(-1, 3)
    c64, nc64 = np.asarray(c, f32).astype(f64), np.asarray(nc, f32).astype(f64)
    k = len(P64)
    d = P64 - c64[None, :]
    dn = np.linalg.norm(d, axis=1)
    reject = dn == 0
    dn_ = np.where(reject, 1.0, dn)
    ncs = np.broadcast_to(nc64, (k, 3))
    with np.errstate(invalid="ignore"):
        a1, a2 = _dot(ncs, d) / dn_, _dot(N64, d) / dn_
    gap = np.abs(a1) - np.abs(a2)
    swap = gap < 0
    tie = np.abs(gap) <= SWAP
    A = _role(d, dn_, ncs, N64, margin)                       # source: the centroid with nc
    B = _role(-d, dn_, N64, ncs, margin)                      # roles swapped: source p with n
    sw = swap[:, None]
    own, other = np.where(sw, B["masks"], A["masks"]), np.where(sw, A["masks"], B["masks"])
    m3 = np.where(tie[:, None], own | other, own)
    t4 = dn * 100.0 + 0.5
    m4 = _edge_mask(t4, np.full(k, margin))
    maybe = ~reject & ((dn * 100.0 < margin) | np.where(swap, B["deg"], A["deg"]) | (tie & (A["deg"] | B["deg"])))
    t = np.concatenate([np.where(sw, B["t"], A["t"]), t4[:, None]], 1)
    return dict(reject=reject, maybe=maybe, swap=swap, tie=tie, gap=gap, t=t, masks=np.concatenate([m3, m4[:, None]], 1))


def pairs32(P, N, c, nc):
    """the same pairs in float32, every operation rounded, in pair_features.h's written order (numpy's arccos / arctan2 stand for
    acosf / atan2f) -> dict(reject, bins [k, 4] by the header's double bin formulas (-1: a NaN feature), t [k, 4])"""
    P, N = np.asarray(P, f32).reshape(-1, 3), np.asarray(N, f32).reshape(-1, 3)
    c, nc = np.asarray(c, f32), np.asarray(nc, f32)
    k = len(P)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dp = P - c[None, :]
        f4 = np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2])
        a, b = np.broadcast_to(nc, (k, 3)).copy(), N.copy()
        angle1 = ((a[:, 0] * dp[:, 0] + a[:, 1] * dp[:, 1]) + a[:, 2] * dp[:, 2]) / f4
        angle2 = ((b[:, 0] * dp[:, 0] + b[:, 1] * dp[:, 1]) + b[:, 2] * dp[:, 2]) / f4
        c1, c2 = np.abs(angle1), np.abs(angle2)
        gap = c2 - c1
        swap = np.where(np.abs(gap) > f32(1e-5), gap > 0, np.arccos(c1) > np.arccos(c2))
        sw = swap[:, None]
        a, b = np.where(sw, b, a), np.where(sw, a, b)
        dp = np.where(sw, -dp, dp)
        f3 = np.where(swap, -angle2, angle1)
        v = np.stack([dp[:, 1] * a[:, 2] - dp[:, 2] * a[:, 1], dp[:, 2] * a[:, 0] - dp[:, 0] * a[:, 2], dp[:, 0] * a[:, 1] - dp[:, 1] * a[:, 0]], 1)
        vn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        v = v / vn[:, None]
        w = np.stack([a[:, 1] * v[:, 2] - a[:, 2] * v[:, 1], a[:, 2] * v[:, 0] - a[:, 0] * v[:, 2], a[:, 0] * v[:, 1] - a[:, 1] * v[:, 0]], 1)
        f2 = (v[:, 0] * b[:, 0] + v[:, 1] * b[:, 1]) + v[:, 2] * b[:, 2]
        y = (w[:, 0] * b[:, 0] + w[:, 1] * b[:, 1]) + w[:, 2] * b[:, 2]
        x = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        f1 = np.arctan2(y, x)
        f4h = f4 * f32(100.0)
    assert f1.dtype == f32 and f2.dtype == f32 and f3.dtype == f32 and f4h.dtype == f32
    t = np.stack([SHAPE_BINS * ((f1.astype(f64) + np.pi) * D_PI), SHAPE_BINS * ((f2.astype(f64) + 1.0) * 0.5),
                  SHAPE_BINS * ((f3.astype(f64) + 1.0) * 0.5), f4h.astype(f64) + 0.5], 1)
    with np.errstate(invalid="ignore"):
        bins = np.where(np.isnan(t), -1, np.clip(np.floor(np.where(np.isnan(t), 0.0, t)), 0, SHAPE_BINS - 1)).astype(np.int64)
    return dict(reject=(f4 == 0) | (vn == 0), bins=bins, t=t, swap=swap)


def viewpoint64(N, d, margin=MARGIN):
    """raw viewpoint coordinate ((n . d + 1) / 2) * 128 in float64 from the float32 normals and view direction -> (t, bin, undecided)"""
    t = ((_dot(np.asarray(N, f32).astype(f64).reshape(-1, 3), np.asarray(d, f32).astype(f64)[None, :]) + 1.0) * 0.5) * VP_BINS
    r = np.rint(t)
    und = (np.abs(t - r) <= margin) & (r >= 1) & (r <= VP_BINS - 1)
    if not np.asarray(d, f32).any():                           # d = 0: every product is an exact zero in any precision, raw 64 exactly
        und[:] = False
    return t, np.clip(np.floor(t), 0, VP_BINS - 1).astype(np.int64), und


def viewpoint32(N, d):
    """the device's float32 dot product (unfused, in order) and the double bin formula"""
    N, d = np.asarray(N, f32).reshape(-1, 3), np.asarray(d, f32)
    dv = ((N[:, 0] * d[0] + N[:, 1] * d[1]).astype(f32) + N[:, 2] * d[2]).astype(f32)
    return np.clip(np.floor(((dv.astype(f64) + 1.0) * 0.5) * VP_BINS), 0, VP_BINS - 1).astype(np.int64)


def finite_normals(P, N):
    P, N = np.asarray(P, f32).reshape(-1, 3), np.asarray(N, f32).reshape(-1, 3)
    ok = np.isfinite(N).all(1)
    return P[ok], N[ok]


def normal_centroid(N):
    """float64 mean of the finite normals, cast to float32 (NaN for none) and their number m"""
    N = np.asarray(N, f32).reshape(-1, 3)
    N = N[np.isfinite(N).all(1)]
    if len(N) == 0:
        return np.full(3, np.nan, f32), 0
    return (N.astype(f64).sum(0) / f64(len(N))).astype(f32), len(N)


def vfh_counts(P, N, c, nc, viewpoint=(0, 0, 0), margin=MARGIN):
    """One region: P / N the selected points and their normals (any of them non-finite normals), c / nc the centroid and normal centroid
    -> dict(counts, lower, upper [308] int64; m; undecided: depositing points with an undecided deposit; shape_undecided / vp_undecided;
    total_lower / total_upper [5]: per block). counts takes every float64 decision at face value."""
    P, N = finite_normals(P, N)
    m = len(P)
    counts, lower, upper = (np.zeros(DIM, np.int64) for _ in range(3))
    out = dict(counts=counts, lower=lower, upper=upper, m=m, undecided=0, shape_undecided=0, vp_undecided=0,
               total_lower=np.zeros(5, np.int64), total_upper=np.zeros(5, np.int64))
    if m < 2:
        return out
    pr = pairs64(P, N, c, nc, margin)
    live = ~pr["reject"]
    single = (pr["masks"] & (pr["masks"] - 1)) == 0
    und_pt = np.zeros(m, bool)
    for blk in range(4):
        mk = pr["masks"][:, blk]
        face = np.clip(np.floor(pr["t"][:, blk]), 0, SHAPE_BINS - 1).astype(np.int64)
        counts[blk * SHAPE_BINS:(blk + 1) * SHAPE_BINS] = np.bincount(face[live], minlength=SHAPE_BINS)
        decided = live & single[:, blk] & ~pr["maybe"]
        und_pt |= live & ~decided
        for b in range(SHAPE_BINS):
            has = live & ((mk >> b) & 1).astype(bool)
            lower[blk * SHAPE_BINS + b] = int((has & decided).sum())
            upper[blk * SHAPE_BINS + b] = int(has.sum())
        out["total_lower"][blk] = int(decided.sum())
        out["total_upper"][blk] = int(live.sum())
    out["shape_undecided"] = int(und_pt.sum())
    d = view_direction(c, viewpoint)
    t, vb, vund = viewpoint64(N, d, margin)
    o = 4 * SHAPE_BINS
    counts[o:] = np.bincount(vb, minlength=VP_BINS)
    lower[o:] = np.bincount(vb[~vund], minlength=VP_BINS)
    upper[o:] = lower[o:]
    for i in np.nonzero(vund)[0]:
        r = int(np.rint(t[i]))
        upper[o + r] += 1
        upper[o + r - 1] += 1
    out["total_lower"][4] = out["total_upper"][4] = m          # every point with a finite normal deposits exactly once
    out["vp_undecided"] = int(vund.sum())
    out["undecided"] = int((und_pt | vund).sum())
    return out


def row_of_counts(counts, m, fill_size_component=False):
    """blocks f1 .. f3 (and f4 with the flag): float32(float64(count) * float64(incr)), incr = 100.0f / float32(m - 1) in float32; block
    f4 zeros otherwise; viewpoint float32(float64(count) * float64(float32(100.0 / m))); m < 2: NaN"""
    counts = np.asarray(counts, f64)
    if m < 2:
        return np.full(DIM, np.nan, f32)
    incr = f64(f32(100.0) / f32(m - 1))
    vp = f64(f32(100.0 / f64(m)))
    row = np.zeros(DIM, f32)
    o = 4 * SHAPE_BINS
    row[:o] = (counts[:o] * incr).astype(f32)
    if not fill_size_component:
        row[3 * SHAPE_BINS:o] = 0
    row[o:] = (counts[o:] * vp).astype(f32)
    return row


def disagreements(P, N, c, nc, viewpoint=(0, 0, 0), margin=MARGIN):
    """float32 transcription against the float64 intervals over one region -> dict(outside: deposits where float32 lands outside the
    float64 candidate set or rejects / keeps a pair float64 is sure about; worst [5]: the largest |t32 - t64| per block over the pairs
    both keep with the same roles; pairs)"""
    P, N = finite_normals(P, N)
    a, b = pairs64(P, N, c, nc, margin), pairs32(P, N, c, nc)
    sure_keep, sure_rej = ~a["reject"] & ~a["maybe"], a["reject"]
    outside = int((sure_keep & b["reject"]).sum() + (sure_rej & ~b["reject"]).sum())
    both = ~a["reject"] & ~b["reject"]
    for blk in range(4):
        ok = b["bins"][:, blk] >= 0
        hit = ((a["masks"][:, blk] >> np.where(ok, b["bins"][:, blk], 0)) & 1).astype(bool) & ok
        outside += int((both & ~hit).sum())
    same = both & ~a["maybe"] & (a["swap"] == b["swap"])
    dt = np.abs(a["t"] - b["t"])
    dt[:, 0] = np.minimum(dt[:, 0], SHAPE_BINS - dt[:, 0])                 # across the seam t1 = 0 and t1 = 45 are one angle
    worst = [float(dt[same & (a["masks"][:, 0] != ALL45), 0].max(initial=0.0))] + [float(dt[same, j].max(initial=0.0)) for j in (1, 2, 3)]
    d = view_direction(c, viewpoint)
    t, vb, vund = viewpoint64(N, d, margin)
    v32 = viewpoint32(N, d)
    outside += int(((v32 != vb) & ~vund).sum())
    N32 = np.asarray(N, f32)
    dv = ((N32[:, 0] * d[0] + N32[:, 1] * d[1]).astype(f32) + N32[:, 2] * d[2]).astype(f32)
    worst.append(float(np.abs(((dv.astype(f64) + 1.0) * 0.5) * VP_BINS - t).max(initial=0.0)))
    return dict(outside=outside, worst=worst, pairs=int(both.sum()))

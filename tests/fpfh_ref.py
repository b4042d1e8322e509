"""FPFH-33 in float64, brute force (numpy only), written from SURVEY Appendix A.4 (PCL computePairFeatures,
computePointSPFHSignature, weightPointSPFHSignature): one object at a time, no grid, no float sums, no fast arithmetic.

Neighbourhood: the library's decision, bit for bit in float32 (normals_ref.sqdist3 / r2_of): d2 = (dx*dx + dy*dy) + dz*dz on the
float32 differences, neighbour iff d2 < r2 = float32(float64(float32(radius))^2). No neighbour or a non-finite keypoint -> NaN row.

Pair (source p, neighbour q != p by index), everything in float64 from the float32 inputs: identical coordinates -> skipped;
d = q - p, cos1 = n_p . d / |d|, cos2 = n_q . d / |d|; |cos2| > |cos1| -> the roles swap (source q, target p, d = -d);
u = n_s, v = d x u / |d x u|, w = u x v; x = u . n_t, y = w . n_t; f1 = atan2(y, x), f2 = v . n_t, f3 = u . d / |d|;
t1 = 11 (f1 + pi) / 2 pi, t2 = 11 (f2 + 1) / 2, t3 = 11 (f3 + 1) / 2; bin = clamp(floor(t), 0, 10).
SPFH(p) adds 100 / (n_p - 1) per deposited pair and feature (n_p = in-ball count with p; alone -> zeros).
FPFH(k) = sum over neighbours with d2 != 0 of SPFH(nb) / d2, every 11-bin block rescaled to sum 100 (a zero block stays zero).

A deposit is UNDECIDED when float32 arithmetic in another operation order may land elsewhere; then the candidate bins are recorded:
  edge        t within EDGE of one of the integers 1..10 (t1, t2: within
              max(EDGE, 5.5 ERR / sin), see below)                        -> the two adjacent bins
  seam        f1: x < 0 and |y| < SEAM * hypot(x, y)                      -> bins 0 and 10
  swap tie    ||cos1| - |cos2|| < SWAP                                    -> the bins of both role assignments (each with its own
                                                                             edge / seam / pole candidates); the same single bin
                                                                             from both -> decided
  pole        f1: hypot(x, y) < POLE                                      -> all 11 bins of the f1 block
  degenerate  |d x n_s| / |d| < DEG                                       -> the pair may or may not be skipped: the block total
                                                                             changes, every keypoint it touches is `exempt`
Every other pair deposits exactly one count per block whichever bin it takes, so the block total S is decided and only the
numerators are intervals: lo counts the decided deposits of a bin, hi adds every undecided deposit that has the bin as candidate.

Margins. pairs32() recomputes every pair in float32 in the CPU oracle's written operation order (oracle/ism_oracle.cpp::
pair_features, double bin formulas on the float32 features); measure() compares it with the float64 values over the pairs of a
scene. Largest values over all scenes of fpfh_scenes.py (54 000 pairs; test_fpfh_cpu.py::test_margins_are_four_times_the_measured_
error prints them per scene and asserts that each constant is >= 4 x and <= 8 x its measured maximum):
  max |t_float32 - t_float64|  (non-degenerate pairs, f1 away from the pole)    MEASURED_T    = 2.72e-6 (generic)  x 4 = 1.09e-5
  max |y/hypot (float32) - y/hypot (float64)|   (same pairs)                    MEASURED_SEAM = 1.43e-6 (generic)  -> SEAM = 5.8e-6
  max |(|cos1| - |cos2|) float32 - float64|                                     MEASURED_SWAP = 2.14e-7 (generic)  -> SWAP = 8.6e-7
The oracle is ONE float32 evaluation order; the device's exact path is the same order, and its fast path documents a difference of
< 2e-5 in t from it. The margin must cover that too, and 4 x MEASURED_T does not: EDGE = 2e-5, the larger of the two
(test_fpfh_cpu.py asserts EDGE >= 2e-5).
POLE, DEG and ERR are not measured but reasoned. x, y and the components of d x n_s / |d| are sums of two or three products of
float32 numbers of magnitude <= 1 and carry an absolute error of a few 2^-24: ERR = 4 * 2^-24 = 2.4e-7.
  pole        the direction of (x, y) moves by <= ERR / hypot rad, 11 / 2 pi of that in t1: 1.3e-5 at hypot = POLE = 2^-5, still inside
              EDGE; closer to the pole f1 is called undecided altogether.
  ill-conditioned frame   the direction of v = d x n_s moves by <= ERR / sin rad, sin = |d x n_s| / |d|, and carries f2 (11 / 2 of it in
              t2) and f1 with it: 1.3e-6 / sin in t, more than EDGE below sin = 0.066. Calling all those pairs degenerate would exempt
              most keypoints, so the edge margin of t1 and t2 GROWS instead: max(EDGE, 5.5 ERR / sin). DEG = 2^-10 only fences off
              the pairs whose float32 cross product may vanish or lose its direction altogether (margin 1.4e-3 there)."""
import numpy as np

from normals_ref import r2_of, sqdist3

f32 = np.float32
MEASURED_T, MEASURED_SEAM, MEASURED_SWAP = 2.72e-6, 1.43e-6, 2.14e-7
EDGE = 2e-5
SEAM = 5.8e-6
SWAP = 8.6e-7
POLE = 2.0 ** -5
DEG = 2.0 ** -10
ERR = 4 * 2.0 ** -24
ALL = (1 << 11) - 1
CATEGORIES = ("edge", "seam", "swap", "pole", "degenerate")
EDGE_C, SEAM_C, SWAP_C, POLE_C, DEG_C = range(5)


def _dot(a, b):
    return (a * b).sum(-1)


def _bit(t):
    return 1 << np.clip(np.floor(t), 0, 10).astype(np.int64)


def _edge_mask(t, margin):
    """candidate bins of a bin coordinate: its own bin, and the neighbour across an edge 1..10 closer than the margin"""
    m = _bit(t)
    r = np.rint(t)
    near = (np.abs(t - r) < margin) & (r >= 1) & (r <= 10)
    ri = np.clip(r, 1, 10).astype(np.int64)
    return np.where(near, (1 << ri) | (1 << (ri - 1)), m), near


def _role(d, dn, ns, nt):
    """one role assignment in float64 -> dict(t [m, 3], x, y, sin, masks [m, 3], edge [m, 3], seam, pole, deg)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.cross(d, ns)
        cn = np.linalg.norm(c, axis=-1)
        v = c / cn[:, None]
        w = np.cross(ns, v)
        x, y = _dot(ns, nt), _dot(w, nt)
        f1, f2, f3 = np.arctan2(y, x), _dot(v, nt), _dot(ns, d) / dn
        sin = cn / dn
        hyp = np.hypot(x, y)
    deg = ~(sin >= DEG)
    t = np.stack([11 * (f1 + np.pi) / (2 * np.pi), 11 * (f2 + 1) / 2, 11 * (f3 + 1) / 2], 1)
    t = np.where(np.isfinite(t), t, 0.0)
    cond = np.maximum(EDGE, 5.5 * ERR / np.maximum(sin, DEG))           # t1 and t2 are as well determined as the direction of v
    masks, edge = _edge_mask(t, np.stack([cond, cond, np.full_like(cond, EDGE)], 1))
    pole = ~deg & (hyp < POLE)
    seam = ~deg & ~pole & (x < 0) & (np.abs(y) < SEAM * hyp)
    masks[:, 0] = np.where(seam, masks[:, 0] | 1 | (1 << 10), masks[:, 0])
    masks[:, 0] = np.where(pole, ALL, masks[:, 0])
    masks[deg, :2] = ALL                                       # if the pair is not skipped, v is noise and so are f1 and f2
    return dict(t=t, x=x, y=y, hyp=hyp, sin=sin, masks=masks, edge=edge, seam=seam, pole=pole, deg=deg)


def pairs64(P, N, src, tgt):
    """the pairs (src[i], tgt[i]) of one object in float64 -> dict of per-pair arrays:
    skip (identical coordinates), swap (roles swapped), tie, gap = |cos1| - |cos2|, A / B (the two role assignments, _role),
    masks [m, 3] (candidate bins as bit masks), cat [m, 3] (category of an undecided deposit, -1 = decided), deg"""
    P64, N64 = np.asarray(P, f32).astype(np.float64), np.asarray(N, f32).astype(np.float64)
    d = P64[tgt] - P64[src]
    dn = np.linalg.norm(d, axis=1)
    skip = (d == 0).all(1)
    dn_ = np.where(skip, 1.0, dn)
    cos1, cos2 = _dot(N64[src], d) / dn_, _dot(N64[tgt], d) / dn_
    gap = np.abs(cos1) - np.abs(cos2)
    swap = gap < 0
    tie = np.abs(gap) < SWAP
    A = _role(d, dn_, N64[src], N64[tgt])
    B = _role(-d, dn_, N64[tgt], N64[src])
    sw = swap[:, None]
    own = np.where(sw, B["masks"], A["masks"])
    other = np.where(sw, A["masks"], B["masks"])
    masks = np.where(tie[:, None], own | other, own)
    deg = np.where(swap, B["deg"], A["deg"]) | (tie & (A["deg"] | B["deg"]))
    pole = np.where(swap, B["pole"], A["pole"]) | (tie & (A["pole"] | B["pole"]))
    seam = np.where(swap, B["seam"], A["seam"]) | (tie & (A["seam"] | B["seam"]))
    single = (masks & (masks - 1)) == 0
    cat = np.full(masks.shape, EDGE_C, np.int64)
    cat[:, 0] = np.where(seam, SEAM_C, cat[:, 0])
    cat = np.where((tie & (own != other).any(1))[:, None] & (own != other), SWAP_C, cat)
    cat[:, 0] = np.where(pole, POLE_C, cat[:, 0])
    cat = np.where(single, -1, cat)
    cat = np.where(deg[:, None], DEG_C, cat)
    cat[skip] = -1
    t = np.where(sw, B["t"], A["t"])
    return dict(skip=skip, swap=swap, tie=tie, gap=gap, A=A, B=B, masks=masks, cat=cat, deg=deg & ~skip, t=t,
                x=np.where(swap, B["x"], A["x"]), y=np.where(swap, B["y"], A["y"]), hyp=np.where(swap, B["hyp"], A["hyp"]),
                sin=np.where(swap, B["sin"], A["sin"]), pole=pole, seam=seam)


def pairs32(P, N, src, tgt):
    """the same pairs in float32, every operation rounded, in the CPU oracle's written order (numpy's arccos / arctan2 stand for
    acosf / atan2f) -> dict(skip, swap, gap, t [m, 3] by the oracle's double bin formulas, f [m, 3], x, y)"""
    P, N = np.asarray(P, f32), np.asarray(N, f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        dp = P[tgt] - P[src]
        f4 = np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2])
        a, b = N[src].copy(), N[tgt].copy()
        angle1 = ((a[:, 0] * dp[:, 0] + a[:, 1] * dp[:, 1]) + a[:, 2] * dp[:, 2]) / f4
        angle2 = ((b[:, 0] * dp[:, 0] + b[:, 1] * dp[:, 1]) + b[:, 2] * dp[:, 2]) / f4
        swap = np.arccos(np.abs(angle1)) > np.arccos(np.abs(angle2))
        sw = swap[:, None]
        a, b = np.where(sw, b, a), np.where(sw, a, b)
        dp = np.where(sw, -dp, dp)
        f3 = np.where(swap, -angle2, angle1)
        v = np.stack([dp[:, 1] * a[:, 2] - dp[:, 2] * a[:, 1], dp[:, 2] * a[:, 0] - dp[:, 0] * a[:, 2],
                      dp[:, 0] * a[:, 1] - dp[:, 1] * a[:, 0]], 1)
        vn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        v = v / vn[:, None]
        w = np.stack([a[:, 1] * v[:, 2] - a[:, 2] * v[:, 1], a[:, 2] * v[:, 0] - a[:, 0] * v[:, 2],
                      a[:, 0] * v[:, 1] - a[:, 1] * v[:, 0]], 1)
        f2 = (v[:, 0] * b[:, 0] + v[:, 1] * b[:, 1]) + v[:, 2] * b[:, 2]
        y = (w[:, 0] * b[:, 0] + w[:, 1] * b[:, 1]) + w[:, 2] * b[:, 2]
        x = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        f1 = np.arctan2(y, x)
    assert f1.dtype == f32 and f2.dtype == f32 and f3.dtype == f32 and vn.dtype == f32
    d_pi = np.float64(f32(1.0) / (f32(2.0) * f32(np.pi)))
    f = np.stack([f1, f2, f3], 1)
    f64 = f.astype(np.float64)
    t = np.stack([11 * ((f64[:, 0] + np.pi) * d_pi), 11 * ((f64[:, 1] + 1.0) * 0.5), 11 * ((f64[:, 2] + 1.0) * 0.5)], 1)
    skip = (f4 == 0) | (vn == 0)
    gap = np.abs(angle1).astype(np.float64) - np.abs(angle2).astype(np.float64)
    return dict(skip=skip, coincident=f4 == 0, swap=swap, gap=gap, t=t, f=f, x=x, y=y)


def neighbour_pairs(P, need, radius):
    """(nbmask [n, n], src, tgt): all ordered pairs p != q by index with q in the ball of p, for the points p flagged in `need`"""
    P = np.asarray(P, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        nb = sqdist3(P[None, :, :], P[:, None, :]) < r2_of(radius)
    nb &= np.isfinite(P).all(1)[None, :]
    src, tgt = np.nonzero(nb & need[:, None])
    keep = src != tgt
    return nb, src[keep], tgt[keep]


class Result:
    """per keypoint: lo / hi [K, 33], count [K], nan [K], undecided [K, 5] (deposits per CATEGORIES), deposits [K], exempt [K],
    min_move [K] (inf where nothing contributes)"""

    def __init__(self, K):
        self.lo, self.hi = np.zeros((K, 33)), np.zeros((K, 33))
        self.count = np.zeros(K, np.int64)
        self.nan = np.zeros(K, bool)
        self.undecided = np.zeros((K, 5), np.int64)
        self.deposits = np.zeros(K, np.int64)
        self.exempt = np.zeros(K, bool)
        self.min_move = np.full(K, np.inf)
        self.n_max = np.zeros(K, np.int64)       # largest in-ball count n_p among the neighbours
        self.usable = np.zeros(K, np.int64)      # neighbours with d2 != 0


def spfh_counts(P, N, need, radius):
    """-> (n_p [n], lo / hi counts [n, 33], deposited pairs [n], undecided deposits per category [n, 5], degenerate pairs [n])"""
    n = len(P)
    nb, src, tgt = neighbour_pairs(P, need, radius)
    pr = pairs64(P, N, src, tgt)
    lo, hi = np.zeros((n, 33), np.int64), np.zeros((n, 33), np.int64)
    dep, ndeg = np.zeros(n, np.int64), np.zeros(n, np.int64)
    cat = np.zeros((n, 5), np.int64)
    live = ~pr["skip"]
    np.add.at(dep, src[live & ~pr["deg"]], 1)
    np.add.at(ndeg, src[pr["deg"]], 1)
    for f in range(3):
        m = pr["masks"][:, f]
        decided = live & (pr["cat"][:, f] < 0)
        for b in range(11):
            has = live & ((m >> b) & 1).astype(bool)
            np.add.at(hi[:, f * 11 + b], src[has], 1)
            np.add.at(lo[:, f * 11 + b], src[has & decided], 1)
        for c in range(5):
            np.add.at(cat[:, c], src[live & (pr["cat"][:, f] == c)], 1)
    return nb.sum(1), lo, hi, dep, cat, ndeg


def fpfh33(pt_off, P, N, kp_off, KP, radius):
    P, N, KP = np.asarray(P, f32), np.asarray(N, f32), np.asarray(KP, f32).reshape(-1, 3)
    out = Result(len(KP))
    r2 = r2_of(radius)
    for o in range(len(pt_off) - 1):
        s, e, ks, ke = int(pt_off[o]), int(pt_off[o + 1]), int(kp_off[o]), int(kp_off[o + 1])
        if ke == ks:
            continue
        if e == s:
            out.nan[ks:ke] = True
            continue
        X, XN, Q = P[s:e], N[s:e], KP[ks:ke]
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = sqdist3(X[None, :, :], Q[:, None, :])
            inb = (d2 < r2) & np.isfinite(X).all(1)[None, :] & np.isfinite(Q).all(1)[:, None]
        n_p, lo, hi, dep, cat, ndeg = spfh_counts(X, XN, inb.any(0), radius)
        use = inb & (d2 != 0)
        with np.errstate(divide="ignore"):
            W = np.where(use, 1.0 / np.where(use, d2, 1).astype(np.float64), 0.0)
            inc = np.where(n_p > 1, 100.0 / np.maximum(n_p - 1, 1), 0.0)
        WI = W * inc[None, :]
        S = WI @ dep
        with np.errstate(invalid="ignore", divide="ignore"):
            out.lo[ks:ke] = np.where(S[:, None] > 0, 100.0 * (WI @ lo) / S[:, None], 0.0)
            out.hi[ks:ke] = np.where(S[:, None] > 0, 100.0 * (WI @ hi) / S[:, None], 0.0)
            move = np.where(use & (dep > 0)[None, :], 100.0 * WI / S[:, None], np.inf)
        out.min_move[ks:ke] = move.min(1)
        out.count[ks:ke] = inb.sum(1)
        out.nan[ks:ke] = inb.sum(1) == 0
        out.undecided[ks:ke] = use.astype(np.int64) @ cat
        out.deposits[ks:ke] = use.astype(np.int64) @ (3 * (dep + ndeg))
        out.exempt[ks:ke] = (use & (ndeg > 0)[None, :]).any(1)
        out.n_max[ks:ke] = np.where(inb, n_p[None, :], 0).max(1)
        out.usable[ks:ke] = use.sum(1)
    out.lo[out.nan] = np.nan
    out.hi[out.nan] = np.nan
    return out


def measure(pt_off, P, N, kp_off, KP, radius):
    """float32 mode against float64 over every pair the scene evaluates -> dict(t, seam, swap: the largest differences; pairs)"""
    P, N, KP = np.asarray(P, f32), np.asarray(N, f32), np.asarray(KP, f32).reshape(-1, 3)
    worst = dict(t=0.0, seam=0.0, swap=0.0, pairs=0)
    for o in range(len(pt_off) - 1):
        s, e, ks, ke = int(pt_off[o]), int(pt_off[o + 1]), int(kp_off[o]), int(kp_off[o + 1])
        if ke == ks or e == s:
            continue
        X, XN, Q = P[s:e], N[s:e], KP[ks:ke]
        with np.errstate(invalid="ignore", over="ignore"):
            inb = (sqdist3(X[None, :, :], Q[:, None, :]) < r2_of(radius)) & np.isfinite(Q).all(1)[:, None]
        _, src, tgt = neighbour_pairs(X, inb.any(0), radius)
        if len(src) == 0:
            continue
        a, b = pairs64(X, XN, src, tgt), pairs32(X, XN, src, tgt)
        assert np.array_equal(a["skip"], b["coincident"])
        live = ~a["skip"]
        worst["swap"] = max(worst["swap"], float(np.abs(a["gap"] - b["gap"])[live].max(initial=0.0)))
        assert (a["tie"] | (a["swap"] == b["swap"]))[live].all()          # outside the tie margin both precisions take the same roles
        ok = live & ~a["deg"] & ~b["skip"] & (a["swap"] == b["swap"])
        dt = np.abs(a["t"] - b["t"])
        dt[:, 0] = np.minimum(dt[:, 0], 11 - dt[:, 0])                      # across the seam t1 = 0 and t1 = 11 are the same angle
        ok1 = ok & ~a["pole"]
        worst["t"] = max(worst["t"], float(dt[ok1, 0].max(initial=0.0)), float(dt[ok, 1:].max(initial=0.0)))
        with np.errstate(invalid="ignore", divide="ignore"):
            yh32 = b["y"].astype(np.float64) / np.hypot(b["x"].astype(np.float64), b["y"].astype(np.float64))
            yh64 = a["y"] / a["hyp"]
        worst["seam"] = max(worst["seam"], float(np.abs(yh32 - yh64)[ok1].max(initial=0.0)))
        worst["pairs"] += int(live.sum())
    return worst

"""CoSPAIR in float64, brute force (numpy only), written from the reference's text (third_party/cospair/cospair.cpp:18-294 with
num_levels 7, num_bins 9, rgb_type 5, num_rgb_bins 9): one object at a time, no grid, no fast arithmetic. The pair
features and their margin machinery are fpfh_ref's (pairs64, pairs32, the categories); nothing of it is copied or edited.

Decided in float32, bit for bit as the device decides (normals_ref.sqdist3):
  snap      the centre is the finite point of the object with the smallest d2 to the keypoint, the lowest index among equals
  shells    level l = 1..7 owns the points with r2_{l-1} <= d2 < r2_l, d2 to the CENTRE, r2_l = float32((l / 7 * float64(radius))^2),
            r2_0 = 0; the centre itself is dropped by index; a point whose normal is not finite is skipped and not counted
  NaN row   keypoint not finite, no finite point, or the centre's normal not finite: counts 0, snap -1
so the pair counts n_l are always decided. Colour indices (colour_indices) follow the reference's double sequence on the
unnormalised Lab of a `rgb2lab` callable (the oracle's) and are always decided too.

Geometry: the features of the pair (source = centre, target = neighbour) in float64 from the float32 inputs (fpfh_ref.pairs64). With
c1 = (f1 + pi) 9 / 2pi, c2 = acos(f2) 9 / pi, c3 = acos(f3) 9 / pi the reference's bins are floor(c), and index = offset + bin inside
the level's 27-entry array, clamped to [0, 26] (bin 9 of f1 / f2 lands on bin 0 of the next feature, bin 9 of f3 is clamped). A deposit
is DECIDED (one index) or UNDECIDED (a set of candidate indices):
  edge        c within its margin of an integer 1..8                         -> the two adjacent bins
              c1 within its margin of 9, f2 / f3 within SPILL of -1           -> bins 8 and 9 (the spill)
  seam        fpfh_ref's rule (x < 0 and |y| < SEAM hypot)                    -> bins 0, 8 and 9 of f1
  swap tie    fpfh_ref's rule                                                 -> the candidates of both role assignments
  pole        fpfh_ref's rule                                                 -> every bin of f1
  degenerate  fpfh_ref's rule (|d x n_s| / |d| < DEG)                         -> every bin of f1 and f2, the computed bins of f3 plus bin 4:
                                                                                 PCL zeroes the features of a pair it gives up (f = 0 is
                                                                                 bin 4 of each), and the pair counts either way
  coincident  identical coordinates: f = 0 exactly                           -> 4 / 4 / 4, decided
Per entry lo counts the decided deposits and hi adds every undecided deposit that has the entry as a candidate; the expected values
are value(lo) and value(hi), value(c) = float32(float32(c) / float32(n_l)) * float32(l).

Margins. measure() recomputes every pair in float32 in the device's exact sequence (fpfh_ref.pairs32 for the features, then
deg_f1 = f1 * 57.29578f + 180, deg = acosf(clamp f) * 57.29578f, c = float64(deg) / 40 or / 20) and compares with float64. Largest
values over the scenes of cospair_scenes.py (test_cospair_cpu.py::test_margins_are_four_to_eight_times_the_measured_error prints them
per scene and asserts >= 4 x and <= 8 x):
  max |c_float32 - c_float64| over the pairs whose margin is EDGE itself (well-conditioned, away from the pole, no tie)
                                                        MEASURED_C = 5.05e-6 (thin)  -> EDGE = 2.2e-5
The device's fast path differs from its exact one by < 2e-5 in c1 and < 4e-6 in f2 / f3 and only decides outside its own guards
(1e-4 in c1, 2e-5 in f); what it may decide is therefore what the exact path decides, and EDGE covers that path.
Reasoned, as in fpfh_ref (ERR = 4 * 2^-24: the absolute error of a float32 sum of three products of magnitudes <= 1):
  f3 carries ERR, f2 and the direction of (x, y) carry ERR / sin (sin = |d x n_s| / |d|: the conditioning of the frame), and acos
  magnifies an error in f by 1 / sqrt(1 - f^2): margin_1 = max(EDGE, 9 / 2pi * ERR / sin), margin_2 = max(EDGE, 9 / pi * ERR /
  (sin sqrt(1 - f2^2))), margin_3 = max(EDGE, 9 / pi * ERR / sqrt(1 - f3^2)), each capped at 0.5 (adjacent bins only; near f = +-1
  the arccosine is far from every edge 1..8). test_cospair_cpu.py asserts that EVERY measured pair lies inside its margin.
  SPILL = 4 ERR / sin for f2, 4 ERR for f3: acos reaches 180 degrees only when the float32 f is <= -1."""
import numpy as np

import fpfh_ref as fr
from normals_ref import sqdist3

f32 = np.float32
LEVELS, BINS, BLOCK, LEVEL, DIM = 7, 9, 27, 54, 378
MEASURED_C = 5.05e-6
EDGE = 2.2e-5
ERR = fr.ERR
CATEGORIES = fr.CATEGORIES
FULL = (1 << 10) - 1                      # bins 0..9 of one feature


def level_r2(radius):
    """[r2_0 = 0, r2_1, .., r2_7] as float32"""
    r = np.float64(f32(radius))
    return f32([0.0] + [(np.float64(l) / LEVELS * r) ** 2 for l in range(1, LEVELS + 1)])


def value(c, n, l):
    """(count / levelpaircount) * l in float32, 0 for an empty level"""
    c, n = np.asarray(c), np.asarray(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (c.astype(f32) / n.astype(f32)).astype(f32) * f32(l)
    return np.where(n > 0, v, f32(0)).astype(f32)


def colour_bins(rgb2lab, rgba):
    """the reference's three colour bins of one 0x00RRGGBB colour (may be -2 .. 10), cospair.cpp:220-231"""
    L, a, b = (f32(v) for v in rgb2lab(int(rgba)))
    l_ = f32(1.0 * np.float64(L) / 100)
    a_ = f32(1.0 * (np.float64(a) + 86.185) / 184.439)
    b_ = f32(1.0 * (np.float64(b) + 107.863) / 202.345)
    return tuple(int(np.floor(np.float64(x) / (1.0 / BINS))) for x in (l_, a_, b_))


def resolve(offset, b):
    """index inside the 27-entry array: offset + bin, clamped to the array"""
    return int(min(max(offset + b, 0), BLOCK - 1))


def colour_indices(rgb2lab, rgba):
    """[n, 3] resolved indices (L, a, b) of every colour"""
    rgba = np.asarray(rgba, np.uint32)
    table = {c: [resolve(BINS * j, b) for j, b in enumerate(colour_bins(rgb2lab, c))] for c in np.unique(rgba).tolist()}
    return np.array([table[c] for c in rgba.tolist()], np.int64).reshape(-1, 3)


def snap(X, q):
    """index of the finite point of X nearest to q in float32 (lowest index among equals), -1 when there is none or q is not finite"""
    X, q = np.asarray(X, f32), np.asarray(q, f32)
    fin = np.isfinite(X).all(1)
    if not fin.any() or not np.isfinite(q).all():
        return -1
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = sqdist3(X, q)
    d2 = np.where(fin, d2, np.inf)
    return int(np.argmin(d2))


def _c_of(role):
    """(c [m, 3], f2, f3) of one role assignment of fpfh_ref._role: its t are 11 (f1 + pi) / 2pi, 11 (f + 1) / 2"""
    t = role["t"]
    f2, f3 = 2 * t[:, 1] / 11 - 1, 2 * t[:, 2] / 11 - 1
    c = np.stack([t[:, 0] * BINS / 11, np.arccos(np.clip(f2, -1, 1)) * BINS / np.pi, np.arccos(np.clip(f3, -1, 1)) * BINS / np.pi], 1)
    return c, f2, f3


def _margins(role, f2, f3):
    sin = np.maximum(role["sin"], fr.DEG)
    s2, s3 = np.sqrt(np.maximum(1 - f2 * f2, 1e-300)), np.sqrt(np.maximum(1 - f3 * f3, 1e-300))
    m = np.stack([np.maximum(EDGE, BINS / (2 * np.pi) * ERR / sin), np.maximum(EDGE, BINS / np.pi * ERR / (sin * s2)),
                  np.maximum(EDGE, BINS / np.pi * ERR / s3)], 1)
    return np.minimum(m, 0.5)


def _bins_mask(c, m):
    """candidate bins (bit mask over 0..9) of a coordinate c in [0, 9] with margin m: its own bin and the one across a close edge 1..8"""
    own = np.clip(np.floor(c), 0, BINS).astype(np.int64)
    r = np.rint(c)
    near = (np.abs(c - r) < m) & (r >= 1) & (r <= BINS - 1)
    ri = np.clip(r, 1, BINS - 1).astype(np.int64)
    return np.where(near, (1 << ri) | (1 << (ri - 1)), 1 << own), near


def _role_candidates(role):
    """bit masks over the bins 0..9 per feature [m, 3] of one role assignment, and the edge flags [m, 3]"""
    c, f2, f3 = _c_of(role)
    m = _margins(role, f2, f3)
    masks, edge = _bins_mask(c, m)
    top = 1 << (BINS - 1) | 1 << BINS
    sin = np.maximum(role["sin"], fr.DEG)
    spill = np.stack([c[:, 0] > BINS - m[:, 0], f2 < -1 + 4 * ERR / sin, f3 < -1 + 4 * ERR], 1)
    masks = np.where(spill, masks | top, masks)
    edge = edge | spill
    masks[:, 0] = np.where(role["seam"], masks[:, 0] | 1 | top, masks[:, 0])
    masks[:, 0] = np.where(role["pole"], FULL, masks[:, 0])
    deg = role["deg"]
    masks[deg, 0] = FULL
    masks[deg, 1] = FULL
    masks[deg, 2] |= 1 << 4
    return masks, edge, c, m


def pair_candidates(P, N, src, tgt):
    """the pairs (src[i] = centre, tgt[i]) of one object -> dict(index [m, 3] bit masks over the 27 entries of a level's geometry array,
    cat [m, 3] (fpfh_ref's category numbers, -1 = decided), c [m, 3] and margin [m, 3] of the role taken, plus fpfh_ref's pair flags)"""
    pr = fr.pairs64(P, N, src, tgt)
    (mA, eA, cA, gA), (mB, eB, cB, gB) = _role_candidates(pr["A"]), _role_candidates(pr["B"])
    sw = pr["swap"][:, None]
    own, other = np.where(sw, mB, mA), np.where(sw, mA, mB)
    tie = pr["tie"][:, None]
    bins = np.where(tie, own | other, own)
    idx = np.zeros_like(bins)
    for f in range(3):                                   # bins -> entries: offset 9 f + bin, the last one clamped into the array
        for b in range(BINS + 1):
            idx[:, f] |= np.where((bins[:, f] >> b) & 1 == 1, 1 << resolve(BINS * f, b), 0)
    skip = pr["skip"]
    idx[skip] = [1 << 4, 1 << 13, 1 << 22]               # coincident: PCL returns f = 0
    single = (idx & (idx - 1)) == 0
    cat = np.full(idx.shape, fr.EDGE_C, np.int64)
    cat[:, 0] = np.where(pr["seam"], fr.SEAM_C, cat[:, 0])
    cat = np.where(tie & (own != other), fr.SWAP_C, cat)
    cat[:, 0] = np.where(pr["pole"], fr.POLE_C, cat[:, 0])
    cat = np.where(pr["deg"][:, None], fr.DEG_C, cat)
    cat = np.where(single, -1, cat)
    return dict(index=idx, cat=cat, c=np.where(sw, cB, cA), margin=np.where(sw, gB, gA), skip=skip, swap=pr["swap"], tie=pr["tie"],
                deg=pr["deg"], pole=pr["pole"], seam=pr["seam"])


class Result:
    """per keypoint: lo / hi [K, 378] counts, n [K, 7] pairs per level, snap [K] (object-local index, -1: NaN row), nan [K],
    undecided [K] deposits, cats [K, 5] undecided deposits per fpfh_ref category; want_lo / want_hi [K, 378] float32 values"""

    def __init__(self, K):
        self.lo, self.hi = np.zeros((K, DIM), np.int64), np.zeros((K, DIM), np.int64)
        self.n = np.zeros((K, LEVELS), np.int64)
        self.snap = np.full(K, -1, np.int64)
        self.nan = np.zeros(K, bool)
        self.undecided = np.zeros(K, np.int64)
        self.cats = np.zeros((K, 5), np.int64)

    def finish(self):
        n = np.repeat(self.n, LEVEL, axis=1)
        lev = np.repeat(np.arange(1, LEVELS + 1), LEVEL)[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            self.want_lo = np.where(n > 0, (self.lo.astype(f32) / n.astype(f32)).astype(f32) * lev.astype(f32), f32(0)).astype(f32)
            self.want_hi = np.where(n > 0, (self.hi.astype(f32) / n.astype(f32)).astype(f32) * lev.astype(f32), f32(0)).astype(f32)
        self.want_lo[self.nan] = np.nan
        self.want_hi[self.nan] = np.nan
        self.decided_row = (self.lo == self.hi).all(1)
        return self


def shells(X, XN, c, radius):
    """(neighbour indices, their level 0..6) of centre index c: in-ball by float32 d2 to the centre, the centre dropped by index,
    non-finite points and normals skipped"""
    r2 = level_r2(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = sqdist3(X, X[c])
    ok = np.isfinite(X).all(1) & np.isfinite(XN).all(1) & (d2 < r2[LEVELS])
    ok[c] = False
    nb = np.nonzero(ok)[0]
    return nb, (d2[nb][:, None] >= r2[None, 1:LEVELS]).sum(1)


def cospair(rgb2lab, pt_off, P, N, rgba, kp_off, KP, radius):
    P, N, KP = np.asarray(P, f32), np.asarray(N, f32), np.asarray(KP, f32).reshape(-1, 3)
    out = Result(len(KP))
    for o in range(len(pt_off) - 1):
        s, e, ks, ke = int(pt_off[o]), int(pt_off[o + 1]), int(kp_off[o]), int(kp_off[o + 1])
        X, XN = P[s:e], N[s:e]
        col = colour_indices(rgb2lab, np.asarray(rgba)[s:e]) if e > s else np.zeros((0, 3), np.int64)
        for k in range(ks, ke):
            c = snap(X, KP[k]) if e > s else -1
            if c < 0 or not np.isfinite(XN[c]).all():
                out.nan[k] = True
                continue
            out.snap[k] = c
            nb, lev = shells(X, XN, c, radius)
            out.n[k] = np.bincount(lev, minlength=LEVELS)
            if len(nb) == 0:
                continue
            pc = pair_candidates(X, XN, np.full(len(nb), c), nb)
            decided = pc["cat"] < 0
            for f in range(3):
                m = pc["index"][:, f]
                for i in range(BINS * f, min(BINS * f + BINS + 1, BLOCK)):
                    has = (m >> i) & 1 == 1
                    if has.any():
                        np.add.at(out.hi[k], lev[has] * LEVEL + i, 1)
                        np.add.at(out.lo[k], lev[has & decided[:, f]] * LEVEL + i, 1)
                np.add.at(out.lo[k], lev * LEVEL + BLOCK + col[nb, f], 1)
                np.add.at(out.hi[k], lev * LEVEL + BLOCK + col[nb, f], 1)
            out.undecided[k] = int((~decided).sum())
            for cnum in range(5):
                out.cats[k, cnum] = int((pc["cat"] == cnum).sum())
    return out.finish()


def c_float32(P, N, src, tgt):
    """the three coordinates c of the pairs in float32, in the device's exact sequence; dict(c [m, 3], skip, swap, coincident)"""
    b = fr.pairs32(P, N, src, tgt)
    f = np.where(b["skip"][:, None], f32(0), b["f"]).astype(f32)
    with np.errstate(invalid="ignore"):
        deg1 = ((f[:, 0] * f32(57.29578)).astype(f32) + f32(180)).astype(f32)
        deg2 = (np.arccos(np.clip(f[:, 1], f32(-1), f32(1))).astype(f32) * f32(57.29578)).astype(f32)
        deg3 = (np.arccos(np.clip(f[:, 2], f32(-1), f32(1))).astype(f32) * f32(57.29578)).astype(f32)
    c = np.stack([deg1.astype(np.float64) / (360.0 / BINS), deg2.astype(np.float64) / (180.0 / BINS), deg3.astype(np.float64) / (180.0 / BINS)], 1)
    return dict(c=c, skip=b["skip"], swap=b["swap"], coincident=b["coincident"])


def measure(pt_off, P, N, kp_off, KP, radius):
    """float32 against float64 over every pair the scene evaluates -> dict(c: the largest |c32 - c64| over the pairs whose margin is
    EDGE itself; ratio: the largest |c32 - c64| / margin over all non-degenerate pairs away from pole, seam and tie; pairs)"""
    P, N, KP = np.asarray(P, f32), np.asarray(N, f32), np.asarray(KP, f32).reshape(-1, 3)
    worst = dict(c=0.0, ratio=0.0, pairs=0)
    for o in range(len(pt_off) - 1):
        s, e, ks, ke = int(pt_off[o]), int(pt_off[o + 1]), int(kp_off[o]), int(kp_off[o + 1])
        X, XN = P[s:e], N[s:e]
        for k in range(ks, ke):
            c = snap(X, KP[k]) if e > s else -1
            if c < 0 or not np.isfinite(XN[c]).all():
                continue
            nb, _ = shells(X, XN, c, radius)
            if len(nb) == 0:
                continue
            src = np.full(len(nb), c)
            a, b = pair_candidates(X, XN, src, nb), c_float32(X, XN, src, nb)
            ok = ~a["skip"] & ~a["deg"] & ~a["tie"] & ~b["skip"] & (a["swap"] == b["swap"])
            d = np.abs(a["c"] - b["c"])
            d[:, 0] = np.minimum(d[:, 0], BINS - d[:, 0])
            use = np.stack([ok & ~a["pole"] & ~a["seam"], ok, ok], 1)
            tight = use & (a["margin"] == EDGE)
            worst["c"] = max(worst["c"], float(d[tight].max(initial=0.0)))
            worst["ratio"] = max(worst["ratio"], float((d / a["margin"])[use].max(initial=0.0)))
            worst["pairs"] += int(ok.sum())
    return worst

"""The GASD region descriptor (ismhip_global_gasd, include/ismhip.h) restated in float64, numpy only, from the header's text: the
selected points in the region's covariance frame, scaled by max_coord onto a 6^3 grid of positions (bins 0..215) and a 4^3 grid of
positions x 12 hue bins (bins 216..983), INTEGER counts, then one product per bin.

Inputs are the selected points (and colours) and the DEVICE's centroid c, frame and max_coord: they are outputs of the same call, held to
their own checks (frame64 and max_coord64 below). The device evaluates coord = (t / max_coord) * h + h in float32; float64 may land
in another cell when coord is close to a cell face. So the counts come as an INTERVAL: a deposit whose coord lies within MARGIN of an
interior face 1 .. 2h - 1, or of the upper face 2h, is UNDECIDED on that axis: it is a candidate for both neighbours (for "dropped" at
the upper face), counted in `upper` for every bin it could reach and in `lower` for none. The face 0 is no decision: max_coord is the
float32 maximum of |t|, so the float32 quotient is >= -1 and coord >= 0; float64 values below 0 are taken as cell 0.

MARGIN, in cell units, from the float32 roundings (u = 2^-24, h <= 3 the half-grid, the frame orthonormal so |d|_2 <= sqrt(3) max_coord):
  d = p - c            each component off by <= u |d_i|                       -> in t: <= u sum |x_i d_i|
  t = (x0 d0 + x1 d1) + x2 d2   three products and two sums, each <= u of its size -> <= 3 u sum |x_i d_i|
                       sum |x_i d_i| <= |x|_2 |d|_2 <= sqrt(3) max_coord      -> |t32 - t64| <= 4 sqrt(3) u max_coord = 6.93 u max_coord
  q = t / max_coord    |q| <= 1: one rounding <= u                            -> |q32 - q64| <= 7.93 u
  q * h                one rounding <= h u                                    -> <= 8.93 h u
  + h                  the sum is <= 2 h: one rounding <= 2 h u               -> |coord32 - coord64| <= 10.93 h u
MARGIN = 12 h u at h = 3 = 36 * 2^-24 = 2.15e-6 (the colour grid, h = 2, is held to the same). test_gasd_cpu.py prints the worst
|coord32 - coord64| per scene and asserts that it stays below MARGIN.
The hue bin is a function of three 8-bit integers in float32 operations that IEEE defines exactly: it is decided, and restated
operation by operation (hue_bins32)."""
import numpy as np

f32, f64 = np.float32, np.float64
DIM, SHAPE_DIM, SHAPE_BINS, HUE_BINS = 984, 512, 216, 12
U = 2.0 ** -24
MARGIN = 36 * U
GAP = 1e-3                      # eigenvalue gaps below GAP * lambda_max: the axes are not compared with the device's
NO_BIN = 255


def hue_bins32(rgba):
    """the hue rule in float32, operation by operation -> uint8 bins 0..11, NO_BIN where nothing is deposited"""
    c = np.asarray(rgba).astype(np.int64) & 0xffffff
    r, g, b = ((c >> 16) & 255).astype(np.int32), ((c >> 8) & 255).astype(np.int32), (c & 255).astype(np.int32)
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        diff_inv = f32(1.0) / (mx - mn).astype(f32)
        hr = f32(60.0) * ((g - b).astype(f32) * diff_inv)
        hg = f32(60.0) * (f32(2.0) + (b - r).astype(f32) * diff_inv)
        hb = f32(60.0) * (f32(4.0) + (r - g).astype(f32) * diff_inv)
        hue = np.where(~np.isfinite(diff_inv), f32(0.0), np.where(mx == r, hr, np.where(mx == g, hg, hb))).astype(f32)
        hue = np.where(hue < 0, hue + f32(360.0), hue).astype(f32)
        k = np.floor((hue / f32(360.0)) * f32(HUE_BINS))
    assert hue.dtype == f32 and k.dtype == f32
    return np.where((k >= 0) & (k < HUE_BINS), k, NO_BIN).astype(np.uint8)


def _rotate64(P, c, frame):
    d = np.asarray(P, f32).reshape(-1, 3).astype(f64) - np.asarray(c, f32).astype(f64)[None, :]
    return d @ np.asarray(frame, f32).reshape(3, 3).astype(f64).T


def rotate32(P, c, frame):
    """t = (x . d, y . d, z . d), d = p - c, in float32: products and sums unfused, in the order (a0 d0 + a1 d1) + a2 d2"""
    d = (np.asarray(P, f32).reshape(-1, 3) - np.asarray(c, f32)[None, :]).astype(f32)
    F = np.asarray(frame, f32).reshape(3, 3)
    return np.stack([((F[a, 0] * d[:, 0] + F[a, 1] * d[:, 1]).astype(f32) + F[a, 2] * d[:, 2]).astype(f32) for a in range(3)], 1)


def max_coord32(P, c, frame):
    t = rotate32(P, c, frame)
    return f32(np.abs(t).max(initial=0.0))


def max_coord64(P, c, frame):
    return float(np.abs(_rotate64(P, c, frame)).max(initial=0.0))


def coords32(P, c, frame, mc, half):
    """(d): coord = (t / max_coord) * half + half in float32, in this order"""
    q = (rotate32(P, c, frame) / f32(mc)).astype(f32)
    return ((q * f32(half)).astype(f32) + f32(half)).astype(f32)


def coords64(P, c, frame, mc, half):
    return (_rotate64(P, c, frame) / f64(f32(mc))) * half + half


def cells32(P, c, frame, mc, half):
    """(e) / (f): floor(coord) per axis, -1 outside 0 .. 2 half - 1 or for a NaN -> [n, 3] int64"""
    k = np.floor(coords32(P, c, frame, mc, half))
    with np.errstate(invalid="ignore"):
        return np.where((k >= 0) & (k < 2 * half), k, -1).astype(np.int64)


def bins32(P, rgba, c, frame, mc, with_color=True):
    """the float32 transcription of (d) to (f) -> (shape bin [n] or -1, colour bin [n] or -1 (all -1 without colour))"""
    s = cells32(P, c, frame, mc, 3)
    shape = np.where((s >= 0).all(1), (s[:, 0] * 6 + s[:, 1]) * 6 + s[:, 2], -1)
    if not with_color:
        return shape, np.full(len(shape), -1, np.int64)
    g = cells32(P, c, frame, mc, 2)
    hb = hue_bins32(rgba).astype(np.int64)
    colour = np.where((g >= 0).all(1) & (hb != NO_BIN), SHAPE_BINS + ((g[:, 0] * 4 + g[:, 1]) * 4 + g[:, 2]) * HUE_BINS + hb, -1)
    return shape, colour


def _block(coord, half, axes, extra, n_extra, margin):
    """one grid: coord [n, 3] float64; axes the grid axes that count (the others are summed out); extra [n] a further decided index
    (the hue bin, -1 = no deposit) of n_extra values, or None -> dict(counts, lower, upper [cells^len(axes) * n_extra], deposits,
    undecided, total_lower, total_upper)"""
    cells = 2 * half
    n = len(coord)
    coord = coord[:, list(axes)]
    k = np.rint(coord)
    near = (np.abs(coord - k) <= margin) & (k >= 1) & (k <= cells)
    face = np.maximum(np.floor(coord), 0)
    alt = np.where(face == k, k - 1, k)                       # the cell across the near face
    face = np.where(face >= cells, -1, face).astype(np.int64)
    alt = np.where(alt >= cells, -1, alt).astype(np.int64)
    ok_extra = np.ones(n, bool) if extra is None else extra >= 0
    e = np.zeros(n, np.int64) if extra is None else np.where(ok_extra, extra, 0)
    size = cells ** len(axes) * n_extra

    def index(c):
        i = np.zeros(n, np.int64)
        for a in range(len(axes)):
            i = i * cells + c[:, a]
        return np.where((c >= 0).all(1) & ok_extra, i * n_extra + e, -1)

    decided = ~near.any(1)
    fi = index(face)
    counts = np.bincount(fi[fi >= 0], minlength=size)
    lower = np.bincount(fi[decided & (fi >= 0)], minlength=size)
    upper = np.zeros(size, np.int64)
    reach = np.zeros(n, bool)
    for combo in range(1 << len(axes)):
        use = np.array([(combo >> a) & 1 for a in range(len(axes))], bool)
        valid = near[:, use].all(1)
        ci = index(np.where(use[None, :], alt, face))
        hit = valid & (ci >= 0)
        upper += np.bincount(ci[hit], minlength=size)
        reach |= hit
    live = ok_extra                                             # a deposit: a point this block looks at
    return dict(counts=counts, lower=lower, upper=upper, deposits=int(live.sum()), undecided=int((live & ~decided).sum()),
                total_lower=int((decided & (fi >= 0)).sum()), total_upper=int(reach.sum()))


def gasd_counts(P, rgba, c, frame, mc, with_color=True, margin=MARGIN, axes=(0, 1, 2)):
    """One region: P the selected points, rgba their packed colours (or None), c / frame / mc the device's centroid, frame [9] and
    max_coord -> dict(counts, lower, upper int64 [984 or 512]; n; deposits; undecided; total_lower / total_upper [2]: per block).
    counts takes every float64 decision at face value. axes = (0, 1): the grids' z index is summed out (rows of 36 + 192 bins, see
    z_marginal): for a region that lies in the plane t.z = 0, where z is undecided by construction."""
    P = np.asarray(P, f32).reshape(-1, 3)
    n = len(P)
    full = tuple(axes) == (0, 1, 2)
    dim = (DIM if with_color else SHAPE_DIM) if full else 36 + (192 if with_color else 0)
    out = dict(counts=np.zeros(dim, np.int64), lower=np.zeros(dim, np.int64), upper=np.zeros(dim, np.int64), n=n, deposits=0, undecided=0,
               total_lower=np.zeros(2, np.int64), total_upper=np.zeros(2, np.int64))
    if n < 2 or not (mc > 0 and np.isfinite(mc)):
        return out
    blocks = [_block(coords64(P, c, frame, mc, 3.0), 3, axes, None, 1, margin)]
    if with_color:
        hb = hue_bins32(rgba).astype(np.int64)
        blocks.append(_block(coords64(P, c, frame, mc, 2.0), 2, axes, np.where(hb == NO_BIN, -1, hb), HUE_BINS, margin))
    o = 0
    for i, b in enumerate(blocks):
        m = len(b["counts"])
        for k in ("counts", "lower", "upper"):
            out[k][o:o + m] = b[k]
        o += m
        out["deposits"] += b["deposits"]; out["undecided"] += b["undecided"]
        out["total_lower"][i] = b["total_lower"]; out["total_upper"][i] = b["total_upper"]
    return out


def z_marginal(counts, with_color=True):
    """a device row of counts summed over the z index of both grids -> [36 (+ 192)]"""
    counts = np.asarray(counts, np.int64)
    s = counts[:SHAPE_BINS].reshape(6, 6, 6).sum(2).ravel()
    if not with_color:
        return s
    return np.concatenate([s, counts[SHAPE_BINS:DIM].reshape(4, 4, 4, HUE_BINS).sum(2).ravel()])


def block_totals(counts, with_color=True):
    counts = np.asarray(counts, np.int64)
    return [int(counts[:SHAPE_BINS].sum()), int(counts[SHAPE_BINS:DIM].sum()) if with_color else 0]


def row_of_counts(counts, n_sel, with_color=True):
    """(g): float32(float64(count) * float64(incr)), incr = 100.0f / float32(n_sel - 1) in float32; without colour 512 floats, the bins
    past the shape block zero; n_sel < 2: NaN"""
    dim = DIM if with_color else SHAPE_DIM
    if n_sel < 2:
        return np.full(dim, np.nan, f32)
    incr = f64(f32(100.0) / f32(n_sel - 1))
    row = (np.asarray(counts, f64)[:dim] * incr).astype(f32)
    if not with_color:
        row[SHAPE_BINS:] = 0
    return row


def covariance64(P, c):
    d = np.asarray(P, f32).reshape(-1, 3).astype(f64) - np.asarray(c, f32).astype(f64)[None, :]
    return d.T @ d


def frame64(P, c, view_direction=(0, 0, 1), margin=MARGIN):
    """(b), (c): the frame from a float64 eigen-decomposition of the unnormalised covariance round c -> dict(frame [3, 3] rows x, y, z;
    w ascending eigenvalues; degenerate: an eigenvalue gap below GAP * lambda_max (the axes are then not unique); undecided: points
    with |t.x| within the float32 error of 0 could change the majority that signs x; tie: the fallback rule signed x)"""
    P = np.asarray(P, f32).reshape(-1, 3)
    C = covariance64(P, c)
    w, V = np.linalg.eigh(C)
    z, x = V[:, 0].copy(), V[:, 2].copy()
    if z @ np.asarray(view_direction, f64) > 0:
        z = -z
    d = P.astype(f64) - np.asarray(c, f32).astype(f64)[None, :]
    t = d @ x
    eps = (margin / 3.0) * max(float(np.abs(d @ V).max(initial=0.0)), 0.0)      # 12 u max_coord: the bound on |t32 - t64| with margin
    exact0 = (d * x[None, :] == 0).all(1)                      # every product an exact zero: t.x = 0 in any precision, on neither side
    pos, neg, unsure = int((t > eps).sum()), int((t < -eps).sum()), int(((np.abs(t) <= eps) & ~exact0).sum())
    tie = pos == neg and unsure == 0
    undecided = unsure > 0 and abs(pos - neg) <= unsure
    if tie:
        k = int(np.argmax(np.abs(x)))                          # the first of equal magnitudes
        flip = x[k] < 0
    else:
        flip = neg > pos
    if flip:
        x = -x
    y = np.cross(z, x)
    lmax = max(float(w[2]), 0.0)
    degenerate = not (min(w[1] - w[0], w[2] - w[1]) > GAP * lmax)
    return dict(frame=np.stack([x, y, z]), w=w, C=C, degenerate=degenerate, undecided=bool(undecided), tie=bool(tie), pos=pos, neg=neg)


def disagreements(P, rgba, c, frame, mc, with_color=True, margin=MARGIN):
    """the float32 transcription against the float64 candidates over one region -> dict(outside: deposits where float32 lands in a cell
    (or drops) that float64 does not hold possible; worst: the largest |coord32 - coord64| over both grids)"""
    outside, worst = 0, 0.0
    for half in (3.0, 2.0) if with_color else (3.0,):
        c32, c64 = coords32(P, c, frame, mc, half).astype(f64), coords64(P, c, frame, mc, half)
        worst = max(worst, float(np.abs(c32 - c64).max(initial=0.0)))
        cells = 2 * half
        k = np.rint(c64)
        near = (np.abs(c64 - k) <= margin) & (k >= 1) & (k <= cells)
        face = np.maximum(np.floor(c64), 0)
        alt = np.where(face == k, k - 1, k)
        got = np.floor(c32)
        outside += int(((got != face) & ~(near & (got == alt))).sum())
    return dict(outside=outside, worst=worst)

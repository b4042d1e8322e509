"""The ESF_LOCAL descriptor (ismhip_esf_local, include/ismhip.h) restated in float64, numpy only, from the header's text: steps 3 to 8
for one keypoint's ball. It shares nothing with the kernel but the written hash h(seed, x).

Inputs are the ball's points (float32, ascending cloud index) and the DEVICE's centroid c and largest distance m (outputs of the same
call, held to checks of their own: scale_bounds). The device evaluates every step in float32; float64 may take another side of a hard
decision that lies close. So the answer is an INTERVAL lo..hi of integer numerators (sixths) per bin.

THE ERROR MODEL. Every float32 operation the header writes (+, -, *, /, sqrt) is correctly rounded: fl(x) = x (1 + d), |d| <= U = 2^-24,
and fl(x) = x when x is a float32 number. Each intermediate is carried here as (value in float64 from the float32 inputs, bound of
|float32 value - that value|), the bound propagated operation by operation (_Q below): a sum adds the bounds, a product a*b gets
|a| eb + |b| ea + ea eb, a quotient and a square root their first-order terms inflated by the bound itself, and every operation adds its
own rounding U |value| -- unless the operands carry no error and the value is a float32 number, in which case float32 computed it exactly
and the bound stays 0. Nothing is tuned: the bounds follow from the written operations, and test_esf_local_cpu.py checks on every scene
that a float32 numpy transcription (esf32) stays inside them. acosf is not a rounded operation: its result is taken within 4 U of the
true arc cosine of its float32 argument (OCML documents 2 ulp at most), and the three operations after it add 3 U * 64.

WHAT IS UNDECIDED
  deposit   a rounding floor(x + 0.5) -- the angle bins, the D2 and D3 bins, the ratio bin -- whose x lies within its bound of an integer
            counts in `hi` of every bin it could reach and in `lo` of none. The bounds of the D2 and D3 coordinates contain those of the
            two maxima. The line and triangle classes are integer comparisons of cell counts (the header states the class thresholds on
            counts, not on the ratio): they need no margin once the voxels are decided.
  attempt   H within its bound of 0.001 (Heron's product is ill conditioned for slivers, so the bound is often far wider than H), or a
            cosine within its bound of 1: the attempt may or may not be accepted. It is carried as a MAYBE sample: the samples that are
            in the first n_samples whatever the maybes do count in lo and hi; those that are in it for SOME outcome count in hi only; the
            maxima range over both sets. A flat scene draws slivers all the time and stays checkable this way. Only when the maybes
            decide whether n_samples are reached before the attempt cap is the keypoint undecided as a whole.
  keypoint  undecided as a whole when a scaled coordinate lies within its bound of an integer -31 .. 31 (at +-32 the clamp holds the
            voxel), so that the voxel of a point could differ.
"""
import numpy as np

f32, f64 = np.float32, np.float64
DIM, BINS, GRID = 640, 64, 64
U = 2.0 ** -24
H_MIN = 0.001
PIH32 = f64(f32(np.pi / 2))
ACOS_ERR = 4 * U                  # |acosf(x) - acos(x)|
TAIL_ERR = 3 * U * 64             # the division, the product and the sum after it, on values below 64
SEED = 0x45534631
SAMPLES = 20000
# numerators in sixths: A3 in/out/mixed, D3 in/out/mixed, D2 in/out/mixed, ratio
W_A3, W_D3, W_D2, W_RATIO = 1, (3, 3, 6), (3, 12, 12), 6
IN, OUT, MIXED = 0, 1, 2


def hash32(seed, x):
    """h(seed, x) of the header, on uint64 arrays"""
    M = np.uint64(0xffffffff)
    v = (np.asarray(x, np.uint64) * np.uint64(0x9E3779B1) + np.uint64(seed)) & M
    v ^= v >> np.uint64(16); v = (v * np.uint64(0x7FEB352D)) & M
    v ^= v >> np.uint64(15); v = (v * np.uint64(0x846CA68B)) & M
    v ^= v >> np.uint64(16)
    return v


def draws(seed, t, n):
    """the three indices of the attempts t [T] into a ball of n points -> [T, 3]"""
    x = np.uint64(3) * np.asarray(t, np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :]
    return ((hash32(seed, x) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def ball(P, q, radius):
    """ascending indices of the finite rows of P [n, 3] with d2 < (float)((double)R * R), d2 in float32 as every sweep of the library"""
    P = np.asarray(P, f32).reshape(-1, 3); q = np.asarray(q, f32)
    if not np.isfinite(q).all():
        return np.zeros(0, np.int64)
    r2 = f32(f64(f32(radius)) * f64(f32(radius)))
    with np.errstate(invalid="ignore", over="ignore"):
        d = P - q[None, :]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return np.nonzero(np.isfinite(P).all(1) & (d2 < r2))[0]


# ------------------------------------------------------------------------------------------------------ values with error bounds
class _Q:
    """value (float64) and bound of |float32 result - value|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, f64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, f64)

    def _rounded(self, v, e):
        with np.errstate(over="ignore", invalid="ignore"):
            exact = (e == 0) & (v.astype(f32).astype(f64) == v)
        return _Q(v, np.where(exact, 0.0, e + U * (np.abs(v) + e)))

    def __add__(self, o): return self._rounded(self.v + o.v, self.e + o.e)
    def __sub__(self, o): return self._rounded(self.v - o.v, self.e + o.e)
    def __mul__(self, o): return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        with np.errstate(divide="ignore", invalid="ignore"):
            den = np.maximum(np.abs(o.v) - o.e, 0.0)
            v = self.v / o.v
            e = np.where(den > 0, (self.e + np.abs(v) * o.e) / den, np.inf)
            e = np.where((self.e == 0) & (o.e == 0), 0.0, e)
        return self._rounded(v, e)

    def sqrt(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.sqrt(np.maximum(self.v, 0.0))
            lo = np.sqrt(np.maximum(self.v - self.e, 0.0))
            e = np.where(self.e == 0, 0.0, np.maximum(np.sqrt(self.v + self.e) - v, v - lo))
        return self._rounded(v, e)

    def abs(self): return _Q(np.abs(self.v), self.e)


def scaled64(P, c, m):
    """g = (p - c) * (32 / m) with its bound -> _Q [n, 3]"""
    s = _Q(f64(32.0)) / _Q(f64(f32(m)))
    return (_Q(np.asarray(P, f32).astype(f64)) - _Q(np.asarray(c, f32).astype(f64)[None, :])) * _Q(s.v[None, None], s.e[None, None])


def cells(g):
    """step 4 for an array of scaled coordinates (any float type) -> int64 cells 0..63"""
    g = np.asarray(g)
    v = np.where(g < 0, np.floor(g) + 32, np.ceil(g) + 31)
    return np.clip(v, 0, GRID - 1).astype(np.int64)


def occupancy(vox):
    """the 64^3 bit set of the voxels vox [n, 3]: every point sets v + {-1, 0, 1}^3 inside the grid"""
    occ = np.zeros((GRID, GRID, GRID), bool)
    off = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3)
    c = (vox[:, None, :] + off[None, :, :]).reshape(-1, 3)
    c = c[((c >= 0) & (c < GRID)).all(1)]
    occ[c[:, 0], c[:, 1], c[:, 2]] = True
    return occ


def walk(occ, va, vb):
    """PCL's lci for the lines va -> vb [k, 3]: (visited [k], inside [k]). The driving axis is the longest (ties x, y, z), L its length;
    the cells at steps 0 .. max(L, 1) - 1 are visited."""
    va = np.asarray(va, np.int64); vb = np.asarray(vb, np.int64)
    k = len(va)
    d = vb - va
    ad = np.abs(d)
    inc = np.where(d < 0, -1, 1)
    drive = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where((ad[:, 1] >= ad[:, 0]) & (ad[:, 1] >= ad[:, 2]), 1, 2))
    L = ad[np.arange(k), drive]
    err = 2 * ad - L[:, None]
    is_drive = np.arange(3)[None, :] == drive[:, None]
    cur = va.copy()
    inside = np.zeros(k, np.int64)
    for i in range(1, int(L.max()) if k else 0):
        act = i < L
        inside += act & occ[cur[:, 0], cur[:, 1], cur[:, 2]]
        step = act[:, None] & (is_drive | (err > 0))
        cur += np.where(step, inc, 0)
        err = np.where(act[:, None] & ~is_drive & (err > 0), err - 2 * L[:, None], err)
        err = np.where(act[:, None], err + 2 * ad, err)
    inside += occ[cur[:, 0], cur[:, 1], cur[:, 2]]
    return np.maximum(L, 1), inside


def line_class(visited, inside):
    return np.where(inside >= visited - 1, IN, np.where(inside <= 7, OUT, MIXED))


def triangle_class(visited, inside):
    """from [k, 3] counts"""
    si, sv = inside.sum(1), visited.sum(1)
    return np.where(si <= 21, OUT, np.where(sv - si < 4, IN, MIXED))


PAIRS = ((0, 1), (2, 1), (2, 0))          # (v21, v31), (v23, v31), (v23, v21) in the order a, b, c of the sides


def _sides(take):
    """v21, v31, v23 as lists of three coordinate arrays; take(k, a): coordinate a of the attempts' k-th point"""
    p = [[take(k, a) for a in range(3)] for k in range(3)]
    return [[p[1][a] - p[0][a] for a in range(3)], [p[2][a] - p[0][a] for a in range(3)], [p[1][a] - p[2][a] for a in range(3)]]


# ------------------------------------------------------------------------------------------------------ the float32 transcription
def esf32(P, c, m, n_samples, seed=SEED):
    """steps 3 to 8 in float32, every operation rounded, in the header's written order (numpy's arccos for acosf) -> dict(nan, counts [640],
    accepted (attempt numbers), tri [S] and line [S, 3] classes). The check of the margins, and of the scenes' claims."""
    P = np.asarray(P, f32).reshape(-1, 3); c = np.asarray(c, f32); m = f32(m)
    n = len(P)
    out = dict(nan=True, counts=np.zeros(DIM, np.int64), accepted=np.zeros(0, np.int64), tri=np.zeros(0, np.int64), line=np.zeros((0, 3), np.int64))
    with np.errstate(all="ignore"):
        s = f32(32.0) / m
        if n < 3 or not (m > 0 and np.isfinite(m) and np.isfinite(s)):
            return out
        g = (P - c[None, :]) * s
        vox = cells(g)
        occ = occupancy(vox)
        t = np.arange(8 * n_samples, dtype=np.int64)
        idx = draws(seed, t, n)
        V = _sides(lambda k, a: g[idx[:, k], a])
        ln = [np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) for v in V]
        s_ = ((ln[0] + ln[1]) + ln[2]) * f32(0.5)
        H = ((s_ * (s_ - ln[0])) * (s_ - ln[1])) * (s_ - ln[2])
        Un = [[v[a] / ln[k] for a in range(3)] for k, v in enumerate(V)]
        ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & (H > f32(H_MIN)) & np.isfinite(H)
        th = []
        for i, j in PAIRS:
            dot = (Un[i][0] * Un[j][0] + Un[i][1] * Un[j][1]) + Un[i][2] * Un[j][2]
            x = np.floor(np.arccos(np.abs(dot)).astype(f32) / f32(PIH32) * f32(63.0) + f32(0.5))
            ok &= (x >= 0) & (x <= 63)
            th.append(np.where(np.isfinite(x), x, 0).astype(np.int64))
        acc = np.nonzero(ok)[0][:n_samples]
        if len(acc) < n_samples:
            return out
        idx = idx[acc]
        ends = ((0, 1), (0, 2), (1, 2))
        vis = np.zeros((n_samples, 3), np.int64); ins = np.zeros((n_samples, 3), np.int64)
        for e, (i, j) in enumerate(ends):
            vis[:, e], ins[:, e] = walk(occ, vox[idx[:, i]], vox[idx[:, j]])
        lc = line_class(vis, ins)
        tc = triangle_class(vis, ins)
        counts = out["counts"]
        for e in range(3):
            np.add.at(counts, tc * BINS + th[e][acc], W_A3)
        d3 = np.sqrt(np.sqrt(H[acc]))
        b3 = np.floor(d3 / d3.max() * f32(63.0) + f32(0.5)).astype(np.int64)
        np.add.at(counts, (3 + tc) * BINS + b3, np.asarray(W_D3)[tc])
        d = np.stack([ln[0][acc], ln[1][acc], ln[2][acc]], 1)
        b2 = np.floor(d / d.max() * f32(63.0) + f32(0.5)).astype(np.int64)
        np.add.at(counts, (6 + lc) * BINS + b2, np.asarray(W_D2)[lc])
        mixed = lc == MIXED
        ratio = ins[mixed].astype(f32) / vis[mixed].astype(f32)
        np.add.at(counts, 9 * BINS + np.floor(ratio * f32(63.0) + f32(0.5)).astype(np.int64), W_RATIO)
    out.update(nan=False, accepted=acc, tri=tc, line=lc)
    return out


# ------------------------------------------------------------------------------------------------------ the float64 restatement
def _deposit(lo, hi, base, xlo, xhi, weight, certain):
    """floor(x + 0.5) deposits: x in [xlo, xhi] (already with the 0.5), bins clipped to 0..63"""
    b0 = np.clip(np.floor(xlo), 0, BINS - 1).astype(np.int64); b1 = np.clip(np.floor(xhi), 0, BINS - 1).astype(np.int64)
    weight = np.broadcast_to(weight, b0.shape)
    sure = certain & (b0 == b1)
    np.add.at(lo, base[sure] + b0[sure], weight[sure])
    for k in range(int((b1 - b0).max()) + 1 if len(b0) else 0):
        sel = b0 + k <= b1
        np.add.at(hi, base[sel] + b0[sel] + k, weight[sel])


def esf64(P, c, m, n_samples, seed=SEED):
    """-> dict(nan: the row must be NaN, whole: the keypoint is undecided as a whole, lo, hi [640], maybes: attempts whose acceptance is
    undecided among those that matter, samples: (certain, possible) counts)"""
    P = np.asarray(P, f32).reshape(-1, 3); c = np.asarray(c, f32); m = f32(m)
    n = len(P)
    out = dict(nan=True, whole=False, lo=np.zeros(DIM, np.int64), hi=np.zeros(DIM, np.int64), maybes=0, samples=(0, 0))
    with np.errstate(all="ignore"):
        if n < 3 or not (m > 0 and np.isfinite(m) and np.isfinite(f32(32.0) / m)):
            return out
        g = scaled64(P, c, m)
        r = np.rint(g.v)
        if ((np.abs(g.v - r) <= g.e) & (np.abs(r) <= 31) & (g.e > 0)).any() or not np.isfinite(g.e).all():
            out.update(nan=False, whole=True)
            return out
        vox = cells(g.v)
        occ = occupancy(vox)
        t = np.arange(8 * n_samples, dtype=np.int64)
        idx = draws(seed, t, n)
        V = _sides(lambda k, a: _Q(g.v[idx[:, k], a], g.e[idx[:, k], a]))
        ln = [((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).sqrt() for v in V]
        s_ = ((ln[0] + ln[1]) + ln[2]) * _Q(f64(0.5))
        H = ((s_ * (s_ - ln[0])) * (s_ - ln[1])) * (s_ - ln[2])
        distinct = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
        yes = distinct & (H.v - H.e > H_MIN) & np.isfinite(H.v)
        no = ~distinct | (H.v + H.e <= H_MIN)
        no |= ~np.isfinite(H.v) & (H.e == 0)
        Un = [[v[a] / ln[k] for a in range(3)] for k, v in enumerate(V)]
        xs = []
        for i, j in PAIRS:
            dot = ((Un[i][0] * Un[j][0] + Un[i][1] * Un[j][1]) + Un[i][2] * Un[j][2]).abs()
            yes &= dot.v + dot.e <= 1.0                                  # above 1 acosf gives a NaN and the attempt is rejected
            no |= distinct & (dot.v - dot.e > 1.0)
            th = np.arccos(np.minimum(dot.v, 1.0))
            sin = np.sqrt(np.maximum(1.0 - dot.v * dot.v, 0.0))
            eth = 2.0 * dot.e / np.maximum(sin, np.sqrt(dot.e)) + ACOS_ERR
            eth = np.where(dot.e == 0, ACOS_ERR, eth)
            xs.append((th / PIH32 * 63.0 + 0.5, eth / PIH32 * 63.0 + TAIL_ERR))
        yes &= ~no
        maybe = ~yes & ~no
        # the samples: certainly among the first n_samples / possibly among them
        rank_all = np.cumsum(yes | maybe) - (yes | maybe)
        rank_yes = np.cumsum(yes) - yes
        certain = yes & (rank_all < n_samples)
        possible = (yes | maybe) & (rank_yes < n_samples)
        if yes.sum() < n_samples:
            if (yes | maybe).sum() < n_samples:
                return out                                               # the attempt cap is reached whatever the maybes do
            out.update(nan=False, whole=True)
            return out
        out["nan"] = False
        out["maybes"] = int((maybe & possible).sum())
        out["samples"] = (int(certain.sum()), int(possible.sum()))
        if not certain.any():
            out["whole"] = True
            return out
        sel = np.nonzero(possible)[0]
        cert = certain[sel]
        idx = idx[sel]
        ends = ((0, 1), (0, 2), (1, 2))
        k = len(sel)
        vis = np.zeros((k, 3), np.int64); ins = np.zeros((k, 3), np.int64)
        for e, (i, j) in enumerate(ends):
            vis[:, e], ins[:, e] = walk(occ, vox[idx[:, i]], vox[idx[:, j]])
        lc = line_class(vis, ins)
        tc = triangle_class(vis, ins)
        lo, hi = out["lo"], out["hi"]
        for x, ex in xs:
            _deposit(lo, hi, tc * BINS, x[sel] - ex[sel], x[sel] + ex[sel], W_A3, cert)
        # D3 and D2: value / maximum * 63 + 0.5, the maximum between that of the certain samples and that of the possible ones
        def scaled(val, err, cert_rows):
            vmax_lo = (val - err)[cert_rows].max(); vmax_hi = (val + err).max()
            xlo = np.maximum(val - err, 0.0) / vmax_hi * 63.0 + 0.5 - TAIL_ERR
            xhi = np.minimum((val + err) / max(vmax_lo, 1e-300), 1.0) * 63.0 + 0.5 + TAIL_ERR
            return xlo, xhi
        Hs = _Q(np.maximum(H.v[sel], 0.0), H.e[sel])
        d3 = Hs.sqrt().sqrt()
        xlo, xhi = scaled(d3.v, np.where(np.isfinite(d3.e), d3.e, 1e30), cert)
        _deposit(lo, hi, (3 + tc) * BINS, xlo, xhi, np.asarray(W_D3)[tc], cert)
        dv = np.stack([ln[e].v[sel] for e in range(3)], 1); de = np.stack([ln[e].e[sel] for e in range(3)], 1)
        xlo, xhi = scaled(dv, de, cert)
        for e in range(3):
            _deposit(lo, hi, (6 + lc[:, e]) * BINS, xlo[:, e], xhi[:, e], np.asarray(W_D2)[lc[:, e]], cert)
        mixed = lc == MIXED
        ratio = ins[mixed] / vis[mixed] * 63.0 + 0.5
        cm = np.broadcast_to(cert[:, None], lc.shape)[mixed]
        _deposit(lo, hi, np.full(len(ratio), 9 * BINS), ratio - TAIL_ERR, ratio + TAIL_ERR, W_RATIO, cm)
    return out


# ------------------------------------------------------------------------------------------------------ the scale (step 3)
def scale_model(P, q, radius):
    """(c [3] float32, m float32) as the header defines them, for the host tests that have no device: c = (float)(q + mean(p - q)) with
    the mean in float64 (the device's fixed point differs from it by less than the bound below), m in float32 operations"""
    P = np.asarray(P, f32).reshape(-1, 3); q = np.asarray(q, f32)
    c = (q.astype(f64) + (P.astype(f64) - q.astype(f64)[None, :]).mean(0)).astype(f32)
    d = P - c[None, :]
    m = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
    return c, f32(m)


def scale_bounds(P, q, radius, c_dev):
    """-> (c64 [3], c_err [3], m64, m_err): the centroid in float64 with the bound of the order-free sum -- every term is rounded to a
    quantum of at most 2^(e - 40), 2^e the power of two above 2 R, so the mean moves by at most half a quantum, and the result is rounded
    to float32 once (half a unit in the last place) -- and the largest distance from the DEVICE's centroid in float64 with the bound of
    its float32 evaluation: a rounded difference, three products, two sums and a square root, 4 U relative."""
    P = np.asarray(P, f32).reshape(-1, 3).astype(f64); q = np.asarray(q, f32).astype(f64)
    c64 = q + (P - q[None, :]).mean(0)
    quantum = 2.0 ** (np.frexp(f64(f32(radius)))[1] + 1 - 40)
    c_err = 0.5 * np.spacing(np.abs(c64).astype(f32)).astype(f64) * (1 + 2 * U) + quantum
    d = P - np.asarray(c_dev, f32).astype(f64)[None, :]
    m64 = np.sqrt((d * d).sum(1)).max()
    return c64, c_err, m64, 4 * U * m64


def esf_local(pt_off, xyz, kp_off, kp, radius, n_samples, seed=SEED, scale=None):
    """the batch: per keypoint the ball, then esf64 on the device's scale (scale [K, 4]; None: scale_model) -> dict(cnt [K], nan [K],
    whole [K], lo, hi [K, 640], scale [K, 4] as used, balls: list of index arrays, maybes [K])"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3); kp = np.asarray(kp, f32).reshape(-1, 3)
    K = len(kp)
    out = dict(cnt=np.zeros(K, np.int64), nan=np.ones(K, bool), whole=np.zeros(K, bool), lo=np.zeros((K, DIM), np.int64),
               hi=np.zeros((K, DIM), np.int64), scale=np.full((K, 4), np.nan, f32), balls=[None] * K, maybes=np.zeros(K, np.int64))
    for o in range(len(pt_off) - 1):
        P = xyz[pt_off[o]:pt_off[o + 1]]
        for k in range(int(kp_off[o]), int(kp_off[o + 1])):
            b = ball(P, kp[k], radius)
            out["cnt"][k] = len(b); out["balls"][k] = b + int(pt_off[o])
            if len(b) < 3:
                continue
            if scale is None:
                c, m = scale_model(P[b], kp[k], radius)
            else:
                c, m = np.asarray(scale[k, :3], f32), f32(scale[k, 3])
            out["scale"][k] = [c[0], c[1], c[2], m]
            a = esf64(P[b], c, m, n_samples, seed)
            out["nan"][k], out["whole"][k], out["lo"][k], out["hi"][k], out["maybes"][k] = a["nan"], a["whole"], a["lo"], a["hi"], a["maybes"]
    return out

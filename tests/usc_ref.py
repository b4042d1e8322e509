"""Float64 restatement of ismhip_point_density / ismhip_usc_tables / ismhip_usc as include/ismhip.h defines them, with the bounds that say
which of its decisions a float32 / libm implementation may take differently.

What is EXACT here, because the definition fixes the float32 operations and numpy performs the same IEEE operations in the same order:
  * ball and density membership: d2 = ((dx*dx) + dy*dy) + dz*dz in float32 from float32 differences, d2 < (float)((double)r * r);
  * the skip rule and everything up to the arguments of acos / atan2: products and sums of float32 values widened to double, sqrt and
    division are correctly rounded operations, so r, z.v, the clamped cosine, |x cross u| and x.u carry the device's own bits;
  * the deposits q_p and their integer sums.
What is NOT pinned to the bit: acos and atan2 (libm against the device's, each within a few double ulps: ANGLE_EPS = 1e-9 degrees is
seven orders above that and eight below a bin), and the radial edges (exp / log of the host against numpy, then rounded to float32:
EDGE_REL = 2^-22, four float32 ulps). A ball point whose theta, phi or r lies within its bound of a bin edge is UNDECIDED: it may sit on
either side. describe() returns, per keypoint, `decided` (no such point) and per bin the interval [q_lo, q_hi]: q_lo counts the decided
points of the bin, q_hi adds every undecided point to each bin it may fall in. On a decided keypoint q_lo == q_hi == Q."""
import numpy as np

F = np.float32
NA, NE, NR = 14, 14, 10
DIM = NA * NE * NR
FLT_EPSILON = float(np.finfo(F).eps)
ANGLE_EPS = 1e-9                 # degrees
EDGE_REL = 2.0 ** -22


def tables(radius, min_radius):
    """(lut float64 [10, 14], edges float64 [11], edges float32 [11]) of ismhip_usc_tables"""
    R, rmin = float(F(radius)), float(F(min_radius))
    j = np.arange(NR + 1, dtype=np.float64)
    e = np.exp(np.log(rmin) + (j / NR) * np.log(R / rmin))
    k = np.arange(NE + 1, dtype=np.float64)
    c = np.cos(k * np.pi / NE)
    # e^3 as the library multiplies it out: e * e * e
    vol = (c[:-1] - c[1:])[None, :] * ((e[1:] * e[1:] * e[1:] - e[:-1] * e[:-1] * e[:-1]))[:, None] / 3.0 * (2.0 * np.pi / NA)
    return 1.0 / np.cbrt(vol), e, e.astype(F)


def _r2(radius):
    return F(np.float64(F(radius)) * np.float64(F(radius)))


def _d2(p, c):
    """float32, in sqdist3's order"""
    d = (p - c).astype(F)
    return ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], d


def density(pt_off, xyz, radius):
    xyz = np.asarray(xyz, F)
    out = np.zeros(len(xyz), np.int64)
    r2 = _r2(radius)
    for o in range(len(pt_off) - 1):
        s, e = int(pt_off[o]), int(pt_off[o + 1])
        p = xyz[s:e]
        fin = np.isfinite(p).all(1)
        pf = p[fin]
        cnt = np.zeros(len(p), np.int64)
        idx = np.nonzero(fin)[0]
        for i in idx:
            d2, _ = _d2(pf, p[i])
            cnt[i] = int((d2 < r2).sum())
        out[s:e] = cnt
    return out


def deposit(n):
    n = max(int(n), 1)
    return (2 ** 32 + n // 2) // n


def _bin_candidates(value, uppers, eps):
    """the first bin whose upper edge is not below value (the last bin beyond every edge), and the set of bins it may be within eps"""
    n = len(uppers) + 1                                  # uppers: the first n - 1 upper edges; the last bin has none
    b = n - 1
    for t in range(n - 1):
        if value <= uppers[t]:
            b = t
            break
    cand = {b}
    for t in range(n - 1):
        if abs(value - uppers[t]) <= eps[t]:
            cand.update((t, t + 1))
    return b, sorted(cand)


def describe(pt_off, xyz, kp_off, kp, lrf, radius, min_radius, dens):
    xyz, kp, lrf = np.asarray(xyz, F), np.asarray(kp, F), np.asarray(lrf, F).reshape(-1, 9)
    lut, _, e32 = tables(radius, min_radius)
    r_up = e32[1:NR].astype(np.float64)
    th_up = np.arange(1, NE, dtype=np.float64) * (180.0 / NE)
    ph_up = np.arange(1, NA, dtype=np.float64) * (360.0 / NA)
    r_eps, th_eps, ph_eps = r_up * EDGE_REL, np.full(NE - 1, ANGLE_EPS), np.full(NA - 1, ANGLE_EPS)
    nkp = len(kp)
    q_lo = np.zeros((nkp, DIM), np.int64); q_hi = np.zeros((nkp, DIM), np.int64)
    decided = np.ones(nkp, bool); nan_row = np.zeros(nkp, bool); count = np.zeros(nkp, np.int64); skipped = np.zeros(nkp, np.int64)
    r2 = _r2(radius)
    deg = 57.29577951308232
    for o in range(len(pt_off) - 1):
        s, e = int(pt_off[o]), int(pt_off[o + 1])
        p = xyz[s:e]
        fin = np.isfinite(p).all(1)
        pf, nf = p[fin], np.asarray(dens[s:e])[fin]
        for k in range(int(kp_off[o]), int(kp_off[o + 1])):
            if not (np.isfinite(kp[k]).all() and np.isfinite(lrf[k]).all()) or len(pf) == 0:
                nan_row[k] = True
                continue
            d2, d = _d2(pf, kp[k])
            inside = d2 < r2
            count[k] = int(inside.sum())
            if count[k] == 0:
                nan_row[k] = True
                continue
            x, z = lrf[k, 0:3].astype(np.float64), lrf[k, 6:9].astype(np.float64)
            for v32, n_p in zip(d[inside], nf[inside]):
                v = v32.astype(np.float64)
                n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                if n2 <= FLT_EPSILON:
                    skipped[k] += 1
                    continue
                r = np.sqrt(n2)
                zv = (z[0] * v[0] + z[1] * v[1]) + z[2] * v[2]
                c = min(1.0, max(-1.0, zv / r))
                theta = float(np.arccos(c)) * deg
                u = v - zv * z
                phi = 0.0
                if not (u[0] == 0.0 and u[1] == 0.0 and u[2] == 0.0):
                    cr = np.array([x[1] * u[2] - x[2] * u[1], x[2] * u[0] - x[0] * u[2], x[0] * u[1] - x[1] * u[0]])
                    cn = np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
                    xu = (x[0] * u[0] + x[1] * u[1]) + x[2] * u[2]
                    phi = float(np.arctan2(cn, xu)) * deg
                    if (cr[0] * z[0] + cr[1] * z[1]) + cr[2] * z[2] < 0.0:
                        phi = 360.0 - phi
                j, cj = _bin_candidates(r, r_up, r_eps)
                kk, ck = _bin_candidates(theta, th_up, th_eps)
                l, cl = _bin_candidates(phi, ph_up, ph_eps)
                q = deposit(n_p)
                if len(cj) == len(ck) == len(cl) == 1:
                    q_lo[k, l * (NE * NR) + kk * NR + j] += q
                    q_hi[k, l * (NE * NR) + kk * NR + j] += q
                else:
                    decided[k] = False
                    for a in cl:
                        for b in ck:
                            for g in cj:
                                q_hi[k, a * (NE * NR) + b * NR + g] += q
    return dict(q_lo=q_lo, q_hi=q_hi, decided=decided, nan_row=nan_row, count=count, skipped=skipped, lut=lut)


def row_from_q(Q, lut):
    """(float)((double)Q * 2^-32 * lut[j, k]) for the bins i = l * 140 + k * 10 + j"""
    i = np.arange(DIM)
    return (np.asarray(Q, np.float64) * 2.0 ** -32 * lut[i % NR, (i // NR) % NE]).astype(F)

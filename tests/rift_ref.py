"""float64 numpy restatement of the RIFT descriptor as this library defines it (include/ismhip.h:
ismhip_intensity_gradients, ismhip_rift), one object at a time. It is the checker of tests/test_gpu_rift.py and is itself checked against
hand-derived answers in tests/test_rift_cpu.py.

Intensities come from the library's float formula and ball membership from its float rule (unfused d2 = (dx*dx + dy*dy) + dz*dz strictly
below (float)((double)r * r)), both exactly; everything else is float64, taken the plain way (two passes about the ball's means, numpy's
eigh and arctan2), not the device's way.

Tolerances, derived here. Notation: n ball points, r the radius, bits = grid_bits(n_points) the width of the device's integer grids.

Gradient. The device rounds every moment term to a quantum and adds integers: per entry of A the sum of products is off by at most
n * 2^(e2 - bits) / 2 <= n r^2 2^-bits (2^e2 <= 2 r^2), the centring term (sum d)(sum d)^T / n by at most 2 n r^2 2^-bits (|sum d| <= n r,
each component sum off by n r 2^-bits), double rounding adds below n r^2 2^-50; so |dA|_2 <= 3 * 3.2 n r^2 2^-bits <= 10 n r^2 2^-bits.
Per entry of b: n r 2^(8 - bits) from the products (|d dI| < 2^(e1 + 8), 2^e1 <= 2 r) and 1.5 n r 2^(8 - bits) from the centring, so
|db|_2 <= 4.4 n r 2^(8 - bits). First order, |dx| <= (|dA|_2 |x| + |db|_2) / lambda_min over the kept eigenvalues, and the tilt of the
kept subspace of a rank-deficient A costs as much again: a factor 2. With lambda_max / lambda_min <= KAPPA_MAX and n r^2 / lambda_max <=
SPREAD_MAX (points beyond either bound are undecided), n r^2 / lambda_min <= COND = KAPPA_MAX * SPREAD_MAX and
    |g_dev - g_ref|_inf <= GRAD_REL * |x| + grad_abs(r),
    GRAD_REL = 2^-23 + 2 * COND * 10 * 2^-bits      (2^-23: the float store of the three components, |g_c| <= 1.0000002 |x|)
    grad_abs(r) = 2 * COND * 4.4 * 2^(8 - bits) / r
(the projection g = x - n (n . x) with a float normal, |n| within 1e-6 of 1, does not lengthen dx by more than that). With bits = 48:
GRAD_REL = 1.7e-7 and grad_abs(0.1) = 5.1e-5 intensity units per length, 2e-7 of the scenes' gradients. The same SPREAD_MAX keeps the
device's noise eigenvalue of a rank-deficient A, at most 3 * 3.2 n r^2 2^-bits / lambda_max <= 7e-13 of the largest, under the 1e-12 cut.
This restatement's own error (two passes in float64, eigh) is about KAPPA_MAX * 1e-15.

Row. The device evaluates distance, angle and weights in float. Against float64 on the same float inputs:
  d = nd dist / (r + eps): u = p - p0 rounds each component (2^-24 relative), so d2 is within 5 * 2^-24, dist within 3.5 * 2^-24 with the
    root's own rounding, d within 5.5 * 2^-24 after the product and the quotient: DELTA_D = 5.5 * 2^-24 * nd;
  angle = atan2(|g x u|, g . u): a cross component a b - c d is off by at most 5 * 2^-24 |g||u| (two rounded factors, two products, one
    difference), the norm of the cross product by sqrt(3) times that plus 2.5 * 2^-24 of itself, the dot product by 8 * 2^-24 |g||u|;
    the two errors move the angle by at most sqrt(11.2^2 + 8^2) * 2^-24 = 13.8 * 2^-24 = 8.2e-7 rad; shot_atan2 adds 2e-8 (its
    polynomial) and about 3e-7 (its float evaluation up to pi): ANGLE_ERR = 1.15e-6 rad; a = ng angle / (pi + eps) adds two roundings of
    a <= ng: DELTA_A = ng * (ANGLE_ERR / pi + 2.5 * 2^-24);
  the deposit (wd wa) mag: each factor and each product rounds once, mag = sqrtf of three squared floats: DEP_REL = 6 * 2^-24;
  fixed point: a deposit enters as round(v 2^(40 - eg)), 2^eg the power of two above the object's largest |g|: 2^(eg - 41) each.
A bin b of the raw histogram h therefore differs by at most
    dh_b = DELTA_D * Ha_b + DELTA_A * Hd_b + DEP_REL * h_b + n_b 2^(eg - 41) + Hg_b
where Ha_b (Hd_b) sums mag_j times the angle (distance) weight alone over the ball points whose distance (angle) coordinate lies within
1 + 1e-4 of the bin, n_b counts them, and Hg_b = sum gerr_j (1 + ng / pi) over the same points carries a bound gerr_j on the error of the
gradients themselves (zero when both sides read the same array). After the division by N = |h|_2:
    |row_dev - row_ref|_b <= (dh_b + row_b |dh|_2) / N * (1 + 1e-6) + 2^-24 row_b,
capped at the project's descriptor tolerance 1e-4 (a cap only tightens the check)."""
import numpy as np
from scipy.spatial import cKDTree

from prefilter_ref import finite, sqd32

MARGIN = 1e-6            # relative distance of d2 from the ball boundary inside which a neighbour makes its query undecided
CUT = 1e-12              # D2: eigenvalues at or below CUT * lambda_max are left out of the pseudo-inverse
KAPPA_MAX = 1e4          # lambda_max / lambda_min over the kept eigenvalues
SPREAD_MAX = 64.0        # n r^2 / lambda_max
COND = KAPPA_MAX * SPREAD_MAX
ROW_TOL_MAX = 1e-4       # the project's descriptor tolerance on a unit-norm row
ANGLE_ERR = 1.15e-6
DEP_REL = 6.0 * 2.0 ** -24
FLT_EPS = np.float32(np.finfo(np.float32).eps)


def grid_bits(n_points, most=48):
    bits = most
    while bits > 24 and n_points + 1 >= 1 << (62 - bits):
        bits -= 1
    return bits


def grad_rel(n_points=0):
    return 2.0 ** -23 + 2.0 * COND * 10.0 * 2.0 ** -grid_bits(n_points)


def grad_abs(radius, n_points=0):
    return 2.0 * COND * 4.4 * 2.0 ** (8 - grid_bits(n_points)) / float(np.float32(radius))


def r2_of(radius):
    return np.float32(np.float64(np.float32(radius)) * np.float64(np.float32(radius)))


def intensity(rgba):
    """PointCloudXYZRGBtoXYZI in float, unfused: (0.299f R + 0.587f G) + 0.114f B"""
    c = np.asarray(rgba).astype(np.int64)
    R, G, B = (((c >> s) & 0xff).astype(np.float32) for s in (16, 8, 0))
    return ((np.float32(0.299) * R).astype(np.float32) + (np.float32(0.587) * G).astype(np.float32)).astype(np.float32) + \
        (np.float32(0.114) * B).astype(np.float32)


def balls(p, q, radius):
    """per query of q the ascending indices of the points of p (finite float32 [n, 3]) with d2 < r2, and whether one of the shortlisted
    points lies within MARGIN of the boundary"""
    r2 = r2_of(radius)
    out, near = [], np.zeros(len(q), bool)
    if not len(p) or not len(q):
        return [np.zeros(0, np.int64) for _ in range(len(q))], near
    tree = cKDTree(p.astype(np.float64))
    lists = tree.query_ball_point(q.astype(np.float64), float(np.float32(radius)) * 1.001 + 1e-12)
    for i, l in enumerate(lists):
        l = np.sort(np.asarray(l, np.int64))
        d2 = sqd32(p[l], q[i][None, :]) if len(l) else np.zeros(0, np.float32)
        near[i] = bool((np.abs(d2.astype(np.float64) - float(r2)) <= MARGIN * float(r2)).any())
        out.append(l[d2 < r2])
    return out, near


def gradients(xyz, normals, rgba, radius):
    """-> dict over all points of the object: grad float64 [n, 3] (NaN where the definition says so and at points that are not finite),
    x float64 [n, 3] (the solution before the projection), count int64 [n], undecided bool [n], near bool [n], ratio float64 [n] (smallest
    over largest eigenvalue of A, NaN without a solve)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3); normals = np.asarray(normals, np.float32).reshape(-1, 3)
    n_all = len(xyz)
    fin = finite(xyz) if n_all else np.zeros(0, bool)
    p = xyz[fin]; nrm = normals[fin].astype(np.float64); inten = intensity(np.asarray(rgba)[fin]).astype(np.float64)
    n = len(p)
    r2 = float(r2_of(radius))
    g = np.full((n, 3), np.nan); xs = np.full((n, 3), np.nan); cnt = np.zeros(n, np.int64); und = np.zeros(n, bool); ratio = np.full(n, np.nan)
    nb, near = balls(p, p, radius)
    p64 = p.astype(np.float64)
    for i in range(n):
        l = nb[i]
        cnt[i] = len(l)
        und[i] = near[i]
        if cnt[i] < 3 or not np.isfinite(nrm[i]).all():
            continue
        d = p64[l] - p64[l].mean(0)
        di = inten[l] - inten[l].mean()
        A = d.T @ d
        b = d.T @ di
        w, V = np.linalg.eigh(A)
        x = np.zeros(3)
        if w[2] > 0:
            keep = w > CUT * w[2]
            rel = np.abs(w) / w[2]
            und[i] |= bool(((rel >= CUT * 1e-2) & (rel <= CUT * 1e2)).any())
            und[i] |= bool(w[2] / w[keep].min() > KAPPA_MAX) or bool(cnt[i] * r2 / w[2] > SPREAD_MAX)
            ratio[i] = w[0] / w[2]
            for k in np.nonzero(keep)[0]:
                x += V[:, k] * (V[:, k] @ b) / w[k]
        xs[i] = x
        g[i] = x - nrm[i] * (nrm[i] @ x)
    out = dict(grad=np.full((n_all, 3), np.nan), x=np.full((n_all, 3), np.nan), count=np.zeros(n_all, np.int64), undecided=np.zeros(n_all, bool),
               near=np.zeros(n_all, bool), ratio=np.full(n_all, np.nan))
    out["grad"][fin] = g; out["x"][fin] = xs; out["count"][fin] = cnt; out["undecided"][fin] = und; out["near"][fin] = near; out["ratio"][fin] = ratio
    return out


def grad_tol(x, radius, n_points=0):
    """the bound on |g_dev - g_ref|_inf per point, from the solutions x [n, 3]"""
    return grad_rel(n_points) * np.linalg.norm(x, axis=1) + grad_abs(radius, n_points)


def rift(xyz, grad, kp, radius, nd=8, ng=16, undecided_points=None, gerr=None):
    """xyz float32 [n, 3], grad float32 [n, 3] (the array the device reads), kp float32 [k, 3] -> dict: rows float64 [k, nd * ng], count
    int64 [k], undecided bool [k], tol float64 [k, nd * ng] (docstring above), amp float64 [k] (the largest derived bound of the row before
    the cap). undecided_points: the gradient pass's flags [n]; gerr: a bound on the error of every gradient [n]"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3); grad = np.asarray(grad, np.float32).reshape(-1, 3); kp = np.asarray(kp, np.float32).reshape(-1, 3)
    fin = finite(xyz) if len(xyz) else np.zeros(0, bool)
    p = xyz[fin]; g = grad[fin].astype(np.float64)
    und_p = np.zeros(len(p), bool) if undecided_points is None else np.asarray(undecided_points, bool)[fin]
    ge = np.zeros(len(p)) if gerr is None else np.asarray(gerr, np.float64)[fin]
    D = nd * ng
    K = len(kp)
    rows = np.full((K, D), np.nan); cnt = np.zeros(K, np.int64); und = np.zeros(K, bool); tol = np.full((K, D), ROW_TOL_MAX); amp = np.zeros(K)
    kfin = finite(kp) if K else np.zeros(0, bool)
    nb, near = balls(p, kp[kfin], radius)
    d_scale = float(np.float32(np.float32(radius) + FLT_EPS)); a_scale = float(np.float32(np.float32(np.pi) + FLT_EPS))
    delta_d = 5.5 * 2.0 ** -24 * nd
    delta_a = ng * (ANGLE_ERR / np.pi + 2.5 * 2.0 ** -24)
    mags = np.linalg.norm(g, axis=1)
    okm = np.isfinite(mags)
    eg = int(np.frexp(mags[okm].max())[1]) if okm.any() else 0
    fix = 2.0 ** (eg - 1 - grid_bits(len(p), 40))
    p64 = p.astype(np.float64)
    for kk, k in enumerate(np.nonzero(kfin)[0]):
        l = nb[kk]
        cnt[k] = len(l)
        und[k] = near[kk] or bool(und_p[l].any())
        if not len(l) or not np.isfinite(g[l]).all():
            continue                                                           # D4: the whole row NaN
        h = np.zeros(D); ha = np.zeros(D); hd = np.zeros(D); hg = np.zeros(D); nbin = np.zeros(D)
        u = p64[l] - kp[k].astype(np.float64)
        dist = np.sqrt((u * u).sum(1))
        mag = mags[l]
        angle = np.arctan2(np.linalg.norm(np.cross(g[l], u), axis=1), (g[l] * u).sum(1))   # 0 for mag == 0 and for u == 0
        d = nd * dist / d_scale
        a = ng * angle / a_scale
        # d_idx from max(ceil(d - 1), 0) to min(floor(d + 1), nd - 1), g_idx from ceil(a - 1) to floor(a + 1): the candidates floor + {-1 .. 2};
        # those within 1 deposit, those within 1 + 1e-4 enter the error sums (the device's d and a are off by DELTA_D, DELTA_A)
        for og in (-1, 0, 1, 2):
            gi = np.floor(a) + og
            wa = 1.0 - np.abs(a - gi)
            for od in (-1, 0, 1, 2):
                di = np.floor(d) + od
                wd = 1.0 - np.abs(d - di)
                sup = (wa >= -1e-4) & (wd >= -1e-4) & (di >= 0) & (di <= nd - 1)
                b = (np.mod(gi, ng) * nd + di).astype(np.int64)[sup]               # PCL's copy-out order: gradient-major
                dep = (wa >= 0) & (wd >= 0)
                np.add.at(h, b, np.where(dep, wd * wa * mag, 0.0)[sup])
                np.add.at(ha, b, (np.maximum(wa, 0.0) * mag)[sup]); np.add.at(hd, b, (np.maximum(wd, 0.0) * mag)[sup])
                np.add.at(hg, b, (ge[l] * (1.0 + ng / np.pi))[sup]); np.add.at(nbin, b, 1.0)
        N = np.sqrt((h * h).sum())
        rows[k] = h / N if N > 0 else 0.0
        if N > 0:
            dh = delta_d * ha + delta_a * hd + DEP_REL * h + nbin * fix + hg
            t = (dh + rows[k] * np.sqrt((dh * dh).sum())) / N * (1.0 + 1e-6) + 2.0 ** -24 * rows[k]
            amp[k] = t.max()
            tol[k] = np.minimum(t, ROW_TOL_MAX)
    return dict(rows=rows, count=cnt, undecided=und, tol=tol, amp=amp)

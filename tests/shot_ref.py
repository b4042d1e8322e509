"""SHOT-352 and CSHOT-1344 restated from SURVEY.md Appendix A.2 / A.3 in numpy, accumulating the histogram in float64, with a bound
on what the device's float arithmetic may differ by, per bin of every row.

Written from the appendix (and, for the colour distance, from color_conversion.cpp:85-94 of the reference) and sharing no code with
oracle/ or csrc/: a second reading of the same specification, so that a misreading the oracle and the kernels might share (a sector
bit, a shell test, a modulo) shows up as a disagreement. The inputs of every HARD decision (local coordinates, the cosine, the
squared distance, the colour distance) are float32 values formed as the appendix states, because their exact zeros and ties are what
the boundary tests plant; everything continuous runs in float64. CIELab comes from lab_ref.py.

THE BOUND (u = 2^-24; "1 ulp" of a float operation is taken as a relative error <= 2 u). The kernels (csrc/shot_deposit.h) take the
hard decisions on the same float32 values in the same way, so the device and this file put every deposit into the same bin and differ
only in the deposited values. For one neighbour, with the terms as the kernel forms them:

  cosine      off = fma(5, cos, 5 - step): the exact value rounded once                          e_cos = u |off|
  radial      dist = v_sqrt_f32(d2): 1 ulp (ASSUMED: the guides give no accuracy for v_sqrt_f32 / v_rcp_f32; the ISA manual's figure
              is 1 ulp). r34 = (radius * 3) * 0.25: one rounding; r14, r12: exact; inv_r12 = 1 / r12: one rounding.
              xr = (dist - r34 | r14) * inv_r12                                                   e_r = (2 u d + u r34 [outer]) / r12 + 3 u |xr|
  elevation   ic = zl * v_rcp_f32(dist): 2 u (sqrt) + 2 u (rcp, ASSUMED 1 ulp) + u (product) = 5 u relative. acos is conditioned like
              1 / sqrt(1 - ic^2): the exact effect of that input error is D = the larger of acos(a - 5 u a) - acos(a) and
              acos(a) - acos(min(1, a + 5 u a)), a = |ic|, which tends to sqrt(2 * 5 u) at the poles. shot_acos itself: A&S 4.4.46
              (2e-8) + relative 5.5 u on sqrt(1 - a) * p(a) (u / 2 from 1 - a under the root, 2 u the root, 2 u Horner on
              p in [1, 1.58] whose partial sums total < 2, u the product); for ic < 0 the float pi (|pi_f - pi| = 8.7e-8) and one rounding.
              xe = (inc - C) * (1 / (pi/2)_f), C = (pi/4)_f or (3 pi/4)_f: u C, u |inc - C|, and 3 u |xe| for the constant and the product
                                                                                                  e_e = (D + e_acos + u C + u |inc - C|) (2 / pi) + 3 u |xe|
  azimuth     shot_atan2: q = min * v_rcp(max): 3 u relative, atan' <= 1; z = q^2 one more rounding into p (|p'| <= 1/3); Horner 2 u
              on p in [0.78, 1]; r = q p: u. A&S 4.4.49: 2e-8. Each fix-up pi/2 - r, pi - r that is TAKEN adds the float constant's
              distance from the real one and one rounding.  c = -(7 pi/8)_f + (pi/4)_f sel: u each constant, u the product, u the sum.
              ad = (az - c) * (1 / (pi/4)_f), clamped (1-Lipschitz)                               e_a = (e_atan + e_c + u |az - c|) (4 / pi) + 3 u |ad|
  colour      the offset bc - step_c is the exact value of the kernel's float cd rounded once (u |off|); that cd differs from this
              file's by the CIELab bounds of lab_ref.py on the two colours, (eL + eL' + (ea + ea' + eb + eb') / 2) / 3, plus 8 u for
              its five float operations and the float32 cast of the reference Lab; times 30. Two EQUAL colours give cd = 0 exactly
              on the device as here (x - x = 0): no term.                                         e_col = 30 d_cd + u |off|
  centre      w + winc: the four terms above and 13 u for the float sums 1 - |.| (4 u) and the three additions (2 u + 3 u + 4 u).
  fixed point every deposit is rounded to a multiple of 2^-28: 2^-29 each.

A deposit whose weight lies within its own e of zero may land in the other bin of its pair (or in none) on the device; then both bins
carry the term. E[bin] sums these per bin. With N = |h|_2 the row is h / N, the device's norm differs by at most |E|_2 (triangle
inequality) and 3 u N (float cast of each bin, float cast of the root), so
    |row_dev - row_ref|[i] <= (E[i] + |h[i]| |E|_2 / N) / N * (1 + 2^-10) + 6 u |row[i]|
(6 u: the 3 u of the norm, the float cast of the bin, the float divide, and this file's own cast of the row to float32). Derived, not
measured; no term is scaled to fit."""
import math
from collections import namedtuple

import numpy as np

import lab_ref

f32 = np.float32
PI = np.pi
U = 2.0 ** -24
FIX = 2.0 ** -29
SLACK = 1.0 + 2.0 ** -10
PI_ERR = abs(float(f32(PI)) - PI)
PI2_ERR = abs(float(f32(PI / 2)) - PI / 2)

Row = namedtuple("Row", "desc count bound decided shape shape_bound undecided_neighbours")


def _dot3(ax, ay, az, b):
    """float32 dot product, summed left to right"""
    return ((ax * f32(b[0])).astype(f32) + (ay * f32(b[1])).astype(f32)).astype(f32) + (az * f32(b[2])).astype(f32)


def _acos(v):
    return math.acos(min(1.0, max(-1.0, v)))


def color_distance32(ref, lab):
    """getColorDistance (color_conversion.cpp:85-94) of normalised Lab triples [.., 3], in the float32 operations CSHOT feeds it (A.3)"""
    ref, lab = np.asarray(ref, f32), np.asarray(lab, f32)
    dl, da, db = (np.abs((ref[..., i] - lab[..., i]).astype(f32)) for i in range(3))
    cd = ((dl + ((da + db).astype(f32) / f32(2)).astype(f32)).astype(f32) / f32(3)).astype(f32)
    return np.clip(cd, f32(0), f32(1))


def _finish(h, E):
    n2 = float((h * h).sum())
    if not n2 > 0:
        return np.full(len(h), np.nan, f32), np.full(len(h), np.nan)
    N = math.sqrt(n2)
    row = h / N
    bound = (E + np.abs(h) * (math.sqrt(float((E * E).sum())) / N)) / N * SLACK + 6 * U * np.abs(row)
    return row.astype(f32), bound


def _describe(points, normals, keypoint, frame, radius, rgba=None, kp_rgba=None, lab=lab_ref):
    p = np.asarray(points, f32).reshape(-1, 3)
    nrm = np.asarray(normals, f32).reshape(-1, 3)
    c = np.asarray(keypoint, f32)
    fr = np.asarray(frame, f32).reshape(3, 3)
    color = rgba is not None
    if not (np.isfinite(fr).all() and np.isfinite(c).all()):
        return None, 0
    fin = np.isfinite(p).all(1)
    p, nrm = p[fin], nrm[fin]
    dx, dy, dz = (p[:, 0] - c[0]).astype(f32), (p[:, 1] - c[1]).astype(f32), (p[:, 2] - c[2]).astype(f32)
    d2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)
    r = float(f32(radius))
    inside = d2 < f32(r * r)
    count = int(inside.sum())
    if count < 5:
        return None, count
    dx, dy, dz, d2, nrm = dx[inside], dy[inside], dz[inside], d2[inside], nrm[inside]
    r34, r14, r12 = 3 * r / 4, r / 4, r / 2

    cos = np.clip(_dot3(nrm[:, 0], nrm[:, 1], nrm[:, 2], fr[2]), f32(-1), f32(1))
    d = np.sqrt(d2.astype(np.float64))
    use = np.isfinite(nrm).all(1) & ~(d < 1e-15)
    xl, yl, zl = _dot3(dx, dy, dz, fr[0]), _dot3(dx, dy, dz, fr[1]), _dot3(dx, dy, dz, fr[2])
    xl = np.where(np.abs(xl) < 1e-30, f32(0), xl); yl = np.where(np.abs(yl) < 1e-30, f32(0), yl); zl = np.where(np.abs(zl) < 1e-30, f32(0), zl)

    n_und = 0
    if color:
        col = (np.asarray(rgba).astype(np.uint32).reshape(-1)[fin][inside]) & np.uint32(0xffffff)
        kcol = np.uint32(int(kp_rgba) & 0xffffff)
        uniq, inv = np.unique(np.concatenate([col, [kcol]]), return_inverse=True)
        L = lab.convert(uniq)
        e_lab = L.e_norm + U * np.abs(L.norm)
        cd = color_distance32(L.norm[inv[-1]], L.norm[inv[:-1]]).astype(np.float64)
        e_sum = e_lab[inv[:-1]] + e_lab[inv[-1]]
        d_cd = np.where(col == kcol, 0.0, (e_sum[:, 0] + (e_sum[:, 1] + e_sum[:, 2]) / 2) / 3 + 8 * U)
        bc = cd * 30
        tc = bc + 0.5
        col_dec = (L.decided[inv[:-1]] & L.decided[inv[-1]] & (np.abs(tc - np.rint(tc)) > 30 * d_cd)) | (col == kcol)
        n_und = int((~col_dec & use).sum())

    D = 1344 if color else 352
    h, E = np.zeros(D), np.zeros(D)

    def dep(b, v, e):
        h[b] += v; E[b] += e + FIX

    for i in np.nonzero(use)[0]:
        x, y, z, di = float(xl[i]), float(yl[i]), float(zl[i]), float(d[i])
        b = (1.0 + float(cos[i])) * 10 / 2
        bit4 = 1 if (y > 0 or (y == 0 and x < 0)) else 0
        bit3 = (1 - bit4) if (x > 0 or (x == 0 and y > 0)) else bit4
        s = ((bit4 << 3) + (bit3 << 2)) << 1
        if x * y > 0 or x == 0:
            s += 0 if abs(x) >= abs(y) else 4
        else:
            s += 4 if abs(x) > abs(y) else 0
        s += 1 if z > 0 else 0
        s += 2 if di > r12 else 0
        step = int(math.floor(b + 0.5))
        b -= step
        e_cos = U * abs(b)
        wgt = 1 - abs(b)
        dep(s * 11 + ((step + 1) % 10 if b > 0 else (step - 1 + 10) % 10), abs(b), e_cos)
        side = []                                            # (sector, weight, e): the deposits both channels receive at their own step
        e_c = 0.0
        if color:
            step_c = int(math.floor(bc[i] + 0.5))
            off = bc[i] - step_c
            e_c = 30 * d_cd[i] + U * abs(off)
            wgt_c = 1 - abs(off)
            up, down = 352 + s * 31 + (step_c + 1) % 30, 352 + s * 31 + (step_c - 1 + 30) % 30
            dep(up if off > 0 else down, abs(off), e_c)
            if abs(off) <= e_c and e_c > 0:
                E[down if off > 0 else up] += e_c + FIX
        # radial
        if di > r12:
            rd = (di - r34) / r12
            e_r = (2 * U * di + U * r34) / r12 + 3 * U * abs(rd)
            wgt_r = 1 - abs(rd)
            if rd <= 0 or rd <= e_r:
                side.append((s - 2, max(-rd, 0.0), e_r))
        else:
            rd = (di - r14) / r12
            e_r = (2 * U * di) / r12 + 3 * U * abs(rd)
            wgt_r = 1 - abs(rd)
            if rd >= 0 or -rd <= e_r:
                side.append((s + 2, max(rd, 0.0), e_r))
        # elevation
        a = min(1.0, abs(z / di))
        inc = _acos(z / di)
        acos_a, da = _acos(a), 5 * U * a
        cond = max(_acos(a - da) - acos_a, acos_a - _acos(a + da))
        e_acos = 2e-8 + 5.5 * U * acos_a + ((PI_ERR + U * inc) if z < 0 else 0.0)
        if inc > PI / 2 or (abs(inc - PI / 2) < 1e-30 and z <= 0):
            C = 3 * PI / 4
            el = (inc - C) / (PI / 2)
            e_e = (cond + e_acos + U * C + U * abs(inc - C)) * (2 / PI) + 3 * U * abs(el)
            if el <= 0 or el <= e_e:
                side.append((s + 1, max(-el, 0.0), e_e))
        else:
            C = PI / 4
            el = (inc - C) / (PI / 2)
            e_e = (cond + e_acos + U * C + U * abs(inc - C)) * (2 / PI) + 3 * U * abs(el)
            if el >= 0 or -el <= e_e:
                side.append((s - 1, max(el, 0.0), e_e))
        wgt_e = 1 - abs(el)
        # azimuth
        wgt_a, e_a = 0.0, 0.0
        if x != 0 or y != 0:
            az = math.atan2(y, x)
            ax_, ay_ = abs(x), abs(y)
            q = min(ax_, ay_) / max(ax_, ay_)
            r0 = math.atan(q)
            e_at = 2e-8 + 5.4 * U * q + U * r0
            if ay_ > ax_:
                r0 = PI / 2 - r0; e_at += PI2_ERR + U * r0
            if x < 0:
                r0 = PI - r0; e_at += PI_ERR + U * r0
            sel = s >> 2
            cen = -7 * PI / 8 + sel * PI / 4
            e_cen = U * (7 * PI / 8) + 2 * U * (PI / 4) * sel + U * abs(cen)
            ad = (az - cen) / (PI / 4)
            e_a = (e_at + e_cen + U * abs(az - cen)) * (4 / PI) + 3 * U * abs(ad)
            ad = max(-0.5, min(0.5, ad))
            wgt_a = 1 - abs(ad)
            fwd, back = (s + 4) % 32, (s - 4 + 32) % 32
            side.append((fwd if ad > 0 else back, abs(ad), e_a))
            if abs(ad) <= e_a:
                side.append((back if ad > 0 else fwd, 0.0, e_a))
        winc, e_inc = wgt_r + wgt_e + wgt_a, e_r + e_e + e_a + 13 * U
        for sec, w, e in side:
            dep(sec * 11 + step, w, e)
            if color:
                dep(352 + sec * 31 + step_c, w, e)
        dep(s * 11 + step, wgt + winc, e_cos + e_inc)
        if color:
            dep(352 + s * 31 + step_c, wgt_c + winc, e_c + e_inc)
    return (h, E, n_und), count


def shot352(points, normals, keypoint, frame, radius):
    """descriptor (352 float32, NaN when the keypoint is skipped), the number of radius neighbours of one keypoint, and the bound
    [352] on |device row - descriptor| of the module docstring (NaN with the descriptor)"""
    got, count = _describe(points, normals, keypoint, frame, radius)
    if got is None:
        return np.full(352, np.nan, f32), count, np.full(352, np.nan)
    row, bound = _finish(got[0], got[1])
    return row, count, bound


def cshot1344(points, normals, rgba, keypoint, kp_rgba, frame, radius, lab=lab_ref):
    """Row of one keypoint: desc [1344] float32 and bound [1344] (NaN when skipped), count, decided (False when a neighbour's colour
    step may fall either way on the device: a colour or the keypoint's colour undecided in `lab`, or bc + 0.5 within the Lab bound of
    an integer), and the shape half on its own: shape / shape_bound [352] = what shot352 returns on the same input (the first 352
    histogram values are those of SHOT-352; CSHOT only normalises them jointly with the colour half)."""
    got, count = _describe(points, normals, keypoint, frame, radius, rgba, kp_rgba, lab)
    if got is None:
        return Row(np.full(1344, np.nan, f32), count, np.full(1344, np.nan), True, np.full(352, np.nan, f32), np.full(352, np.nan), 0)
    h, E, n_und = got
    row, bound = _finish(h, E)
    shape, shape_bound = _finish(h[:352], E[:352])
    return Row(row, count, bound, n_und == 0, shape, shape_bound, n_und)


def describe(objs, kps, frames, radius):
    """rows for a ragged batch: objs = [(points, normals)], kps = [keypoints of object o], frames = [(len(kps[o]), 9)]"""
    rows, counts = [], []
    for (p, n), kp, fr in zip(objs, kps, frames):
        for k, f in zip(kp, fr):
            dsc, cnt, _ = shot352(p, n, k, f, radius)
            rows.append(dsc); counts.append(cnt)
    return np.asarray(rows, f32).reshape(-1, 352), np.asarray(counts, np.uint32)

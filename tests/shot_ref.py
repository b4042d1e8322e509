"""SHOT-352 restated from SURVEY.md Appendix A.2 in numpy, accumulating the histogram in float64.

Written from the appendix alone and sharing no code with oracle/: a second reading of the same specification, so that a
misreading the oracle and the kernels might share (a sector bit, a shell test, a modulo) shows up as a disagreement. The inputs
of every HARD decision (local coordinates, the cosine, the squared distance) are float32 values formed as the appendix states,
because their exact zeros and ties are what the boundary tests plant; everything continuous runs in float64."""
import numpy as np

f32 = np.float32
PI = np.pi


def _dot3(ax, ay, az, b):
    """float32 dot product, summed left to right"""
    return ((ax * f32(b[0])).astype(f32) + (ay * f32(b[1])).astype(f32)).astype(f32) + (az * f32(b[2])).astype(f32)


def shot352(points, normals, keypoint, frame, radius):
    """descriptor (352 float32, NaN when the keypoint is skipped) and the number of radius neighbours of one keypoint"""
    nan = np.full(352, np.nan, f32)
    p = np.asarray(points, f32).reshape(-1, 3)
    nrm = np.asarray(normals, f32).reshape(-1, 3)
    c = np.asarray(keypoint, f32)
    fr = np.asarray(frame, f32).reshape(3, 3)
    if not (np.isfinite(fr).all() and np.isfinite(c).all()):
        return nan, 0
    fin = np.isfinite(p).all(1)
    p, nrm = p[fin], nrm[fin]
    dx, dy, dz = (p[:, 0] - c[0]).astype(f32), (p[:, 1] - c[1]).astype(f32), (p[:, 2] - c[2]).astype(f32)
    d2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32) + (dz * dz).astype(f32)
    r = float(f32(radius))
    inside = d2 < f32(r * r)
    count = int(inside.sum())
    if count < 5:
        return nan, count
    dx, dy, dz, d2, nrm = dx[inside], dy[inside], dz[inside], d2[inside], nrm[inside]
    r34, r14, r12 = 3 * r / 4, r / 4, r / 2

    cos = np.clip(_dot3(nrm[:, 0], nrm[:, 1], nrm[:, 2], fr[2]), f32(-1), f32(1))
    d = np.sqrt(d2.astype(np.float64))
    use = np.isfinite(nrm).all(1) & ~(d < 1e-15)
    xl, yl, zl = _dot3(dx, dy, dz, fr[0]), _dot3(dx, dy, dz, fr[1]), _dot3(dx, dy, dz, fr[2])
    xl = np.where(np.abs(xl) < 1e-30, f32(0), xl); yl = np.where(np.abs(yl) < 1e-30, f32(0), yl); zl = np.where(np.abs(zl) < 1e-30, f32(0), zl)

    h = np.zeros(32 * 11, np.float64)
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
        step = int(np.floor(b + 0.5))
        vol = s * 11
        b -= step
        wgt = 1 - abs(b)
        if b > 0:
            h[vol + (step + 1) % 10] += b
        else:
            h[vol + (step - 1 + 10) % 10] += -b
        if di > r12:
            rd = (di - r34) / r12
            if di > r34:
                wgt += 1 - rd
            else:
                wgt += 1 + rd; h[(s - 2) * 11 + step] -= rd
        else:
            rd = (di - r14) / r12
            if di < r14:
                wgt += 1 + rd
            else:
                wgt += 1 - rd; h[(s + 2) * 11 + step] += rd
        inc = np.arccos(min(1.0, max(-1.0, z / di)))
        if inc > PI / 2 or (abs(inc - PI / 2) < 1e-30 and z <= 0):
            e = (inc - 3 * PI / 4) / (PI / 2)
            if inc > 3 * PI / 4:
                wgt += 1 - e
            else:
                wgt += 1 + e; h[(s + 1) * 11 + step] -= e
        else:
            e = (inc - PI / 4) / (PI / 2)
            if inc < PI / 4:
                wgt += 1 + e
            else:
                wgt += 1 - e; h[(s - 1) * 11 + step] += e
        if x != 0 or y != 0:
            az = np.arctan2(y, x)
            sel = s >> 2
            ad = (az - (-7 * PI / 8 + sel * PI / 4)) / (PI / 4)
            ad = max(-0.5, min(0.5, ad))
            if ad > 0:
                wgt += 1 - ad; h[((s + 4) % 32) * 11 + step] += ad
            else:
                wgt += 1 + ad; h[((s - 4 + 32) % 32) * 11 + step] -= ad
        h[vol + step] += wgt
    return (h / np.sqrt((h * h).sum())).astype(f32), count


def describe(objs, kps, frames, radius):
    """rows for a ragged batch: objs = [(points, normals)], kps = [keypoints of object o], frames = [(len(kps[o]), 9)]"""
    rows, counts = [], []
    for (p, n), kp, fr in zip(objs, kps, frames):
        for k, f in zip(kp, fr):
            dsc, cnt = shot352(p, n, k, f, radius)
            rows.append(dsc); counts.append(cnt)
    return np.asarray(rows, f32).reshape(-1, 352), np.asarray(counts, np.uint32)

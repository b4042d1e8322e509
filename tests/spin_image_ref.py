"""A numpy restatement of the SpinImage descriptor as include/ismhip.h defines it (ismhip_keypoint_normals, ismhip_spin_image; DESIGN.md
section 4.15): the float steps in float32, unfused and in the written order, everything after them in float64. The bins are summed as
float64 here, not as 2^-28 integers: the device's fixed point is then held to 1e-7 absolute by the derivation in tests/test_gpu_spin_image.py.

It also counts UNDECIDED neighbours, those whose fate a last-bit difference could change: |beta| or alpha within 1e-9 * lim of lim, d2
within one ulp of the ball test, norm within a factor of two of the skip test. The scenes are built so that there are none."""
import numpy as np

F = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)


def dim_of(w):
    return (w + 1) * (2 * w + 1)


def r2_of(radius):
    return F(np.float64(F(radius)) * np.float64(F(radius)))


def bin_of(radius, w):
    """(bin, lim) = ((double)radius / w / sqrt(2.0), bin * w)"""
    b = np.float64(F(radius)) / w / np.sqrt(2.0)
    return b, b * w


def keypoint_normals(xyz, normals, kp):
    """per keypoint the normal of the lowest-index finite point with equal coordinates and that index; (0, 0, 0) and -1 without one"""
    xyz = np.asarray(xyz, F); normals = np.asarray(normals, F); kp = np.asarray(kp, F).reshape(-1, 3)
    fin = np.isfinite(xyz).all(1)
    axes = np.zeros((len(kp), 3), F)
    idx = np.full(len(kp), -1, np.int32)
    for k, q in enumerate(kp):
        hit = np.nonzero(fin & (xyz[:, 0] == q[0]) & (xyz[:, 1] == q[1]) & (xyz[:, 2] == q[2]))[0] if len(xyz) else []
        if len(hit):
            idx[k] = hit[0]; axes[k] = normals[hit[0]]
    return axes, idx


def spin_row(xyz, c, n, radius, w=8):
    """one keypoint -> dict(row float32 [(w+1)(2w+1)], cnt, deposited, undecided)"""
    D = dim_of(w)
    xyz = np.asarray(xyz, F).reshape(-1, 3); c = np.asarray(c, F); n = np.asarray(n, F)
    nan_row = np.full(D, np.nan, F)
    if not (np.isfinite(c).all() and np.isfinite(n).all()):
        return dict(row=nan_row, cnt=0, deposited=0, undecided=0)
    p = xyz[np.isfinite(xyz).all(1)]
    d = p - c                                                           # float32
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]     # float32, unfused
    r2 = r2_of(radius)
    undecided = int(((d2 == r2) | (d2 == np.nextafter(r2, F(0))) | (d2 == np.nextafter(r2, F(np.inf)))).sum())
    nb = d2 < r2
    cnt = int(nb.sum())
    d, d2 = d[nb], d2[nb]
    norm = np.sqrt(d2)                                                  # float32, correctly rounded
    norm64 = norm.astype(np.float64)
    undecided += int(((norm64 >= 5.0 * DBL_EPSILON) & (norm64 < 20.0 * DBL_EPSILON)).sum())
    live = ~(norm64 < 10.0 * DBL_EPSILON)
    d, norm64 = d[live], norm64[live]
    dot = (d[:, 0] * n[0] + d[:, 1] * n[1]) + d[:, 2] * n[2]             # float32, unfused
    cos = dot.astype(np.float64) / norm64
    if (~(np.abs(cos) <= 1.0 + 10.0 * FLT_EPSILON)).any():             # beyond rounding, or no number (an overflowed dot product)
        return dict(row=nan_row, cnt=cnt, deposited=0, undecided=undecided)
    cos = np.clip(cos, -1.0, 1.0)
    beta = norm64 * cos
    alpha = norm64 * np.sqrt(1.0 - cos * cos)
    b, lim = bin_of(radius, w)
    undecided += int(((np.abs(np.abs(beta) - lim) <= 1e-9 * lim) | (np.abs(alpha - lim) <= 1e-9 * lim)).sum())
    inside = ~((np.abs(beta) >= lim) | (alpha >= lim))
    alpha, beta = alpha[inside], beta[inside]
    ta, tb = alpha / b, beta / b
    fa, fb = np.floor(ta), np.floor(tb)
    ia, ib = fa.astype(np.int64), fb.astype(np.int64) + w
    wa, wb = ta - fa, tb - fb
    H = np.zeros((w + 2, 2 * w + 2))                                    # one spare row and column: entries outside the matrix are dropped
    np.add.at(H, (ia, ib), (1.0 - wa) * (1.0 - wb))
    np.add.at(H, (ia + 1, ib), wa * (1.0 - wb))
    np.add.at(H, (ia, ib + 1), (1.0 - wa) * wb)
    np.add.at(H, (ia + 1, ib + 1), wa * wb)
    H = H[:w + 1, :2 * w + 1].reshape(-1)
    if cnt > 1:
        with np.errstate(invalid="ignore", divide="ignore"):
            H = H / H.sum()                                             # no deposit at all: 0 / 0, the NaN row
    return dict(row=H.astype(F), cnt=cnt, deposited=int(inside.sum()), undecided=undecided)


def spin_images(pt_off, xyz, kp_off, kp, axes, radius, w=8):
    """a ragged batch -> dict(rows [nkp, D] float32, cnt [nkp] int32, deposited, undecided (totals))"""
    kp = np.asarray(kp, F).reshape(-1, 3)
    rows = np.zeros((len(kp), dim_of(w)), F)
    cnt = np.zeros(len(kp), np.int32)
    dep = np.zeros(len(kp), np.int64)
    und = 0
    for o in range(len(pt_off) - 1):
        cloud = np.asarray(xyz, F)[int(pt_off[o]):int(pt_off[o + 1])]
        for k in range(int(kp_off[o]), int(kp_off[o + 1])):
            a = spin_row(cloud, kp[k], axes[k], radius, w)
            rows[k] = a["row"]; cnt[k] = a["cnt"]; dep[k] = a["deposited"]; und += a["undecided"]
    return dict(rows=rows, cnt=cnt, deposited=dep, undecided=und)


def batch_normals(pt_off, xyz, normals, kp_off, kp):
    kp = np.asarray(kp, F).reshape(-1, 3)
    axes = np.zeros((len(kp), 3), F); idx = np.full(len(kp), -1, np.int32)
    for o in range(len(pt_off) - 1):
        s, e, ks, ke = int(pt_off[o]), int(pt_off[o + 1]), int(kp_off[o]), int(kp_off[o + 1])
        axes[ks:ke], idx[ks:ke] = keypoint_normals(np.asarray(xyz, F)[s:e], np.asarray(normals, F)[s:e], kp[ks:ke])
    return axes, idx

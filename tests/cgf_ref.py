"""float64 numpy restatement of the CGF descriptor as this library defines it (include/ismhip.h): the raw
spherical histogram of third_party/cgf/cgf.cpp:98-161 and the perceptron of third_party/cgf/embedding.py:103-108 with a derived error
bound. No import from the package: the tests hold the device to this file.

The histogram. Everything the device does in float32 (the ball test, p - k, the three unfused dot products against the frame) is done
here in float32 by the same operations, so it has the same bits; everything after is float64 on both sides. A deposit is UNDECIDED when
moving x, y, z by twice the rounding error that their float32 dot products actually made (measured against the float64 product sums,
zero for an axis-aligned frame) moves it into another bin, and a keypoint is undecided when one of its deposits is, when the choice of
its nearest ball point hangs on a difference of d2 inside the float32 error of d2 and the two candidates fall into different bins, or
when the sign of z . n that flips its frame does."""
import numpy as np

F = np.float32
NR, NT, NP = 17, 11, 12
DIM = NR * NT * NP                                  # 2244
RAD2DEG = 57.29578                                  # pcl::rad2deg(double)
U = 2.0 ** -24


def radii(radius):
    """(R, rmin, LRF radius) of features_cgf.cpp:50-52 after std::to_string ("%f") and stod; the normal radius is 0.1 * R (cgf.cpp:93)"""
    r = float(F(radius))
    return float("%f" % r), float("%f" % (r * 0.05)), float("%f" % (r * 0.75))


def bins(x, y, z, R, rmin):
    """cgf.cpp:140-150 in float64 -> (bin_r, bin_theta, bin_phi); a NaN coordinate goes to bin 0 (named deviation: the reference's cast
    is undefined there). The casts truncate towards zero."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z)
        theta = np.arccos(z / r) * RAD2DEG
        phi = np.arctan2(y, x) * RAD2DEG
        tr = (NR - 1) * (np.log(r) - np.log(rmin)) / np.log(R / rmin) + 1.0
        tt = NT * theta / 180.0
        tp = NP * (phi + 180.0) / 360.0

        def cut(t, n):
            t = np.where(t > 0.0, t, 0.0)           # NaN and everything at or below zero: bin 0
            return np.minimum(np.trunc(np.minimum(t, float(n))), n - 1).astype(np.int64)
        return cut(tr, NR), cut(tt, NT), cut(tp, NP)


def index(br, bt, bp):
    return br + NR * bt + NR * NT * bp


def frame(lrf9, normal):
    """cgf.cpp:112-129 on a float32 SHOT frame (x, y, z axes, nine floats) and the keypoint's float32 PCA normal -> (ax, ay, az, kind,
    undecided): kind "identity" for a frame with a NaN in its x axis, "flipped" when (z0 n0 + z1 n1) + z2 n2 < 0 in float32, else "kept"
    (a NaN normal flips nothing)"""
    f = np.asarray(lrf9, F).reshape(3, 3)
    n = np.asarray(normal, F)
    if np.isnan(f[0]).any():
        return F([1, 0, 0]), F([0, 1, 0]), F([0, 0, 1]), "identity", False
    with np.errstate(all="ignore"):
        dot = F(F(F(f[2, 0] * n[0]) + F(f[2, 1] * n[1])) + F(f[2, 2] * n[2]))
        exact = float(np.dot(f[2].astype(np.float64), n.astype(np.float64)))
    undecided = bool(np.isfinite(exact) and abs(exact) <= 2.0 * abs(float(dot) - exact) and float(dot) != exact)
    if dot < 0:
        return -f[0], -f[1], -f[2], "flipped", undecided
    return f[0], f[1], f[2], "kept", undecided


def raw(xyz, kp, lrf, normals, radius):
    """The raw rows of the keypoints kp [m, 3] over the cloud xyz [n, 3] (one object), with the device's (or the oracle's) float32 frames
    lrf [m, 9] at the LRF radius and keypoint normals [m, 3]. radius: the configured Radius (rounded here as radii() says).
    -> dict(counts [m, 2244] int64, sum [m], rows [m, 2244] float32, undecided [m] bool, ball [m] points in the ball, skipped [m] the index
    of the point the skip rule left out (-1: empty ball), kind [m] the frame's kind, deposits_undecided, deposits)"""
    xyz = np.asarray(xyz, F); kp = np.asarray(kp, F)
    R, rmin, _ = radii(radius)
    r2 = F(R * R)
    m = len(kp)
    counts = np.zeros((m, DIM), np.int64)
    out = dict(counts=counts, sum=np.zeros(m, np.int64), undecided=np.zeros(m, bool), ball=np.zeros(m, np.int64), skipped=np.full(m, -1, np.int64),
               kind=[], deposits=0, deposits_undecided=0)
    fin = np.isfinite(xyz).all(1)
    for k in range(m):
        ax, ay, az, kind, und = frame(lrf[k], normals[k])
        out["kind"].append(kind)
        if not np.isfinite(kp[k]).all():
            out["kind"][-1] = "nan"
            continue
        with np.errstate(all="ignore"):
            v = xyz - kp[k]                                       # float32
            d2 = F(F(v[:, 0] * v[:, 0]) + F(v[:, 1] * v[:, 1])) + F(v[:, 2] * v[:, 2])
        ball = np.flatnonzero(fin & (d2 < r2))
        out["ball"][k] = len(ball)
        if len(ball) == 0:
            out["undecided"][k] = und
            continue
        order = ball[np.lexsort((ball, d2[ball]))]                # by d2, ties to the lowest index
        skip = order[0]
        out["skipped"][k] = skip
        vb = v[ball]
        x = F(F(vb[:, 0] * ax[0]) + F(vb[:, 1] * ax[1])) + F(vb[:, 2] * ax[2])
        y = F(F(vb[:, 0] * ay[0]) + F(vb[:, 1] * ay[1])) + F(vb[:, 2] * ay[2])
        z = F(F(vb[:, 0] * az[0]) + F(vb[:, 1] * az[1])) + F(vb[:, 2] * az[2])
        idx = index(*bins(x, y, z, R, rmin))
        # the rounding error the three dot products made
        v64 = vb.astype(np.float64)
        err = [2.0 * np.abs(c.astype(np.float64) - v64 @ a.astype(np.float64)) for c, a in ((x, ax), (y, ay), (z, az))]
        moved = np.zeros(len(ball), bool)
        if any(e.any() for e in err):
            for sx in (-1.0, 1.0):
                for sy in (-1.0, 1.0):
                    for sz in (-1.0, 1.0):
                        moved |= index(*bins(x + sx * err[0], y + sy * err[1], z + sz * err[2], R, rmin)) != idx
        # a near-tie for "nearest": another ball point whose d2 differs by less than the float32 error of d2 and which lands elsewhere
        near = (d2[ball] != d2[skip]) & (np.abs(d2[ball].astype(np.float64) - float(d2[skip])) <= 8.0 * U * float(d2[skip]))
        pos = {p: i for i, p in enumerate(ball)}
        tie = bool((near & (idx != idx[pos[skip]])).any())
        keep = (ball != skip) & (d2[ball].astype(np.float64) > 1e-15)
        np.add.at(counts[k], idx[keep], 1)
        out["sum"][k] = int(keep.sum())
        out["deposits"] += int(keep.sum()); out["deposits_undecided"] += int((moved & keep).sum())
        out["undecided"][k] = und or tie or bool((moved & keep).any())
    s = out["sum"].astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        rows = np.where(s > 0, counts / np.where(s > 0, s, 1.0), 0.0).astype(F)
    rows[[i for i, kd in enumerate(out["kind"]) if kd == "nan"]] = np.nan
    out["rows"] = rows
    return out


def pca_normal(xyz, kp, radius):
    """the normal of ismhip_keypoint_normals_pca in float64: the eigenvector of the smallest eigenvalue of the covariance of the ball's
    points (d2 < (float)(radius^2) in float32, at least 3), flipped towards (0,0,0) -> (normals [m, 3], count [m], gap [m] = the
    relative gap between the two smallest eigenvalues: the direction is only as well determined as the gap is wide)"""
    xyz = np.asarray(xyz, F); kp = np.asarray(kp, F)
    r2 = F(float(F(radius)) * float(F(radius)))
    fin = np.isfinite(xyz).all(1)
    nrm = np.full((len(kp), 3), np.nan); cnt = np.zeros(len(kp), np.int64); gap = np.zeros(len(kp))
    for k in range(len(kp)):
        v = xyz - kp[k]
        d2 = F(F(v[:, 0] * v[:, 0]) + F(v[:, 1] * v[:, 1])) + F(v[:, 2] * v[:, 2])
        ball = fin & (d2 < r2)
        cnt[k] = ball.sum()
        if cnt[k] < 3:
            continue
        d = xyz[ball].astype(np.float64) - kp[k].astype(np.float64)
        d -= d.mean(0)
        w, V = np.linalg.eigh(d.T @ d / cnt[k])
        n = V[:, 0]
        if np.dot(-kp[k].astype(np.float64), n) < 0:
            n = -n
        nrm[k] = n
        gap[k] = (w[1] - w[0]) / max(w[2], 1e-300)
    return nrm, cnt, gap


# ---------------------------------------------------------------------------------------------------------------- the perceptron
def gamma(k):
    return k * U / (1.0 - k * U)


def mlp(x, layers):
    """y = the float64 forward pass of layers [(W [in, out], b [out], relu), ...] on x [n, in], and a bound on |y_float32 - y| that holds
    for ANY order of the float32 sums: per layer e_out = |W|^T e_in + gamma_{n+1} (|W|^T (|x| + e_in) + |b|), n = in (n products and
    the bias, n + 1 roundings at most on every term), gamma_k = k u / (1 - k u), u = 2^-24; ReLU is 1-Lipschitz; the input carries no
    error. Derived, not measured."""
    x = np.asarray(x, np.float64)
    e = np.zeros_like(x)
    for W, b, relu in layers:
        W = np.asarray(W, np.float64); b = np.asarray(b, np.float64)
        aW = np.abs(W)
        e = e @ aW + gamma(W.shape[0] + 1) * ((np.abs(x) + e) @ aW + np.abs(b))
        x = x @ W + b
        if relu:
            x = np.maximum(x, 0.0)
    return x, e


def mlp_bound_unit_mass(layers):
    """the same bound for ANY non-negative input row of sum <= 1 (what a raw CGF row is), without knowing the row: |x|^T |W| <= the
    column maxima of |W| in the first layer, and from there the bound on the values, h_out <= h^T |W| + |b|, is carried next to the error
    -> e [out]"""
    h = e = None
    for W, b, _relu in layers:
        aW = np.abs(np.asarray(W, np.float64)); ab = np.abs(np.asarray(b, np.float64))
        reach = aW.max(0) if h is None else h @ aW
        carried = 0.0 if e is None else e @ aW
        e = carried + gamma(aW.shape[0] + 1) * (reach + carried + ab)
        h = reach + ab
    return e

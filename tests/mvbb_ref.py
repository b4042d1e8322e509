"""float64 restatement of ismhip_region_mvbb (include/ismhip.h): brute-force pairs, a monotone-chain hull over
ALL points (no pre-filter), plain Python / numpy doubles in the header's order. Beside every decision stands its margin; a decision
whose margin is below the bound derived here is UNDECIDED, and a comparison against another implementation of the same definition
stops there.

The bound. The kernel and this file run the same operations in the same order, so they can differ only where sqrt or a division is
not correctly rounded on one side: a relative 2^-52 per such operation. Through the steps (normalise, project, bound, lift: a few
dozen operations deep, ten rounds) that stays below 2^-44 of the cloud's scale unless a short hull edge amplifies it: an edge
of length L turns a coordinate error of 2^-52 M into a direction error of 2^-52 M / L. DECISION = 2^-40 leaves a factor of 16 over
2^-44, and is the margin the kernel's pre-filter uses. Decisions are relative to their natural scale: d2 of the diameter for pair
gaps, M^2 (M the larger projected extent) for orientation tests and area gaps. A volume e0 e1 e2 carries the absolute rounding of
its extents, about 10 * 2^-53 D each (D the diameter), so a relative 3 * 10 * 2^-53 D / e_min < 2^-46 D / e_min: a volume comparison
is undecided within that of its threshold. Step D's threshold TAKE = 1 - 2^-36 stands well off a converged box's own volume, so
finding such a box again is a decided "not taken" unless the box is thinner than about D / 500. Two hull edges whose areas tie are
harmless when they are sides of one rectangle (parallel or perpendicular) and the round is a decided "not taken": the two edge
indices of that round go to `soft` (not compared) and the comparison goes on; any other tie is undecided. Step A is
exempt: its d2 comes from float differences that are exact in double and three products summed in one order: the same bits on both
sides, ties included.
Values: `vol_tol` is 16 times the volume's rounding above; box()'s `tol` is scale * (2^-22 + 2^-40 * cond): two float32 roundings of the output cast plus the double chain, cond = the
largest M / L over the chosen edges."""
import math

import numpy as np

ROUNDS, TRACE = 10, 48
DECISION = 2.0 ** -40
TAKE = 1.0 - 2.0 ** -36             # step D keeps a round's box if its volume is below TAKE x the best one's
VOLUME_NOISE = 2.0 ** -46           # x D / (smallest extent): relative rounding of a volume (see the module text)


def _dot(p, a):
    return (p[..., 0] * a[0] + p[..., 1] * a[1]) + p[..., 2] * a[2]


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(v):
    length = math.sqrt(_dot3(v, v))
    if length == 0.0:
        return [float(v[0]), float(v[1]), float(v[2])]
    return [v[0] / length, v[1] / length, v[2] / length]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]]


def base(u):
    """gdiam_generate_orthonormal_base on normalise(u), its case list as written -> (u, bx, by)"""
    u = _normalize(u)
    n = _normalize
    if u[0] == 0.0:
        if u[1] == 0.0:
            return u, n([1.0, 0.0, 0.0]), n([0.0, 1.0, 0.0])
        if u[2] == 0.0:
            return u, n([1.0, 0.0, 0.0]), n([0.0, 0.0, 1.0])
        return u, n([0.0, -u[2], u[1]]), n([1.0, 0.0, 0.0])
    if u[1] == 0.0 and u[2] == 0.0:
        return u, n([0.0, 1.0, 0.0]), n([0.0, 0.0, 1.0])
    if u[1] == 0.0:
        return u, n([-u[2], 0.0, u[0]]), n([0.0, 1.0, 0.0])
    if u[2] == 0.0:
        return u, n([-u[1], u[0], 0.0]), n([0.0, 0.0, 1.0])
    o1 = n([-u[1], u[0], 0.0])
    return u, o1, n(_cross(u, o1))


def bound(p, axes):
    lo, hi = [], []
    for a in axes:
        s = _dot(p, a)
        lo.append(float(s.min()))
        hi.append(float(s.max()))
    vol = ((hi[0] - lo[0]) * (hi[1] - lo[1])) * (hi[2] - lo[2])
    return dict(axes=[list(map(float, a)) for a in axes], lo=lo, hi=hi, vol=vol)


def farthest_pair(q, rows=256):
    """(i, j, d2, relative gap to the runner-up) over the rows of q: largest d2, ties to the lowest (i, j); `rows` rows of the pair
    matrix at a time"""
    n = q.shape[0]
    best, bi, bj, second = -1.0, -1, -1, -1.0
    for a in range(0, n - 1, rows):
        b = min(a + rows, n - 1)
        d = q[a:b, None, :] - q[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2[np.arange(b - a)[:, None] + a >= np.arange(n)[None, :]] = -1.0      # pairs i < j only
        flat = d2.ravel()
        k = int(np.argmax(flat))                              # row-major: the first of equal maxima is the lowest (i, j)
        top = float(flat[k])
        flat[k] = -1.0
        runner = float(flat.max()) if flat.size > 1 else -1.0
        if top > best:                                        # an earlier block holds the lower i
            second = max(best, runner)
            best, bi, bj = top, a + k // n, k % n
        else:
            second = max(second, top)
    gap = (best - second) / best if best > 0 and second >= 0 else (1.0 if second < 0 else 0.0)
    return int(bi), int(bj), best, gap


def hull(x, y, idx, m2):
    """strict vertices, counter-clockwise from the lowest (x, y) -> (positions into x / y, margin). The margin is taken from the result,
    not from the chain's tests (two interior points that nearly coincide make a tiny turn that decides nothing): the smallest turn at a
    vertex and the smallest distance measure turn(a, b, p) of a point p that is no vertex from an edge (a, b), over m2. Above the
    bound, every implementation whose tests err by less finds these vertices."""
    order = np.lexsort((idx, y, x))
    pts = []
    for o in order:
        if pts and x[o] == x[pts[-1]] and y[o] == y[pts[-1]]:
            continue
        pts.append(int(o))

    def turn(o, a, b):
        return (x[a] - x[o]) * (y[b] - y[o]) - (y[a] - y[o]) * (x[b] - x[o])

    if len(pts) == 1:
        return pts, math.inf
    h = []
    for p in pts:
        while len(h) >= 2 and turn(h[-2], h[-1], p) <= 0.0:
            h.pop()
        h.append(p)
    t = len(h) + 1
    for p in reversed(pts[:-1]):
        while len(h) >= t and turn(h[-2], h[-1], p) <= 0.0:
            h.pop()
        h.append(p)
    h.pop()
    if len(h) < 3 or not m2 > 0:
        return h, 0.0
    ha = np.array(h)
    hb = np.roll(ha, -1)
    hp = np.roll(ha, 1)
    margin = float(((x[ha] - x[hp]) * (y[hb] - y[hp]) - (y[ha] - y[hp]) * (x[hb] - x[hp])).min())
    rest = np.setdiff1d(np.array(pts), ha)
    if rest.size:
        c = (x[hb] - x[ha])[None, :] * (y[rest][:, None] - y[ha][None, :]) - (y[hb] - y[ha])[None, :] * (x[rest][:, None] - x[ha][None, :])
        margin = min(margin, float(c.min()))
    return h, margin / m2


def box(points):
    """points: float array [n, 3] (finite) in index order -> dict(n, center, size, axes [3][3], volume, trace [48], undecided_at, soft, tol).
    soft: trace indices below undecided_at that are not to be compared (always [7], the kernel's own diagnostic); undecided_at: the first trace index whose decision is undecided (TRACE: none); tol: see the module text."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = p.shape[0]
    trace = [0] * TRACE
    for k in (0, 1, 2, 3):
        trace[k] = -1
    for r in range(ROUNDS):
        trace[8 + 4 * r + 2] = trace[8 + 4 * r + 3] = -1
    nan = float("nan")
    ident = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if n == 0:
        return dict(n=0, center=[nan] * 3, size=[0.0] * 3, axes=[[nan] * 3] * 3, volume=0.0, trace=trace, undecided_at=TRACE, soft=[], tol=0.0, vol_tol=0.0)
    scale = float(np.abs(p).max()) + 1e-300
    degenerate = n < 2
    if not degenerate:
        i, j, d2a, _ = farthest_pair(p)
        diff = p[i] - p[j]
        degenerate = _dot3(diff, diff) == 0.0
    if degenerate:
        b = bound(p, ident)
        trace[6] = 1
        return dict(n=n, center=[(b["lo"][k] + b["hi"][k]) * 0.5 for k in range(3)], size=[0.0] * 3, axes=ident, volume=0.0, trace=trace,
                    undecided_at=TRACE, soft=[], tol=scale * 2.0 ** -22, vol_tol=0.0)
    undecided = [TRACE]

    def flag(at, margin):
        if margin < DECISION:
            undecided[0] = min(undecided[0], at)

    trace[0], trace[1] = i, j
    diam = math.sqrt(d2a)
    d1 = _normalize(diff)
    # B
    t = _dot(p, d1)
    pp = np.stack([p[:, 0] - t * d1[0], p[:, 1] - t * d1[1], p[:, 2] - t * d1[2]], axis=1)
    i2, j2, _, gap = farthest_pair(pp)
    flag(2, gap * (_dot3(pp[i2] - pp[j2], pp[i2] - pp[j2]) / d2a))    # the gap in units of the diameter's d2
    trace[2], trace[3] = i2, j2
    v = pp[i2] - pp[j2]
    prd = _dot3(v, d1)
    q = [v[0] - prd * d1[0], v[1] - prd * d1[1], v[2] - prd * d1[2]]
    length = math.sqrt(_dot3(q, q))
    flag(2, abs(length - 1e-6) / 1e-6)
    if length < 1e-6:
        trace[5] = 1
        _, d2v, d3v = base(d1)
    else:
        d2v = [q[0] / length, q[1] / length, q[2] / length]
        d3v = _normalize(_cross(d1, d2v))
    # C
    best = bound(p, [d1, d2v, d3v])
    aabb = bound(p, ident)
    emin = min(min(b_["hi"][k] - b_["lo"][k] for k in range(3)) for b_ in (aabb, best))
    if not (emin > 0 and abs(aabb["vol"] - best["vol"]) >= VOLUME_NOISE * (diam / emin) * max(aabb["vol"], best["vol"])):
        flag(4, 0.0)
    if aabb["vol"] < best["vol"]:
        best = aabb
        trace[4] = 1
    # D
    idx = np.arange(n)
    cond = 1.0
    soft = set()
    for r in range(ROUNDS):
        at = 8 + 4 * r
        u, bx, by = base(best["axes"][r % 3])
        x, y = _dot(p, bx), _dot(p, by)
        m = max(float(x.max() - x.min()), float(y.max() - y.min()))
        h, hm = hull(x, y, idx, m * m)
        flag(at, hm)
        ex, ey, e0, e1 = 1.0, 0.0, h[0], h[0]
        same_rectangle = None
        if len(h) > 1:
            hx, hy = x[h], y[h]
            areas = []
            for k in range(len(h)):
                a, b = h[k], h[(k + 1) % len(h)]
                dx, dy = x[b] - x[a], y[b] - y[a]
                ln = math.sqrt(dx * dx + dy * dy)
                dx, dy = dx / ln, dy / ln
                s = hx * dx + hy * dy
                tt = hy * dx - hx * dy
                areas.append((float((s.max() - s.min()) * (tt.max() - tt.min())), a, b, dx, dy, ln))
            areas.sort(key=lambda z: (z[0], z[1]))
            _, e0, e1, ex, ey, ln = areas[0]
            cond = max(cond, m / ln)
            close = [z for z in areas[1:] if not m > 0 or (z[0] - areas[0][0]) / (m * m) < DECISION]
            if close:                                         # a tie: harmless only between edges of one and the same rectangle
                same_rectangle = all(min(abs(z[3] * ex + z[4] * ey), abs(z[3] * ey - z[4] * ex)) < 2.0 ** -30 for z in close)
        o1 = _normalize([(-ey) * bx[k] + ex * by[k] for k in range(3)])
        o2 = _normalize([ex * bx[k] + ey * by[k] for k in range(3)])
        cand = bound(p, [u, o1, o2])
        thr = best["vol"] * TAKE
        emin = min(min(b_["hi"][k] - b_["lo"][k] for k in range(3)) for b_ in (cand, best))
        sure = emin > 0 and abs(cand["vol"] - thr) >= VOLUME_NOISE * (diam / emin) * best["vol"]
        if not sure:
            flag(at, 0.0)
        take = cand["vol"] < thr
        if same_rectangle is not None:
            if same_rectangle and sure and not take:
                soft.update((at + 2, at + 3))                 # the box stays: which of its flush edges was found decides nothing
            else:
                flag(at, 0.0)
        if take:
            best = cand
        trace[at:at + 4] = [1 if take else 0, len(h), int(e0), int(e1)]
    # the output convention
    ext = [best["hi"][k] - best["lo"][k] for k in range(3)]
    order = sorted(range(3), key=lambda k: (-ext[k], k))
    ax = [list(best["axes"][k]) for k in order]
    lo = [best["lo"][k] for k in order]
    hi = [best["hi"][k] for k in order]
    for r in range(2):
        k = 0
        if abs(ax[r][1]) > abs(ax[r][k]):
            k = 1
        if abs(ax[r][2]) > abs(ax[r][k]):
            k = 2
        if ax[r][k] < 0.0:
            ax[r] = [-c for c in ax[r]]
            lo[r], hi[r] = -hi[r], -lo[r]
    a3 = _cross(ax[0], ax[1])
    if _dot3(a3, ax[2]) < 0.0:
        lo[2], hi[2] = -hi[2], -lo[2]
    ax[2] = a3
    mid = [(lo[k] + hi[k]) * 0.5 for k in range(3)]
    center = [(mid[0] * ax[0][k] + mid[1] * ax[1][k]) + mid[2] * ax[2][k] for k in range(3)]
    return dict(n=n, center=center, size=[hi[k] - lo[k] for k in range(3)], axes=ax, volume=best["vol"], trace=trace,
                vol_tol=best["vol"] * 16.0 * VOLUME_NOISE * diam / max(min(hi[k] - lo[k] for k in range(3)), 1e-300),
                undecided_at=undecided[0], soft=sorted(k for k in soft | {7} if k < undecided[0]), tol=scale * (2.0 ** -22 + 2.0 ** -40 * cond))


def select(points, center=None, radius=None):
    """the region rule of include/ismhip.h on one object's points -> indices of the selected (finite) points, ascending"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    ok = np.isfinite(p).all(1)
    if radius is not None and radius >= 0:
        c = np.asarray(center, dtype=np.float32)
        d = p - c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        with np.errstate(invalid="ignore"):
            ok &= d2 < np.float32(np.float64(np.float32(radius)) * np.float64(np.float32(radius)))
    return np.nonzero(ok)[0]


def region_box(points, center=None, radius=None):
    """box() of a region; trace indices are indices into `points` (the object), as the kernel reports them"""
    sel = select(points, center, radius)
    b = box(np.asarray(points, dtype=np.float32).reshape(-1, 3)[sel])
    b["trace"] = list(b["trace"])
    for k in [0, 1, 2, 3] + [8 + 4 * r + c for r in range(ROUNDS) for c in (2, 3)]:
        if b["trace"][k] >= 0:
            b["trace"][k] = int(sel[b["trace"][k]])
    return b

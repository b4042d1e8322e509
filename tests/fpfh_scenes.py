"""Seeded scenes for FPFH-33 (numpy only): the smallest inputs that reach each hard decision of csrc/fpfh.hip. fpfh_ref.py gives the
float64 intervals, test_fpfh_cpu.py proves on the host that every scene reaches its decision, test_gpu_fpfh.py runs the kernels on
the same bytes. scene(name) -> dict(objs=[(points, normals)], kps=[keypoints], radius, cell, ...); every builder is deterministic.

The small constructed objects share one frame ("Darboux objects"): a centre c with normal n_s = (0, 0, 1) and neighbours at
c + k (5, 0, 12) / 128, k = 1, 2, 3, with normals b. In ANY float32 operation order |d| = 13 k / 128 (5-12-13: the squares and
their sum are exact), cos1 = 12/13 -> f3 = 0.923 (t3 = 10.58), v = d x n_s = (0, -d_x, 0) / d_x = (0, -1, 0) and w = (1, 0, 0), because
every other product has a factor 0. Hence f2 = -b_y, x = b_z and y = b_x EXACTLY, whatever the arithmetic: the target normal sets the
features bit by bit. |cos2| = |5 b_x + 12 b_z| / 13 stays well below 12/13, so the centre always plays the source (from both ends
of the pair), and the neighbours' normals differ from each other so that no neighbour-neighbour pair is a role tie."""
import numpy as np

from frontend_scenes import _unit, ellipsoid, soa

f32 = np.float32
STEP = np.array([5.0, 0.0, 12.0]) / 128.0
N_S = f32([0, 0, 1])
DARBOUX_RADIUS, DARBOUX_CELL = 0.5, 0.25
QUEUE_COUNTS = [2, 3, 64, 65, 66, 128, 129, 130, 193]          # in-ball counts n_p: 1, 2, 63, 64, 65, 127, 128, 129, 192 queued pairs
SUM_COUNTS = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65]              # usable neighbours of one keypoint inside one cell row


def darboux_object(x0, normals, kp_on_centre=False, nb_y=0.0):
    """centre (x0, 0, 0) + three neighbours (module docstring) -> ((points, normals), keypoints). x0: a small integer"""
    p = [[x0, 0.0, 0.0]] + [[x0 + k * STEP[0], nb_y, k * STEP[2]] for k in (1, 2, 3)]
    n = [N_S] + [f32(b) for b in normals]
    kp = [[x0, 0.0, 0.0]] if kp_on_centre else [[x0, 2.0 ** -7, 0.0]]
    return (f32(p), f32(n)), f32(kp)


def _edge(j):
    return 2.0 * j / 11.0 - 1.0


def _xz(s, t1):
    """(b_x, b_z) of length s whose angle atan2(b_x, b_z) has the bin coordinate t1"""
    phi = 2 * np.pi * t1 / 11 - np.pi
    return s * np.sin(phi), s * np.cos(phi)


# ---------------------------------------------------------------------------------------------- generic
GENERIC_RADIUS = 0.2
NOISE = (0.3, 0.7, 0.5)        # sigma of the normal noise of the three surfaces


def generic():
    """ellipsoid (800), the same with noisy normals (600), a sphere WITHOUT keypoints (400), a gently curved patch with slightly
    noisy normals (400; a flat patch with equal normals would make every pair a role tie) and, last, an exact copy of the first
    object. 16 keypoints each, 8 on surface points and 8 pulled 8 % towards the origin. Radius 0.2: in-ball counts <= ~50.
    All three surfaces carry normal noise (NOISE): on a smooth surface a ball of <= 50 out of >= 400 points spans so little
    curvature that a row has only ~12 populated bins, and a bin that stays empty on the device too proves nothing."""
    rng = np.random.default_rng(101)
    ep, en = ellipsoid(rng, 800)
    en = _unit(en + NOISE[0] * rng.normal(size=en.shape)).astype(f32)
    qp, qn = ellipsoid(rng, 600)
    qn = _unit(qn + NOISE[1] * rng.normal(size=qn.shape)).astype(f32)
    sp = _unit(rng.normal(size=(400, 3))).astype(f32)
    xy = rng.uniform(-0.6, 0.6, size=(400, 2))
    pp = np.concatenate([xy, 0.3 * (xy[:, :1] ** 2 - 0.5 * xy[:, 1:] ** 2) + 0.3 * xy[:, :1] * xy[:, 1:]], 1)
    g = np.stack([-(0.6 * xy[:, 0] + 0.3 * xy[:, 1]), -(-0.3 * xy[:, 1] + 0.3 * xy[:, 0]), np.ones(400)], 1)
    pn = _unit(_unit(g) + NOISE[2] * rng.normal(size=(400, 3))).astype(f32)
    pp = pp.astype(f32)

    def kps(p, scale):
        """8 keypoints on surface points and 8 pulled towards the centre, each with >= 20 neighbours and none closer than 0.2 r
        (a neighbour at 0.01 r would outweigh all others 400 : 1 and hide them; the pre-filters remove such twins upstream)"""
        out = []
        for sc_, want in ((1.0, 8), (scale, 16)):
            for i in rng.permutation(len(p)):
                q = (p[i].astype(np.float64) * sc_).astype(f32)
                d2 = ((p.astype(np.float64) - q) ** 2).sum(1)
                d2 = d2[d2 > 0]
                if (d2 < GENERIC_RADIUS ** 2).sum() >= 20 and d2.min() >= (0.2 * GENERIC_RADIUS) ** 2:
                    out.append(q)
                if len(out) == want:
                    break
        return f32(out)

    objs = [(ep, en), (qp, qn), (sp, sp.copy()), (pp, pn), (ep.copy(), en.copy())]
    k0 = kps(ep, 0.92)
    k = [k0, kps(qp, 0.92), np.zeros((0, 3), f32), kps(pp, 0.92), k0.copy()]
    return dict(objs=objs, kps=k, radius=GENERIC_RADIUS, cell=0.1, copy=(0, 4))


# ---------------------------------------------------------------------------------------------- f2 and f1 on the bin edges
def _ulps(a, i):
    """the float32 i ulps further from zero than a (a != 0)"""
    return (np.asarray(a, f32).view(np.int32) + np.asarray(i, np.int32)).view(f32)


def f2_edges():
    """30 Darboux objects (edge j = 1..10) x (float32 below / at / above the edge 2j/11 - 1). All three neighbours have b_y = -a, so
    f2 of the six centre pairs is EXACTLY a (module docstring: f2 = -b_y through products by 0 and 1 only); their (b_x, b_z) put f1 at
    t1 = 7.3, 8.5, 9.7 (chosen so that every feature of the neighbour-neighbour pairs stays > 0.04 from an edge too). The keypoint sits beside the centre, or on it for the 'at' objects."""
    objs, kps, meta = [], [], []
    for j in range(1, 11):
        e = f32(_edge(j))
        for v, a in enumerate((np.nextafter(e, f32(-2)), e, np.nextafter(e, f32(2)))):
            s = np.sqrt(1 - float(a) ** 2)
            nrm = [[_xz(s, t1)[0], -a, _xz(s, t1)[1]] for t1 in (7.3, 8.5, 9.7)]
            o, k = darboux_object(float(j % 4), nrm, kp_on_centre=v == 1)
            objs.append(o); kps.append(k); meta.append((j, v - 1, a))
    return dict(objs=objs, kps=kps, radius=DARBOUX_RADIUS, cell=DARBOUX_CELL, meta=meta, feature=1)


def atan2_inputs(target, s):
    """float32 (y, x) with |(y, x)| ~ s and numpy's float32 arctan2(y, x) == target, bit for bit: searched over the 65 x 65 float32
    neighbours of s (sin, cos)(target)"""
    y0, x0 = f32(s * np.sin(float(target))), f32(s * np.cos(float(target)))
    i = np.arange(-32, 33, dtype=np.int32)
    yy, xx = np.meshgrid(_ulps(y0, i), _ulps(x0, i), indexing="ij")
    hit = np.argwhere(np.arctan2(yy, xx) == f32(target))
    assert len(hit), target
    best = hit[np.argmin(np.abs(hit - 32).sum(1))]
    return yy[best[0], best[1]], xx[best[0], best[1]]


def f1_edges():
    """The same for f1. The centre pairs have y = b_x and x = b_z exactly, so f1 = atan2f(b_x, b_z) of two numbers the scene chooses:
    for the float32 g below / at / above the edge 2 pi j / 11 - pi, (b_x, b_z) is SEARCHED among the float32 neighbours of
    s (sin g, cos g) until numpy's float32 arctan2 returns g bit for bit (atan2f of another library may differ from it by an ulp;
    test_fpfh_cpu.py checks the oracle's value). b_y = -f2 puts f2 in the middle of bins 9, 8, 0 (s = |(b_x, b_z)| = 0.69, 0.84,
    0.42: |cos2| <= s stays below 12/13, and no two neighbours share their cosine)."""
    objs, kps, meta = [], [], []
    for j in range(1, 11):
        e = f32(2 * np.pi * j / 11 - np.pi)
        for v, g in enumerate((np.nextafter(e, f32(-4)), e, np.nextafter(e, f32(4)))):
            nrm = []
            for t2 in (9.5, 8.5, 0.5):
                f2 = 2 * t2 / 11 - 1
                y, x = atan2_inputs(g, np.sqrt(1 - f2 * f2))
                nrm.append([y, -f2, x])
            o, k = darboux_object(float(j % 4), nrm, kp_on_centre=v == 1)
            objs.append(o); kps.append(k); meta.append((j, v - 1, g))
    return dict(objs=objs, kps=kps, radius=DARBOUX_RADIUS, cell=DARBOUX_CELL, meta=meta, feature=0)


# ---------------------------------------------------------------------------------------------- the +-pi seam of f1
SEAM_TARGETS = ((0.6, -0.8), (0.28, -0.96), (0.8, -0.6))      # (b_y, b_z) of the three neighbours: x = b_z < 0, distinct |cos2|
SEAM_TINY, SEAM_CLEAR = 2.0 ** -40, 2.0 ** -12


def seam():
    """x = u . n_t < 0 throughout.
    objects 0..3  Darboux objects with b = (y, b_y, b_z), y = +2^-12 / -2^-12 / +2^-40 / -2^-40 for all three neighbours. y is exact in
                  any arithmetic (products by 0 and 1), so its sign and the bin (10 for +, 0 for -) are certain. The float64
                  reference can call only the +-2^-12 pairs decided (|y| / hypot = 3e-4 > SEAM); the +-2^-40 pairs fall under its
                  seam rule like any |y| at rounding-noise level, and there the device is held to the oracle's row.
    object 4      the signed-zero probe: b = (-0.0, b_y, b_z) and neighbours at y = -0.0 (centre at +0.0, so d_y = -0.0). In the
                  oracle's operation order every term of y = (w0 b0 + w1 b1) + w2 b2 is then -0.0 for the pairs whose source is
                  the centre: y = -0.0f, atan2f(-0, x < 0) = -pi -> bin 0 (a `y < 0` test would say +pi, bin 10).
                  test_fpfh_cpu.py confirms y = -0.0f in the float32 mode and bin 0 in the oracle's row.
    objects 5..8  the same frame turned by a seeded rotation, b = b_z u + b_y (-v) rounded to float32: y is mathematically 0 and
                  rounding noise in float32 -- undecided between bins 0 and 10, the oracle's operation order decides."""
    objs, kps = [], []
    for y in (SEAM_CLEAR, -SEAM_CLEAR, SEAM_TINY, -SEAM_TINY):
        o, k = darboux_object(float(len(objs) % 4), [[y, by, bz] for by, bz in SEAM_TARGETS])
        objs.append(o); kps.append(k)
    o, k = darboux_object(1.0, [[-0.0, by, bz] for by, bz in SEAM_TARGETS], nb_y=-0.0)
    objs.append(o); kps.append(k)
    rng = np.random.default_rng(303)
    for _ in range(4):
        R, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        (p, n), k = darboux_object(0.0, [[0.0, by, bz] for by, bz in SEAM_TARGETS])
        objs.append(((p.astype(np.float64) @ R.T).astype(f32), (n.astype(np.float64) @ R.T).astype(f32)))
        kps.append((k.astype(np.float64) @ R.T).astype(f32))
    return dict(objs=objs, kps=kps, radius=DARBOUX_RADIUS, cell=DARBOUX_CELL, clear=(0, 1), tiny=(2, 3), zero_probe=4,
                rotated=(5, 6, 7, 8))


# ---------------------------------------------------------------------------------------------- role swap ties
def swap_tie():
    """two-point objects p = (-a, 0, 0), q = (a, 0, 0), a = 1/16 (d = (1/8, 0, 0): the division by |d| is exact):
    0      mirror pair n_p = (-0.96, 0, 0.28), n_q = (0.96, 0, 0.28): cos1 = -0.96, cos2 = 0.96, |cos1| == |cos2| bit for bit (by
           symmetry both role assignments give the same features)
    1      n_p = (0.96, 0, 0.28), n_q = (0.96, 0.28, 0): cos1 == cos2 = 0.96 bit for bit, and the roles matter: f3 = +0.96 without
           the swap (bin 10), -0.96 with it (bin 0). PCL swaps on acos|cos1| > acos|cos2|, so a tie does not swap
    2, 3   object 1 with n_q.x one float32 ulp larger / smaller: the cosines 1 ulp apart, once in each direction. At 0.96 one ulp of
           the cosine is 7 ulps of its arccosine, so any acosf orders them and the roles follow the cosines
    4, 5   object 0 with n_q.x one ulp larger / smaller
    6..8   anti-parallel normals n_q = -n_p (exact tie in every precision), generic d: x = -1, y = 0 up to rounding (the seam too)
    9      120 points of a cap of the unit sphere with n = p (every pair a tie up to the rounding of the inputs; both role
           assignments give the same features there), 6 keypoints."""
    a = 1.0 / 16
    objs, kps = [], []
    s = f32(0.96)
    up, down = np.nextafter(s, f32(2)), np.nextafter(s, f32(0))
    for n_p, n_q in (([-0.96, 0, 0.28], [s, 0, 0.28]), ([0.96, 0, 0.28], [s, 0.28, 0]), ([0.96, 0, 0.28], [up, 0.28, 0]),
                     ([0.96, 0, 0.28], [down, 0.28, 0]), ([-0.96, 0, 0.28], [up, 0, 0.28]), ([-0.96, 0, 0.28], [down, 0, 0.28])):
        objs.append((f32([[-a, 0, 0], [a, 0, 0]]), f32([n_p, n_q])))
        kps.append(f32([[0, 0.03125, 0.0625]]))
    rng = np.random.default_rng(404)
    for _ in range(3):
        n = _unit(rng.normal(size=(1, 3)))[0]
        d = _unit(rng.normal(size=(1, 3)))[0] * 0.125
        nf = n.astype(f32)
        objs.append((f32([[0.5, 0.25, 0.125], np.array([0.5, 0.25, 0.125]) + d]), np.stack([nf, -nf])))
        kps.append(f32([[0.5, 0.25, 0.15625]]))
    cap = _unit(rng.normal(size=(120, 3)) * 0.12 + np.array([0.0, 0.0, 1.0])).astype(f32)
    objs.append((cap, cap.copy()))
    kps.append(np.concatenate([cap[:3], (cap[3:6].astype(np.float64) * 0.97).astype(f32)]))
    return dict(objs=objs, kps=kps, radius=0.2, cell=0.1, exact=(0, 1, 6, 7, 8), ulp=(2, 3, 4, 5), sphere=9)


# ---------------------------------------------------------------------------------------------- pole, degenerate, coincident
def pole_and_degenerate():
    """object 0  Darboux object with b = (0, -1, 0), (0, 1, 0) (n_t = +-v exactly: f2 = +-1, x = y = 0, the atan2 pole) and one
                 ordinary neighbour
    object 1     two points, d parallel to n_s (q = p + (0, 0, 1/8), n_p = (0, 0, 1)): |d x n_s| = 0 exactly, the pair is skipped
                 from both ends: both SPFH are zero and so is the row
    object 2     the same plus a third, ordinary point: the skipped pair changes the block total
    object 3     a curved 40-point patch; its point 0 three more times at identical coordinates (other normals); two isolated
                 points. Keypoints: on the fourfold point, beside it, beside isolated point A (a point alone in its ball: zero SPFH,
                 count 1), ON isolated point B (its only neighbour coincides with it: count 1, row of zeros), in the middle of
                 nowhere inside the grid (no neighbour: NaN), a NaN keypoint, a keypoint far outside the grid."""
    objs, kps = [], []
    o, k = darboux_object(1.0, [[0, -1, 0], [0, 1, 0], [0.48, 0.6, 0.64]])
    objs.append(o); kps.append(k)
    objs.append((f32([[0, 0, 0], [0, 0, 0.125]]), f32([[0, 0, 1], [0.6, 0, 0.8]])))
    kps.append(f32([[0.03125, 0, 0.0625]]))
    objs.append((f32([[0, 0, 0], [0, 0, 0.125], [0.125, 0.0625, 0.03125]]), f32([[0, 0, 1], [0.6, 0, 0.8], [0.28, 0.96, 0]])))
    kps.append(f32([[0.03125, 0, 0.0625]]))
    rng = np.random.default_rng(505)
    xy = rng.uniform(-0.25, 0.25, size=(40, 2))
    p = np.concatenate([xy, 0.8 * (xy[:, :1] ** 2 + 0.5 * xy[:, 1:] ** 2)], 1).astype(f32)
    n = _unit(np.stack([-1.6 * xy[:, 0], -0.8 * xy[:, 1], np.ones(40)], 1)).astype(f32)
    dup_n = _unit(rng.normal(size=(3, 3))).astype(f32)
    iso = f32([[2.0, 0.5, 0.25], [2.0, -1.5, 0.25]])
    p = np.concatenate([p, np.tile(p[:1], (3, 1)), iso])
    n = np.concatenate([n, dup_n, f32([[0, 0, 1], [0, 1, 0]])])
    objs.append((p, n))
    kps.append(f32([p[0], p[0] + f32([0.015625, 0, 0.03125]), iso[0] + f32([0.0625, 0, 0]), iso[1], [1.0, -0.5, 0.125],
                    [np.nan, 0, 0], [100.0, 100.0, 100.0]]))
    return dict(objs=objs, kps=kps, radius=0.25, cell=0.125, pole=0, degenerate=(1, 2), patch=3)


# ---------------------------------------------------------------------------------------------- neighbour counts of k_spfh
def queue_counts():
    """one object per count c of QUEUE_COUNTS: c - 1 points in a ball of radius 0.2 r around C and a rim point E = C + (0.6 r, 0, 0),
    all within r of each other, so n_E = c and k_spfh queues c - 1 pairs for E. The keypoint C + (1.55 r, 0, 0) lies 0.95 r from E
    and >= 1.35 r from everything else: E is its only neighbour, the row is SPFH(E) rescaled and one wrong pair moves a value by
    100 / (c - 1) >= 0.52."""
    rng = np.random.default_rng(606)
    r = 0.25
    objs, kps = [], []
    for j, c in enumerate(QUEUE_COUNTS):
        C = np.array([0.5 * (j % 3), 0.25 * (j % 2), 0.125 * j])
        q = C + _unit(rng.normal(size=(c - 1, 3))) * (0.2 * r * rng.uniform(0.2, 1.0, size=(c - 1, 1)) ** (1 / 3))
        p = np.concatenate([[C + [0.6 * r, 0, 0]], q]).astype(f32)
        objs.append((p, _unit(rng.normal(size=(c, 3))).astype(f32)))
        kps.append((C + [1.55 * r, 0, 0]).astype(f32).reshape(1, 3))
    return dict(objs=objs, kps=kps, radius=r, cell=0.125)


# ---------------------------------------------------------------------------------------------- neighbour counts of k_fpfh_sum
def sum_counts():
    """one object per count c of SUM_COUNTS: c points in a ball of radius 0.02 (far inside one grid cell of 0.25, so the keypoint's
    candidates are ONE cell row, gathered in steps of 64: 65 = 64 + 1) and a keypoint 0.03 beside its centre that sees them all.
    Last object: 300 points of an ellipsoid, four keypoints whose neighbours are spread over several cell rows, one step each."""
    rng = np.random.default_rng(707)
    objs, kps = [], []
    for j, c in enumerate(SUM_COUNTS):
        C = np.array([0.125 + (j % 3), 0.125, 0.125 + j % 2])
        p = (C + _unit(rng.normal(size=(c, 3))) * 0.02 * rng.uniform(0.1, 1.0, size=(c, 1)) ** (1 / 3)).astype(f32)
        objs.append((p, _unit(rng.normal(size=(c, 3))).astype(f32)))
        kps.append((C + [0.03, 0, 0]).astype(f32).reshape(1, 3))
    ep, en = ellipsoid(rng, 300)
    objs.append((ep, en))
    cand = (ep.astype(np.float64) * 0.98).astype(f32)
    dense = [i for i in range(300) if (((ep - cand[i]).astype(np.float64) ** 2).sum(1) < 0.25 ** 2).sum() >= 25][:4]
    kps.append(cand[dense])
    return dict(objs=objs, kps=kps, radius=0.25, cell=0.25, spread=len(SUM_COUNTS))


# ---------------------------------------------------------------------------------------------- exactly on the radius
def radius_probes(radius):
    """float32 distances (below, equal, above) along an axis from the origin: d * d rounded to float32 is the largest value < r2,
    == r2 and the smallest value > r2, r2 = float32(float64(float32(radius))^2)"""
    r = f32(radius)
    r2 = f32(np.float64(r) * np.float64(r))
    cand = _ulps(r, np.arange(-8, 9, dtype=np.int32))
    d2 = (cand * cand).astype(f32)
    assert (d2 == r2).any(), radius
    return cand[d2 < r2].max(), cand[d2 == r2][0], cand[d2 > r2].min()


def _radius_scene(radius):
    """object 0: the SOURCE point at the origin (exact differences) with neighbours at the three probe distances along x, y, z, five
    ordinary points around it and a keypoint beside it (k_spfh decides). Object 1: the KEYPOINT at the origin, the same three probe
    points, each with two ordinary companions, and three ordinary points near the keypoint (k_fpfh_mark and k_fpfh_sum decide)."""
    rng = np.random.default_rng(808)
    below, equal, above = radius_probes(radius)
    probes = f32([[below, 0, 0], [0, equal, 0], [0, 0, above]])
    near = (rng.uniform(-0.06, 0.06, size=(5, 3)) + [0.03, 0.03, 0.03]).astype(f32)
    p0 = np.concatenate([f32([[0, 0, 0]]), probes, near])
    comp = np.concatenate([probes + f32(o) for o in ([0.03125, 0.015625, 0.0625], [-0.0625, 0.03125, -0.015625])])
    near1 = (rng.uniform(-0.08, 0.08, size=(3, 3)) + [0.02, -0.03, 0.04]).astype(f32)
    p1 = np.concatenate([probes, comp, near1])
    nrm = lambda m: _unit(rng.normal(size=(m, 3))).astype(f32)
    objs = [(p0, nrm(len(p0))), (p1, nrm(len(p1)))]
    kps = [f32([[0.015625, 0.03125, 0.0078125]]), f32([[0, 0, 0]])]
    return dict(objs=objs, kps=kps, radius=radius, cell=float(radius) / 2, probes=(below, equal, above))


def exact_radius():
    """dyadic radius 1/4 (r2 = 1/16 exactly) and dyadic offsets"""
    return _radius_scene(0.25)


def inexact_radius():
    """the same probes at radius 0.3 (float32(0.3)^2 is not representable: r2 is the rounded product)"""
    return _radius_scene(0.3)


SCENES = dict(generic=generic, f1_edges=f1_edges, f2_edges=f2_edges, seam=seam, swap_tie=swap_tie,
              pole_and_degenerate=pole_and_degenerate, queue_counts=queue_counts, sum_counts=sum_counts,
              exact_radius=exact_radius, inexact_radius=inexact_radius)
_cache, _soa, _ref = {}, {}, {}


def scene(name):
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]


def arrays(name):
    """(pt_off, points, normals, kp_off, keypoints) of a scene, as the oracle and the C ABI take them"""
    if name not in _soa:
        _soa[name] = soa(scene(name)["objs"], scene(name)["kps"])
    return _soa[name]


def reference(name):
    """fpfh_ref.fpfh33 of a scene, computed once per process and shared by the tests"""
    if name not in _ref:
        import fpfh_ref
        _ref[name] = fpfh_ref.fpfh33(*arrays(name), scene(name)["radius"])
    return _ref[name]


def object_pairs(name, o):
    """(points, normals, src, tgt) of object o: every ordered pair of neighbours (all points as sources)"""
    import fpfh_ref
    p, n = scene(name)["objs"][o]
    _, src, tgt = fpfh_ref.neighbour_pairs(p, np.ones(len(p), bool), scene(name)["radius"])
    return p, n, src, tgt

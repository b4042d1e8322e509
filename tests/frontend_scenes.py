"""Seeded scenes for the descriptor front end, built for the branches the generic-position scenes never take (numpy only).

Each builder returns plain arrays, so the CPU tests can prove with grid_model that a scene reaches its path and the GPU tests can
run the kernels on exactly the same bytes. Every scene is an ordinary valid input."""
import numpy as np

f32 = np.float32

def soa(objs, kps):
    """ragged batch -> (pt_off, points, normals, kp_off, keypoints) as the oracle and the C ABI take them"""
    pt_off = np.concatenate([[0], np.cumsum([len(o[0]) for o in objs])]).astype(np.uint32)
    kp_off = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.uint32)
    cat = lambda parts: np.concatenate([np.asarray(a, f32).reshape(-1, 3) for a in parts]).astype(f32)
    return pt_off, cat([o[0] for o in objs]), cat([o[1] for o in objs]), kp_off, cat(kps)


def cols(a):
    return [np.ascontiguousarray(a[:, i]) for i in range(a.shape[1])]


# ---------------------------------------------------------------------------------------------- dense, wide batch
DENSE_CELL = 0.05
DENSE_RADIUS = 0.45
CLUMP_AT = np.array([0.2, 0.1, 0.33])
FAR_SHIFT = np.array([1000.0, -2500.0, 400.0])
FUSED_SURFACE = 45000          # + 20 000 clump points = 65 000: one workgroup builds the grid
WIDE_SURFACE = 60000           # + 20 000 = 80 000: past the fused build's limit, the five-kernel build
FPFH_RADIUS = 0.25
FPFH_OBJECT = 5                # the mid-sized object of the wide batch that carries the FPFH keypoints


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ellipsoid(rng, n, axes=(1.0, 0.6, 0.35)):
    d = _unit(rng.normal(size=(n, 3)))
    s = np.asarray(axes)
    return (d * s).astype(f32), _unit(d / s).astype(f32)


def dense_object(n_surface, seed=11):
    """ellipsoid surface + a 20 000-point Gaussian clump (sigma 0.004): balls of 5 000 - 28 000 neighbours, single cell rows that
    hold more candidates than one window of the traversal; 40 keypoints, 10 beside the clump and 30 on the surface"""
    rng = np.random.default_rng(seed)
    p, n = ellipsoid(rng, n_surface)
    clump = (CLUMP_AT + 0.004 * rng.normal(size=(20000, 3))).astype(f32)
    cn = _unit(rng.normal(size=(20000, 3))).astype(f32)
    pts, nrm = np.concatenate([p, clump]), np.concatenate([n, cn])
    near = (CLUMP_AT + rng.uniform(-0.03, 0.03, size=(10, 3))).astype(f32)
    surf = (p[rng.choice(n_surface, 30, replace=False)] * f32(0.98)).astype(f32)
    surf[0] = p[5]                                   # one keypoint coincides with a surface point
    return pts, nrm, np.concatenate([near, surf]).astype(f32)


def translated(pts, kp, shift=FAR_SHIFT):
    """the same object far from the origin (float32 sums: the grid there is coarser than the clump, many points coincide)"""
    return (pts.astype(np.float64) + shift).astype(f32), (kp.astype(np.float64) + shift).astype(f32)


def mid_object(seed=12, n_surface=6000, n_disc=2000):
    """ellipsoid + a thin dense disc on its top: ~8000 points, the object of the FPFH and PCA-normal sweeps with > 64 cell rows"""
    rng = np.random.default_rng(seed)
    p, n = ellipsoid(rng, n_surface)
    disc = (np.array([0.05, 0.03, 0.352]) + rng.normal(size=(n_disc, 3)) * np.array([0.03, 0.03, 0.0004])).astype(f32)
    dn = np.tile(f32([0, 0, 1]), (n_disc, 1))
    return np.concatenate([p, disc]), np.concatenate([n, dn]), rng


def wide_batch(n_surface, seed=21, with_color=True):
    """11 objects (>= 8 and no multiple of 8: the XCD block map deals one full group of 8 and a group of 3 objects + 5 padding
    slots), uneven keypoint counts:
    the dense object, its far-away copy, a mid-sized object, edge_scene-style small ones, an EMPTY and a 4-point object.
    Returns dict(objs=[(points, normals)], kps=[keypoints], rgba, kp_rgba, fpfh_kps=[keypoints for FPFH; only FPFH_OBJECT and the small ones])"""
    rng = np.random.default_rng(seed)
    dp, dn, dk = dense_object(n_surface)
    tp, tk = translated(dp, dk)
    mp, mn, mrng = mid_object()

    def sphere(n, scale, shift, noise=0.01):
        d = _unit(rng.normal(size=(n, 3)))
        return ((d * (1 + noise * rng.normal(size=(n, 1)))) * scale + shift).astype(f32), d.astype(f32)

    def plane(n, noise=0.02):
        p = np.concatenate([rng.uniform(-1, 1, size=(n, 2)), noise * rng.normal(size=(n, 1))], axis=1)
        return p.astype(f32), np.tile(f32([0, 0, 1]), (n, 1))

    e_p, e_n = ellipsoid(rng, 2500)
    e_p[::97] = np.nan                                                    # non-finite points never enter the search surface
    objs = [(dp, dn), sphere(3000, 1.0, 0.0), (np.zeros((0, 3), f32), np.zeros((0, 3), f32)), (tp, dn), sphere(4, 1.0, 0.0, 0.0),
            (mp, mn), (e_p, e_n), plane(2000), sphere(500, 0.3, [3.0, -2.0, 1.0]), sphere(1500, 0.8, [-40.0, 25.0, 60.0]), plane(700)]
    n_kp = [None, 42, 1, None, 4, 17, 33, 9, 3, 21, 6]
    kps = []
    for o, (p, _) in enumerate(objs):
        if o == 0:
            kps.append(dk)
        elif o == 3:
            kps.append(tk)
        elif len(p) == 0:
            kps.append(f32([[0.1, 0.2, 0.3]]))                            # a keypoint in an empty object
        else:
            ok = np.isfinite(p).all(1)
            sel = p[ok][rng.choice(ok.sum(), min(n_kp[o], ok.sum()), replace=False)]
            k = sel.copy(); k[1:] = (sel[1:].astype(np.float64) * 0.98 + 0.02 * sel[:1]).astype(f32)   # the first one sits on a surface point
            if o == 1:
                k[-2] = [30.0, 0, 0]; k[-1] = [np.nan, 0, 0]              # far away / non-finite keypoint
            kps.append(k.astype(f32))
    # FPFH: keypoints of the mid object whose ball (FPFH_RADIUS) lies inside the grid in y and z -> (2 * 5 + 1)^2 cell rows
    band = np.nonzero((np.abs(mp[:6000, 2]) < 0.07) & (np.abs(mp[:6000, 1]) < 0.3))[0]
    fk = [np.zeros((0, 3), f32) for _ in objs]
    fk[FPFH_OBJECT] = mp[mrng.choice(band, 12, replace=False)].astype(f32)
    for o in (1, 2, 4, 7, 8):
        fk[o] = kps[o][:5]
    out = dict(objs=objs, kps=kps, fpfh_kps=fk, rgba=None, kp_rgba=None)
    if with_color:
        out["rgba"] = [rng.integers(0, 1 << 24, size=len(o[0])).astype(np.uint32) for o in objs]
        out["kp_rgba"] = [rng.integers(0, 1 << 24, size=len(k)).astype(np.uint32) for k in kps]
    return out


# ---------------------------------------------------------------------------------------------- grid shape switch (x cells)
# make_grid_meta caps an axis at ISM_GRID_MAXDIM cells, and the wide batch's objects (2 wide at cell 0.05) sit at that cap on x for
# every x fraction: there ISMHIP_GRID_XFRAC changes nothing. Here the dense object is turned so that its SHORT axis (0.7) lies along
# x and the cell is large enough that x stays below the cap up to 5 cells per y/z cell, while a ball of radius 0.9 still covers
# ~ 11 x 11 cell rows and the clump fills single rows past a candidate window.
THIN_CELL = 0.12
THIN_RADIUS = 0.9
THIN_FPFH_RADIUS = 0.25
XFRACS = [1, 2, 5]             # the tested values of ISMHIP_GRID_XFRAC beside the default
_TURN = [2, 0, 1]              # new (x, y, z) = old (z, x, y)


def thin_batch(seed=22):
    """dense object turned thin along x, its far-away copy, the turned mid object (FPFH keypoints) and a small sphere"""
    rng = np.random.default_rng(seed)
    dp, dn, dk = dense_object(FUSED_SURFACE)
    dp, dn, dk = dp[:, _TURN].copy(), dn[:, _TURN].copy(), dk[:, _TURN].copy()
    tp, tk = translated(dp, dk, np.array([400.0, 1000.0, -2500.0]))
    mp, mn, mrng = mid_object()
    mp, mn = mp[:, _TURN].copy(), mn[:, _TURN].copy()
    d = _unit(rng.normal(size=(500, 3)))
    sp = (d * 0.3 + [3.0, -2.0, 1.0]).astype(f32)
    objs = [(dp, dn), (tp, dn), (mp, mn), (sp, d.astype(f32))]
    mk = (mp[mrng.choice(6000, 17, replace=False)] * f32(0.98)).astype(f32)
    kps = [dk, tk, mk, (sp[:3] * f32(0.99)).astype(f32)]
    fk = [np.zeros((0, 3), f32), np.zeros((0, 3), f32), mk[:8], kps[3]]
    return dict(objs=objs, kps=kps, fpfh_kps=fk,
                rgba=[rng.integers(0, 1 << 24, size=len(o[0])).astype(np.uint32) for o in objs],
                kp_rgba=[rng.integers(0, 1 << 24, size=len(k)).astype(np.uint32) for k in kps])


# ---------------------------------------------------------------------------------------------- FPFH through a second window
FPFH_CLUMP_RADIUS = 0.006
FPFH_CLUMP_POINTS = 7000


def fpfh_clump_object(seed=13):
    """ellipsoid + a 7000-point Gaussian clump (sigma 0.004) that sits inside one or two cell rows: with the small radius 0.006 a
    clump point has ~1 500 neighbours (the oracle stays quick) but its cell rows hold all 7000 candidates -- one row batch of
    k_spfh longer than a candidate window. Keypoints: three inside the clump."""
    rng = np.random.default_rng(seed)
    p, n = ellipsoid(rng, 6000)
    at = np.array([0.21, 0.12, 0.31])
    clump = (at + 0.004 * rng.normal(size=(FPFH_CLUMP_POINTS, 3))).astype(f32)
    cn = _unit(rng.normal(size=(FPFH_CLUMP_POINTS, 3))).astype(f32)
    kp = (at + rng.uniform(-0.002, 0.002, size=(3, 3))).astype(f32)
    return np.concatenate([p, clump]), np.concatenate([n, cn]), kp


# ---------------------------------------------------------------------------------------------- PCA normals over > 64 rows
NORMALS_CELL = 0.025
NORMALS_RADIUS = 0.15


def normals_scene():
    """the mid object (every point is a query: the disc's points sweep > 64 rows) + a small sphere + two isolated points (NaN)"""
    mp, _, rng = mid_object()
    mp[33] = np.nan
    sp = (_unit(rng.normal(size=(900, 3))) * 0.4 + [2.0, 1.0, -1.5]).astype(f32)
    return [mp, sp, f32([[0, 0, 0], [5, 5, 5]])]


# ---------------------------------------------------------------------------------------------- LRF sign ties
MIRROR_M = [400, 640, 641, 1500, 4096, 4097, 6000]
MIRROR_RADIUS = 2.5
MIRROR_CELL = 0.5
QUEUE_KEYPOINTS = 1100


def mirror_cloud(m, seed=31):
    """{p, -p}: every neighbour's mirror image votes the other way, so BOTH sign sums of the frame at the origin are exactly 0 and
    the five median neighbours decide; the anisotropy keeps the eigenvectors apart. The neighbourhood is the whole cloud (2 m)."""
    rng = np.random.default_rng(seed + m)
    base = (rng.normal(size=(m, 3)) * [0.3, 0.18, 0.1]).astype(f32)
    return np.concatenate([base, -base]).astype(f32)


def sign_sums(pts, frame):
    """2 * #(v . axis >= 0) - n for the x and z axes of a frame at the origin (double arithmetic on the float data)"""
    v = pts.astype(np.float64)
    f = np.asarray(frame, np.float64).reshape(3, 3)
    return tuple(int(2 * ((v @ f[a]) >= 0).sum() - len(v)) for a in (0, 2))


# ---------------------------------------------------------------------------------------------- SHOT boundary lattice
LATTICE_RADII = [0.25, 0.5, 0.75]
LATTICE_FRAMES = [f32([1, 0, 0, 0, 1, 0, 0, 0, 1]),          # identity
                  f32([0, 1, 0, 0, 0, 1, 1, 0, 0]),          # x -> y, y -> z, z -> x
                  f32([0, -1, 0, 1, 0, 0, 0, 0, 1])]         # quarter turn about z
COS_EDGES = [-0.9, -0.7, -0.5, -0.3, -0.1, 0.1, 0.3, 0.5, 0.7, 0.9]


def edge_cosines():
    """the float32 values at and either side of every cosine bin edge"""
    out = []
    for e in COS_EDGES:
        c = f32(e)
        out += [np.nextafter(c, f32(-2)), c, np.nextafter(c, f32(2))]
    return np.asarray(out, f32)


def lattice(frame):
    """the 729 points (k/8)^3, k = -4..4, keypoint at the origin. All coordinates are dyadic, so local coordinates, squared
    distances and the shell radius are EXACT in float32 and the hard decisions of the SHOT sector sit exactly on their edges:
    xl, yl, zl == 0, |xl| == |yl|, d^2 == r^2/4, d^2 == r^2. Normals: cosine to the frame's z axis = a float at / beside a bin edge."""
    g = np.arange(-4, 5) / 8.0
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    fr = np.asarray(frame, f32).reshape(3, 3)
    c = np.resize(edge_cosines(), len(p))
    rng = np.random.default_rng(41)
    c = c[rng.permutation(len(p))]
    n = c[:, None] * fr[2][None, :] + np.sqrt(1 - c.astype(np.float64) ** 2).astype(f32)[:, None] * fr[0][None, :]
    return p, n.astype(f32)


def lattice_census(p, frame, radius):
    """how many neighbours sit on each hard decision (exact: dyadic data)"""
    fr = np.asarray(frame, np.float64).reshape(3, 3)
    d2 = (p.astype(np.float64) ** 2).sum(1)
    inside = d2 < radius * radius
    loc = p[inside].astype(np.float64) @ fr.T
    return dict(n=int(inside.sum()), x0=int((loc[:, 0] == 0).sum()), y0=int((loc[:, 1] == 0).sum()), z0=int((loc[:, 2] == 0).sum()),
                diag=int((np.abs(loc[:, 0]) == np.abs(loc[:, 1])).sum()), shell=int((d2[inside] == radius * radius / 4).sum()),
                on_radius=int((d2 == radius * radius).sum()))


# colours for the lattice: neighbour colours whose CSHOT colour distance cd (float32) to the keypoint colour is the float below / at /
# above (k - 0.5) / 30, i.e. cd * 30 + 0.5 sits on an integer: the hard decision of the colour bin. To regenerate them (after a change
# of rgb2lab or of the colour distance): edge_colors(ora.rgb2lab, kp_color, range(1 << 24)) is the whole search; it calls rgb2lab once
# per candidate (minutes), so the list below was made by first narrowing the 2^24 colours with a numpy copy of Appendix A.3's LUT
# formulas and the same distance, then keeping what edge_colors confirms. test_frontend_cpu.py runs edge_colors on the list itself.
EDGE_KP_COLOR = 13887557
EDGE_COLORS = [497434, 534151, 562970, 599687, 821206, 1049944, 1115224, 1576308, 1690211, 3107279, 3497556, 4262870,
               5401079, 6590044, 6960031, 7366276, 8416626, 8626566, 8853227, 9513816, 10139714, 10361717, 10382487, 10843863,
               11158377, 11295425, 11481680, 11844545, 11888916, 11938814, 12086648, 12827198, 14723039, 15411660, 16061383]


def color_distance(lab_ref, lab):
    """CSHOT's colour distance of two raw CIELab triples, in float32 as Appendix A.3 states it"""
    (lr, ar, br), (l, a, b) = [(f32(v[0]) / f32(100), f32(v[1]) / f32(120), f32(v[2]) / f32(120)) for v in (lab_ref, lab)]
    cd = (abs(f32(lr - l)) + f32(f32(abs(f32(ar - a)) + abs(f32(br - b))) / f32(2))) / f32(3)
    return min(max(f32(cd), f32(0)), f32(1))


def edge_colors(rgb2lab, kp_color, candidates):
    """[(colour, k, side)] of the candidates whose colour distance to kp_color is the float32 below (side 0), at (1) or above (2)
    the bin edge (k - 0.5) / 30"""
    ref, out = rgb2lab(int(kp_color)), []
    for c in candidates:
        cd = color_distance(ref, rgb2lab(int(c)))
        k = int(round(float(cd) * 30 + 0.5))
        e = f32((k - 0.5) / 30.0)
        three = [np.nextafter(e, f32(-1)), e, np.nextafter(e, f32(2))]
        if cd in three:
            out.append((int(c), k, three.index(cd)))
    return out


def lattice_colors(p, seed=61):
    """random colours, except that the points nearest the keypoint (inside every test radius) carry the edge colours"""
    rng = np.random.default_rng(seed)
    rgba = rng.integers(0, 1 << 24, size=len(p)).astype(np.uint32)
    d2 = (p.astype(np.float64) ** 2).sum(1)
    near = np.argsort(d2, kind="stable")[1:27]                # the 26 lattice points within 0.25 (index 0 is the keypoint itself)
    rgba[near] = EDGE_COLORS[:26]
    far = np.argsort(d2, kind="stable")[27:27 + len(EDGE_COLORS) - 26]
    rgba[far] = EDGE_COLORS[26:]
    return rgba


# ---------------------------------------------------------------------------------------------- SHOT neighbour queue
QUEUE_COUNTS = [4, 5, 63, 64, 65, 127, 128, 129]
QUEUE_RADIUS = 0.3


def queue_clusters(seed=51):
    """one object of isolated clusters of exactly 4, 5, 63, 64, 65, 127, 128, 129 points, each within QUEUE_RADIUS of its own
    keypoint and > 2 radii from everything else, plus a 5-point cluster with a point ON the keypoint (the frame estimate sees
    4 neighbours -> NaN; SHOT on a supplied frame sees 5 -> finite). Returns points, normals, keypoints, frames, counts."""
    rng = np.random.default_rng(seed)
    pts, kps, counts = [], [], []
    for j, n in enumerate(QUEUE_COUNTS + [5]):
        c = np.array([2.0 * j, 0.5 * (j % 3), -0.25 * (j % 2)])
        q = c + _unit(rng.normal(size=(n, 3))) * rng.uniform(0.02, 0.25, size=(n, 1))
        if j == len(QUEUE_COUNTS):
            q[2] = c
        pts.append(q); kps.append(c); counts.append(n)
    pts = np.concatenate(pts).astype(f32)
    kps = np.asarray(kps, f32)
    pts[sum(counts[:-1]) + 2] = kps[-1]                     # coincident in float32 too
    nrm = _unit(rng.normal(size=(len(pts), 3))).astype(f32)
    frames = []
    for _ in kps:
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[2] = -q[2]
        frames.append(q.reshape(9))
    return pts, nrm, kps, np.asarray(frames, f32), np.asarray(counts)


# ---------------------------------------------------------------------------------------------- FPFH bin edges
FPFH_EDGE_RADIUS = 0.25


def fpfh_edge_objects():
    """30 four-point objects. Object (j, v): centre point with normal (a, sqrt(1 - a^2), 0), a = the float32 below / at / above the
    bin edge 2 j / 11 - 1 (j = 1..10), and three neighbours along +x at 1/64, 1/32, 1/16 with normal (0, 0.6, 0.8). Neighbour
    normals have zero x, so the centre's normal always plays n1 and f3 of every pair that involves the centre is EXACTLY a (dyadic
    spacings: the division is exact): inside the guard band of the fast bins, on both sides of the edge. f1 and f2 of those pairs
    and all three features of the neighbour-neighbour pairs sit far from any edge. With 4 points a wrong bin moves 100/3."""
    objs, kps = [], []
    for j in range(1, 11):
        e = f32(2.0 * j / 11.0 - 1.0)
        for v, a in enumerate((np.nextafter(e, f32(-2)), e, np.nextafter(e, f32(2)))):
            x0 = float(j % 4)                              # small integers: x0 + 2^-k is exact
            p = f32([[x0, 0, 0], [x0 + 1 / 64, 0, 0], [x0 + 1 / 32, 0, 0], [x0 + 1 / 16, 0, 0]])
            n = f32([[a, np.sqrt(1 - float(a) ** 2), 0]] + [[0, 0.6, 0.8]] * 3)
            objs.append((p, n))
            kps.append(f32([[x0, 0.0078125, 0]] if v != 1 else [[x0, 0, 0]]))       # beside / on the centre point
    return objs, kps

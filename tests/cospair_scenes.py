"""Seeded scenes for CoSPAIR (numpy only): the smallest inputs at which each decision of csrc/cospair.hip can go wrong. cospair_ref.py
gives the float64 intervals, test_cospair_cpu.py proves on the host that every scene reaches its decision and keeps inside the cap on
undecided deposits, test_gpu_cospair.py runs the kernels on the same bytes.
scene(name) -> dict(objs=[(points, normals)], rgba=[colours 0x00RRGGBB], kps=[keypoints], radius, cell, ...); every builder is seeded."""
import numpy as np

import fpfh_scenes as fps
from frontend_scenes import _unit, ellipsoid, soa

f32 = np.float32


def _colours(rng, n):
    return rng.integers(0, 1 << 24, size=n).astype(np.uint32)


def _noisy(rng, n, sigma):
    return _unit(n + sigma * rng.normal(size=n.shape)).astype(f32)


def _patch(rng, n, extent, centre=(0.0, 0.0, 0.0), sigma=0.2):
    """n points of a gently curved patch of radius `extent` around `centre` whose normals scatter by sigma around +z: every pair has
    a well-conditioned Darboux frame and a target normal far from the pole of f1 (which is perpendicular to the source normal), so
    even a ball of tens of thousands of pairs keeps its undecided deposits to the few that fall on a bin edge. Point 0 is the centre."""
    rad = extent * np.sqrt(rng.uniform(0, 1, size=n))
    phi = rng.uniform(0, 2 * np.pi, size=n)
    xy = np.stack([rad * np.cos(phi), rad * np.sin(phi)], 1)
    xy[0] = 0
    z = 0.6 * (xy[:, 0] ** 2 - 0.5 * xy[:, 1] ** 2) / extent + 0.08 * extent * rng.normal(size=n)
    z[0] = 0
    p = (np.concatenate([xy, z[:, None]], 1) + np.asarray(centre)).astype(f32)
    return p, _noisy(rng, np.tile([0.0, 0.0, 1.0], (n, 1)), sigma)


# ---------------------------------------------------------------------------------------------- shells, snap
SHELL_RADIUS = 0.875            # r_l = l / 8 and r2_l = l^2 / 64 exactly


def shells():
    """centre at the origin (index 0) with two coincident duplicates (indices 1, 2: other normals and colours; ordinary level-1 pairs
    that take the degenerate bins 4 / 4 / 4), two interior points of level 1, and points EXACTLY at d = r_l on the axes for l = 1, 2, 4,
    6, 7: d2 == r2_l puts them into level l + 1 (2, 3, 5, 7) and excludes the one at r_7. Levels 4 and 6 stay empty between populated
    ones. Keypoints: exactly on the centre (three points at d2 = 0: the lowest index is the centre); at (0, 3/8, 0), equidistant
    (1/8) from the points at (0, 2/8, 0) (index 6) and (0, 4/8, 0) (index 5, the lower index, listed first on purpose); 100 radii off
    the grid (snaps to the point with the largest x); beside an interior point."""
    rng = np.random.default_rng(901)
    p = f32([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0.0625, 0.03125, 0.015625], [-0.03125, 0.0625, -0.046875],
             [0, 0.5, 0], [0, 0.25, 0], [0.125, 0, 0], [0, 0, 0.75], [0.875, 0, 0], [0, 0, -0.125], [-0.25, 0, 0]])
    n = _unit(rng.normal(size=(len(p), 3))).astype(f32)
    n[0] = [0, 0, 1]
    kp = f32([[0, 0, 0], [0, 0.375, 0], [87.5, 0, 0], [0.0625, 0.03125, 0.0234375]])
    return dict(objs=[(p, n)], rgba=[_colours(rng, len(p))], kps=[kp], radius=SHELL_RADIUS, cell=0.35,
                want_snap=[0, 5, 9, 3], want_levels={0: [4, 2, 2, 0, 1, 0, 1]})


# ---------------------------------------------------------------------------------------------- queue
QUEUE_PAIRS = [1, 2, 63, 64, 65, 128, 129]
QUEUE_RADIUS = 0.25


def queue():
    """one object per count c: a centre with c patch points inside its ball and a keypoint a hair beside the centre"""
    rng = np.random.default_rng(902)
    objs, rgba, kps = [], [], []
    for j, c in enumerate(QUEUE_PAIRS):
        C = np.array([0.5 * (j % 3), 0.25 * (j % 2), 0.125 * j])
        p, n = _patch(rng, c + 1, 0.8 * QUEUE_RADIUS, C, sigma=0.4)
        objs.append((p, n)); rgba.append(_colours(rng, c + 1))
        kps.append((p[:1].astype(np.float64) + [0.001, 0.0005, 0.0]).astype(f32))
    return dict(objs=objs, rgba=rgba, kps=kps, radius=QUEUE_RADIUS, cell=0.1)


# ---------------------------------------------------------------------------------------------- hard decisions
def hard():
    """object 0  a Darboux object (fpfh_scenes: centre normal +z, neighbours at k (5, 0, 12) / 128, so f2 = -b_y, x = b_z, y = b_x and
                 f3 = 12/13 EXACTLY in any float32 order) with the target normals
                   (+0, 0.6, -0.8)   y = +0, x < 0: f1 = +pi exactly, deg_f1 = 360, bin 9 -> entry 9, which is f2's bin 0 (spill); f2 = -0.6: 126.9 deg, bin 6
                   (0, 1, 0)         f2 = -1 exactly: deg_f2 = 180, bin 9 -> entry 18, f3's bin 0 (spill); x = y = 0, the pole: f1 = 0, bin 4
                   (0, -1, 0)        f2 = +1: bin 0 -> entry 9; the pole again
    object 1     two points on a line along their common normal (d parallel to n): the cross product vanishes, PCL zeroes the
                 features, 4 / 4 / 4 -- the pair counts"""
    rng = np.random.default_rng(903)
    o0, k0 = fps.darboux_object(1.0, [[0.0, 0.6, -0.8], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], kp_on_centre=True)
    o1 = (f32([[0, 0, 0], [0, 0, 0.125]]), f32([[0, 0, 1], [0, 0, 1]]))
    objs, kps = [o0, o1], [k0, f32([[0, 0, 0]])]
    return dict(objs=objs, rgba=[_colours(rng, len(o[0])) for o in objs], kps=kps, radius=fps.DARBOUX_RADIUS, cell=fps.DARBOUX_CELL,
                # (object, level 0..6) -> geometry counts {entry: count} worked out by hand above; f3 = 12/13 -> acos = 22.6 deg, bin 1, entry 19
                want={(0, 1): {9: 1, 15: 1, 19: 1}, (0, 2): {4: 1, 18: 1, 19: 1}, (0, 4): {4: 1, 9: 1, 19: 1}, (1, 1): {4: 1, 13: 1, 22: 1}})


def _from_fpfh(name, seed):
    s = fps.scene(name)
    rng = np.random.default_rng(seed)
    return dict(objs=s["objs"], rgba=[_colours(rng, len(o[0])) for o in s["objs"]], kps=s["kps"], radius=s["radius"], cell=s["cell"], src=s)


def hard_seam():
    """the +-pi seam constructions of fpfh_scenes.seam, with seeded colours"""
    return _from_fpfh("seam", 904)


def hard_swap():
    """the role-swap ties of fpfh_scenes.swap_tie"""
    return _from_fpfh("swap_tie", 905)


def hard_pole():
    """pole, degenerate and coincident constructions of fpfh_scenes.pole_and_degenerate (a NaN keypoint, one far off the grid)"""
    return _from_fpfh("pole_and_degenerate", 906)


# ---------------------------------------------------------------------------------------------- palette
PALETTE = [("black", 0x000000), ("white", 0xFFFFFF), ("red", 0xFF0000), ("green", 0x00FF00), ("blue", 0x0000FF), ("cyan", 0x00FFFF),
           ("magenta", 0xFF00FF), ("yellow", 0xFFFF00), ("grey", 0x808080)]


def palette():
    """a centre and nine neighbours, one of each colour of PALETTE, all in level 7 of a keypoint on the centre: the colour array of
    that level holds exactly the palette's indices (test_cospair_cpu.py checks them against its hand table)"""
    rng = np.random.default_rng(907)
    ang = np.arange(9) * (2 * np.pi / 9)
    p = np.concatenate([[[0, 0, 0]], np.stack([0.23 * np.cos(ang), 0.23 * np.sin(ang), 0.02 * np.cos(3 * ang)], 1)]).astype(f32)
    n = _noisy(rng, np.tile([0.0, 0.0, 1.0], (10, 1)), 0.3)
    rgba = np.array([0x123456] + [c for _, c in PALETTE], np.uint32)
    return dict(objs=[(p, n)], rgba=[rgba], kps=[f32([[0, 0, 0]])], radius=0.25, cell=0.1)


# ---------------------------------------------------------------------------------------------- uniform colour
def uniform():
    """more than 4 000 neighbours of ONE colour: every colour deposit of a level hits the same three counters (the same-address worst case).
    One row of ~12 000 deposits: the seed is the first of 908.. at which none of them lies within the margin of a bin edge (the scene
    has to leave its single row fully decided, test_cospair_cpu.py::test_cap_on_undecided_deposits)"""
    rng = np.random.default_rng(912)
    p, n = _patch(rng, 4301, 0.24)
    return dict(objs=[(p, n)], rgba=[np.full(4301, 0x336699, np.uint32)], kps=[f32([[0.0005, 0.0, 0.0]])], radius=0.25, cell=0.1)


# ---------------------------------------------------------------------------------------------- thin batch
THIN_RADIUS = 0.3


def thin():
    """nine objects (one full group of eight of the XCD block map and a second group with padding blocks), ragged keypoint runs:
    0  a patch of 52 001 points inside one ball: a row of >= 50 000 pairs
    1  a small noisy ellipsoid, 6 keypoints          2  the same, NO keypoints
    3  an object of ONE point: the keypoint snaps to it, nothing else is there: the row is all zeros, finite, counts 0
    4  the ellipsoid with point 7 moved next to point 8 and given a NaN normal: a keypoint ON point 7 (NaN row) and one beside point 8 (its neighbour 7 is skipped
       and not counted)
    5  the ellipsoid, a NaN keypoint between two ordinary ones
    6, 7, 8  the ellipsoid with 4, 7 and 9 keypoints"""
    rng = np.random.default_rng(909)
    big = _patch(rng, 52001, 0.27)
    ep, en = ellipsoid(rng, 500, axes=(0.5, 0.3, 0.175))
    en = _noisy(rng, en, 0.3)
    bp, bad = ep.copy(), en.copy()
    bp[7] = ep[8] + f32([0.01, 0, 0]); bad[7] = np.nan
    pick = lambda m: (ep[rng.choice(500, m, replace=False)].astype(np.float64) * 0.98).astype(f32).reshape(-1, 3)
    objs = [big, (ep, en), (ep, en), (f32([[0.25, -0.5, 1.0]]), f32([[0, 1, 0]])), (bp, bad), (ep, en), (ep, en), (ep, en), (ep, en)]
    k5 = pick(3); k5[1] = [np.nan, 0, 0]
    kps = [f32([[0.0004, 0.0002, 0.0]]), pick(6), np.zeros((0, 3), f32), f32([[0.3, -0.5, 1.0]]),
           np.stack([bp[7], (bp[8].astype(np.float64) * 0.999).astype(f32)]), k5, pick(4), pick(7), pick(9)]
    return dict(objs=objs, rgba=[_colours(rng, len(o[0])) for o in objs], kps=kps, radius=THIN_RADIUS, cell=0.12, nan_rows=[8, 11],
                single_row=7, nan_neighbour_row=9, big_row=0)


# ---------------------------------------------------------------------------------------------- generic
def generic():
    """a coloured noisy ellipsoid of 7 000 points, 256 keypoints just inside its surface (the first one ON a point); ~170 pairs per row"""
    rng = np.random.default_rng(910)
    p, n = ellipsoid(rng, 7000)
    n = _noisy(rng, n, 0.3)
    kp = (p[rng.choice(7000, 256, replace=False)].astype(np.float64) * 0.98).astype(f32)
    kp[0] = p[11]
    return dict(objs=[(p, n)], rgba=[_colours(rng, 7000)], kps=[kp], radius=0.2, cell=0.08)


SCENES = dict(shells=shells, queue=queue, hard=hard, hard_seam=hard_seam, hard_swap=hard_swap, hard_pole=hard_pole, palette=palette,
              uniform=uniform, thin=thin, generic=generic)
CAPPED = ("generic", "queue", "thin", "uniform")         # the scenes held to the cap on undecided deposits
_cache, _soa, _ref = {}, {}, {}


def scene(name):
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]


def arrays(name):
    """(pt_off, points, normals, rgba, kp_off, keypoints) of a scene, as the C ABI takes them"""
    if name not in _soa:
        s = scene(name)
        pt_off, p, n, kp_off, kp = soa(s["objs"], s["kps"])
        _soa[name] = (pt_off, p, n, np.concatenate(s["rgba"]).astype(np.uint32), kp_off, kp)
    return _soa[name]


def reference(name, rgb2lab):
    """cospair_ref.cospair of a scene, computed once per process and shared by the tests"""
    if name not in _ref:
        import cospair_ref
        pt_off, p, n, rgba, kp_off, kp = arrays(name)
        _ref[name] = cospair_ref.cospair(rgb2lab, pt_off, p, n, rgba, kp_off, kp, scene(name)["radius"])
    return _ref[name]

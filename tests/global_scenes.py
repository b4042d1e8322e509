"""Seeded scenes for the region (global) descriptors, numpy only: the smallest shapes at which the one-workgroup-per-region kernel can
go wrong. Every object is a SKEWED blob (exponential along x and z), so the sign votes of its frame are far from a tie and the
eigenvalues are apart: the frame is stable against the last bits of the covariance. A case is a dict
  objs     list of (points [n, 3], normals [n, 3]) float32, one per object (non-finite points allowed)
  regions  list of (object, centre xyz or None, radius or None); None / None = the whole object
  cell     the grid cell of the cloud (the region kernel does not use the grid; the cloud needs one)"""
import numpy as np

f32 = np.float32
SIZES = [0, 1, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 4099]
BIG_N = 70000                     # above GRID_FUSED_MAX_PTS (65 536): the five-kernel grid build, 274 points per thread
TIE_M = 10000                     # 20 000 points: more than k_lrf_tie's LDS key store (8 192) and than 16 384


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def blob(rng, n, scale=(1.0, 0.6, 0.35), shift=(0.0, 0.0, 0.0)):
    """n points of a skewed anisotropic blob with random unit normals"""
    p = rng.normal(size=(n, 3))
    p[:, 0] = rng.exponential(size=n)
    p[:, 2] = 0.5 * rng.exponential(size=n) + 0.3 * p[:, 2]
    p = p * np.asarray(scale) * 0.2 + np.asarray(shift)
    return p.astype(f32), _unit(rng.normal(size=(max(n, 1), 3)))[:n].astype(f32)


def nan_object(k=3):
    return np.full((k, 3), np.nan, f32), np.full((k, 3), np.nan, f32)


def sizes_case(seed=101):
    """one whole-object region per size of SIZES; size 0 is an object of three NaN points"""
    rng = np.random.default_rng(seed)
    objs = [nan_object() if n == 0 else blob(rng, n, shift=rng.uniform(-1, 1, 3)) for n in SIZES]
    return dict(name="sizes", objs=objs, regions=[(o, None, None) for o in range(len(objs))], cell=0.1)


def big_case(seed=102):
    rng = np.random.default_rng(seed)
    return dict(name="big", objs=[blob(rng, BIG_N)], regions=[(0, None, None), (0, (0.2, 0.0, 0.1), 0.25)], cell=0.1)


def mixed_case(seed=103):
    """three objects of unequal size with non-finite points among them; two regions on object 1 and the regions in reverse object
    order; a region that selects nothing; one with fewer than five points; a selection radius with two points exactly on it"""
    rng = np.random.default_rng(seed)
    a, an = blob(rng, 700)
    b, bn = blob(rng, 3000, shift=(2.0, -1.0, 0.5))
    c, cn = blob(rng, 150, shift=(-3.0, 0.0, 0.0))
    a[0, 0], a[17, 1], a[699, 2] = np.nan, np.inf, -np.inf
    b[5, 2], b[1500, 0] = np.nan, np.nan
    c[149, 1] = np.nan
    # exact boundary on object 2: centre (-3, 0, 0) is exact in float32, radius 0.5; (0.5, 0, 0) and (0, -0.5, 0) from it have d2 == r2
    c[0] = [-2.5, 0.0, 0.0]
    c[1] = [-3.0, -0.5, 0.0]
    c[2] = [-3.0, 0.25, 0.0]
    regions = [(2, (-3.0, 0.0, 0.0), 0.5), (1, None, None), (1, (2.1, -1.0, 0.55), 0.12), (0, None, None), (0, (50.0, 50.0, 50.0), 0.3),
               (2, None, None), (1, (2.0, -1.0, 0.5), 0.004)]
    return dict(name="mixed", objs=[(a, an), (b, bn), (c, cn)], regions=regions, cell=0.1)


def tie_case(seed=104):
    """{p, -p} on a dyadic lattice (multiples of 2^-16): every coordinate sum is exact, the centroid is exactly the origin, both sign
    sums are exactly 0 and the five median neighbours by (distance, index) decide -- over 20 000 points"""
    rng = np.random.default_rng(seed)
    base = np.round(rng.normal(size=(TIE_M, 3)) * [0.3, 0.18, 0.1] * 65536.0) / 65536.0
    base = base[(base != 0).any(1)]
    p = np.concatenate([base, -base]).astype(f32)
    return dict(name="tie", objs=[(p, _unit(rng.normal(size=(len(p), 3))).astype(f32))], regions=[(0, None, None)], cell=0.5)


def needle_case(seed=105):
    """a thin needle along x: in a 1 x 1 x 8 grid the points crowd into the bins around phi = 0 and phi = +-180 (a centroid is the mean
    of its points, so ONE azimuth bin cannot hold them all); with 8 x 1 x 1 on `shell` and with 1 x 1 x 1 every point hits one address"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.exponential(size=3000), 2e-3 * rng.exponential(size=3000), 1e-3 * rng.normal(size=3000)], 1)
    return dict(name="needle", objs=[(p.astype(f32), _unit(rng.normal(size=(3000, 3))).astype(f32))], regions=[(0, None, None)], cell=0.2)


def shell_case(seed=106):
    """points at (almost) one distance, 1, from their centroid: a skewed density on a sphere, recentred, then pushed back onto the
    sphere; a mirror pair at distance 1.05 sets the radius without moving the centroid, so the shell sits clear of the ball's edge, at
    raw_r = 8 / 1.05 = 7.6 of an 8 x 1 x 1 grid: every point in the last bin"""
    rng = np.random.default_rng(seed)
    d = _unit(rng.normal(size=(2000, 3)) * [1.0, 0.6, 0.35] + [0.4, 0.0, 0.2])
    for _ in range(50):
        d = _unit(d - d.mean(0))
    u = np.array([[0.6, 0.0, 0.8]]) * 1.05
    d = np.concatenate([d, u, -u])
    return dict(name="shell", objs=[(d.astype(f32), _unit(d).astype(f32))], regions=[(0, None, None)], cell=0.2)


def all_cases():
    return [sizes_case(), big_case(), mixed_case(), tie_case(), needle_case(), shell_case()]


# (case name, bins, min_radius, log_radius): what the SHORT_SHOT_GLOBAL entry is run with on every case
GRIDS = {"sizes": [((2, 2, 8), 0.1, False), ((8, 4, 8), 0.1, False)], "big": [((2, 2, 8), 0.1, False)],
         "mixed": [((2, 2, 8), 0.1, False), ((4, 2, 8), 0.05, True)], "tie": [((2, 2, 8), 0.1, False)],
         "needle": [((1, 1, 8), 0.1, False), ((1, 1, 1), 0.1, False)], "shell": [((8, 1, 1), 0.1, False)]}


def finite_points(case, o):
    p, n = case["objs"][o]
    ok = np.isfinite(p).all(1)
    return p[ok], n[ok]

"""Scenes of the VoxelGridCulling tests (tests/test_culling_cpu.py, tests/test_gpu_culling.py, tests/test_gpu_culling_host.py) and the
selection cases worked by hand. Generic scenes are the bumpy ellipsoids of tests/iss3d_scenes.py with normals (the smooth ellipsoid's,
disturbed, so that the principal curvatures are far from a tie) and striped colours with jitter."""
import functools

import numpy as np

import culling_ref as ref
from iss3d_scenes import bumpy_ellipsoid

f32 = np.float32
FLT_MIN = ref.FLT_MIN
NAN, INF = np.nan, np.inf
# (points, LeafSize, seed): 300 - 2000 points, 20 - 150 keypoints
SCENES = ((2000, 0.15, 11), (1200, 0.2, 12), (300, 0.25, 13))


def normals_of(p, seed, noise=0.05):
    rng = np.random.default_rng(seed + 1000)
    n = p.astype(np.float64) / np.array([0.5, 0.35, 0.25]) ** 2 + rng.normal(scale=noise, size=p.shape) * np.linalg.norm(p / np.array([0.5, 0.35, 0.25]) ** 2, axis=1, keepdims=True)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)


def colors_of(p, seed):
    """two base colours in stripes along x, +-6 jitter per channel -> packed 0x00RRGGBB uint32"""
    rng = np.random.default_rng(seed + 2000)
    base = np.where((np.sin(14.0 * p[:, 0]) > 0)[:, None], np.array([200, 60, 40]), np.array([60, 90, 190]))
    c = np.clip(base + rng.integers(-6, 7, size=base.shape), 0, 255).astype(np.uint32)
    return (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]


def make(n, seed):
    xyz = bumpy_ellipsoid(n, seed)
    return dict(xyz=xyz, normals=normals_of(xyz, seed), rgba=colors_of(xyz, seed))


@functools.lru_cache(maxsize=None)
def scene(k):
    n, _leaf, seed = SCENES[k]
    s = make(n, seed)
    for a in s.values():
        a.setflags(write=False)
    return s


def concat(objs):
    """list of scene dicts -> (pt_off uint32 [n + 1], xyz, normals, rgba)"""
    off = np.concatenate([[0], np.cumsum([len(o["xyz"]) for o in objs])]).astype(np.uint32)
    cat = lambda key, shape, dt: (np.concatenate([o[key] for o in objs]) if len(objs) else np.zeros(shape, dt)).astype(dt)
    return off, cat("xyz", (0, 3), f32).reshape(-1, 3), cat("normals", (0, 3), f32).reshape(-1, 3), cat("rgba", (0,), np.uint32)


def sized(sizes, seed=21):
    """objects of the given point counts, cut from one bumpy ellipsoid each"""
    return [make(max(n, 1), seed + i) if n else dict(xyz=np.zeros((0, 3), f32), normals=np.zeros((0, 3), f32), rgba=np.zeros(0, np.uint32))
            for i, n in enumerate(sizes)]


def with_holes(s, seed=31):
    """NaN and +-inf points and normals interleaved"""
    rng = np.random.default_rng(seed)
    xyz, nrm = s["xyz"].copy(), s["normals"].copy()
    n = len(xyz)
    bad = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(rng.choice(n, n // 10, replace=False)):
        xyz[i, j % 3] = bad[j % 3]
    for j, i in enumerate(rng.choice(n, n // 10, replace=False)):
        nrm[i, (j + 1) % 3] = bad[(j + 2) % 3]
    return dict(xyz=xyz, normals=nrm, rgba=s["rgba"].copy())


def non_unit(s, seed=41):
    rng = np.random.default_rng(seed)
    return dict(xyz=s["xyz"], normals=(s["normals"] * rng.uniform(0.5, 3.0, size=(len(s["xyz"]), 1))).astype(f32), rgba=s["rgba"])


def plane_patch(n_side=24, step=0.01):
    g = np.arange(n_side, dtype=f32) * f32(step)
    x, y = np.meshgrid(g, g, indexing="ij")
    xyz = np.stack([x.ravel(), y.ravel(), np.zeros(n_side * n_side, f32)], 1).astype(f32)
    return dict(xyz=xyz, normals=np.tile(np.array([0, 0, 1], f32), (len(xyz), 1)), rgba=np.full(len(xyz), 0x00808080, np.uint32))


CYL_R, CYL_STEP, CYL_HALF = 1.0, 0.01, 40


def cylinder_strip():
    """one row of points on the unit cylinder round z, angles j * CYL_STEP, j = -CYL_HALF .. CYL_HALF, analytic normals"""
    phi = np.arange(-CYL_HALF, CYL_HALF + 1) * CYL_STEP
    n = np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)], 1)
    return dict(xyz=(CYL_R * n).astype(f32), normals=n.astype(f32), rgba=np.zeros(len(phi), np.uint32))


# ---- selection worked by hand -----------------------------------------------------------------------------------------------------------
# every case: g, c, the arguments of culling_ref.select / capi.culling_select, the expected keep mask and thresholds (geometry, colour, combined)
T, F = True, False
RATIO_BELOW_04 = float(np.nextafter(f32(0.4), f32(0)))      # float32(0.4) * 5 rounds to 2.0; one float below, the product is below 2
_G8 = [0, 1, 2, 3, 4, 5, 6, 8]           # / 8  -> 0 .125 .25 .375 .5 .625 .75 1
_C8 = [4, 4, 0, 0, 4, 0, 4, 2]           # / 4  -> 1 1 0 0 1 0 1 .5 ; combined 1 1.125 .25 .375 1.5 .625 1.75 1.5, sorted idx 4 -> 1.125
_GH = [0.2, 0.9, 0.6, 0.4, 0.7]
_CH = [0.1, 0.2, 0.3, 0.4, 0.5]
SELECT_CASES = [
    dict(name="one entry, combined", g=[0.3], c=[0.7], kw=dict(), keep=[T], thr=[0.3, 0.7, 0.0]),
    dict(name="one entry, require both", g=[0.3], c=[0.7], kw=dict(combine="RequireBoth"), keep=[T], thr=[0.3, 0.7, 0.0]),
    dict(name="two entries, geometry only", g=[2, 1], c=[0, 0], kw=dict(color_on=False), keep=[T, F], thr=[2, FLT_MIN, FLT_MIN]),
    dict(name="two entries, colour only", g=[0, 0], c=[1, 2], kw=dict(geo_on=False), keep=[F, T], thr=[FLT_MIN, 2, FLT_MIN]),
    dict(name="ratio * size exactly 2", g=[5, 1, 4, 2, 3], c=[0] * 5, kw=dict(color_on=False, ratio=0.4), keep=[T, F, T, F, T], thr=[3, FLT_MIN, FLT_MIN]),
    dict(name="ratio * size one float below 2", g=[5, 1, 4, 2, 3], c=[0] * 5, kw=dict(color_on=False, ratio=RATIO_BELOW_04), keep=[T, F, T, T, T],
         thr=[2, FLT_MIN, FLT_MIN]),
    dict(name="ties at the threshold", g=[1, 2, 2, 2, 3, 3, 0, 2], c=[0] * 8, kw=dict(color_on=False), keep=[F, T, T, T, T, T, F, T], thr=[2, FLT_MIN, FLT_MIN]),
    dict(name="NaN and inf, threshold inf", g=[NAN, INF, -INF, 1, NAN], c=[0] * 5, kw=dict(color_on=False), keep=[T, T, F, F, T], thr=[INF, FLT_MIN, FLT_MIN]),
    dict(name="NaN and inf, threshold NaN", g=[NAN, INF, -INF, 1, NAN], c=[0] * 5, kw=dict(color_on=False, ratio=0.7), keep=[T] * 5, thr=[NAN, FLT_MIN, FLT_MIN]),
    dict(name="all equal", g=[0.25] * 5, c=[0] * 5, kw=dict(color_on=False), keep=[T] * 5, thr=[0.25, FLT_MIN, FLT_MIN]),
    dict(name="gmax 0, combined", g=[-1, 0, -2], c=[0.5, 1, 0.25], kw=dict(), keep=[T, T, T], thr=[-1, 0.5, INF]),
    dict(name="gmax 0, both", g=[-1, 0, -2], c=[0.5, 1, 0.25], kw=dict(combine="RequireBoth"), keep=[T, T, F], thr=[-1, 0.5, INF]),
    dict(name="threshold and cutoff, combined", g=_GH, c=_CH, kw=dict(geo_type="threshold", geo_threshold=0.5), keep=[F, T, T, T, T], thr=[0.5, 0.3, FLT_MIN]),
    dict(name="threshold and cutoff, both", g=_GH, c=_CH, kw=dict(geo_type="threshold", geo_threshold=0.5, combine="RequireBoth"), keep=[F, F, T, F, T],
         thr=[0.5, 0.3, FLT_MIN]),
    dict(name="cutoff and threshold, one", g=_GH, c=_CH, kw=dict(color_type="threshold", color_threshold=0.25, combine="RequireOne"), keep=[F, T, T, T, T],
         thr=[0.6, 0.25, FLT_MIN]),
    dict(name="eight entries, one", g=_G8, c=_C8, kw=dict(combine="RequireOne"), keep=[T, T, F, F, T, T, T, T], thr=[4, 4, 1.125]),
    dict(name="eight entries, both", g=_G8, c=_C8, kw=dict(combine="RequireBoth"), keep=[F, F, F, F, T, F, T, F], thr=[4, 4, 1.125]),
    dict(name="eight entries, combined", g=_G8, c=_C8, kw=dict(combine="RequireCombinedList"), keep=[F, T, F, F, T, F, T, T], thr=[4, 4, 1.125]),
]

"""Seeded scenes for the two kernels in front of the path: PCA normals (lrf.hip) and voxel-grid keypoints (voxel.hip). numpy only.

As in frontend_scenes.py every builder returns plain arrays and every scene is an ordinary valid input; test_prepath_cpu.py proves
on the host that each scene reaches its case, the GPU tests run the kernels on the same bytes. Shapes are the smallest at which
the kernels can still go wrong."""
import itertools

import numpy as np

import frontend_scenes as fs

f32 = np.float32
R_NORMAL = 0.15
CELL = 0.06


def flat(objs):
    """list of [n, 3] arrays -> (pt_off uint32, points float32 [N, 3])"""
    off = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.uint32)
    return off, np.concatenate([np.asarray(o, f32).reshape(-1, 3) for o in objs]).astype(f32)


def _sphere(rng, n, noise):
    p = fs._unit(rng.normal(size=(n, 3)))
    return (p * (1.0 + noise * rng.normal(size=(n, 1)))).astype(f32)


# ---------------------------------------------------------------------------------------------- normals
def generic():
    """the objects of test_estimate_normals_pca: off-origin ellipsoid (4000), noisy sphere (3000), two isolated points; one NaN point"""
    rng = np.random.default_rng(50)
    o0 = fs.ellipsoid(rng, 4000)[0] + f32([1.5, -0.7, 0.4])
    o1 = _sphere(rng, 3000, 0.005) * f32(0.8) + f32([0.1, 0.2, 2.5])
    o2 = f32([[0, 0, 0], [5, 5, 5]])
    o0[17] = np.nan
    return dict(objs=[o0, o1, o2], radius=R_NORMAL, cell=CELL)


def far():
    """a 3000-point ellipsoid at (1000, -2500, 400): the float formula of the reference is meaningless there, the device's is not"""
    rng = np.random.default_rng(51)
    p = fs.ellipsoid(rng, 3000)[0]
    return dict(objs=[(p.astype(np.float64) + fs.FAR_SHIFT).astype(f32)], radius=R_NORMAL, cell=CELL)


def _int_vectors(norm2):
    """integer vectors with no zero component and the given squared norm, in a fixed order"""
    m = int(np.sqrt(norm2))
    return [v for v in itertools.product(range(-m, m + 1), repeat=3) if all(v) and sum(c * c for c in v) == norm2]


# planes of the radius probes as (in-plane step u, in-plane step w): three axis planes and the same turned by the 3-4-5 rotation
# (the turned axis advances by 5 h per step, so every coordinate stays a multiple of h)
PROBE_PLANES = [((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0)), ((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)),
                ((3, 4, 0), (0, 0, 1)), ((0, 3, 4), (1, 0, 0)), ((4, 0, 3), (0, 1, 0))]
N_ON, N_IN = 3, 3             # per probe: points exactly on the radius, points one float32 step inside it


def radius_scene(h, m, seed=52):
    """Per probe q (8 of them, 1.0 apart): a planar lattice patch of step h around q, N_ON off-plane points at q + h * v with
    |v|^2 = m^2 (v integer: their distance is exactly the radius r = m h when h is a power of two -> d2 == r2, NOT neighbours) and
    N_IN further such points moved one float32 step towards q along their longest component (d2 < r2: neighbours).
    h = 2^-6, m = 9 -> v = permutations of (+-1, +-4, +-8) [and (4,4,7), (3,6,6)], all decisions exact.
    h = 0.05, m = 3 -> v = permutations of (+-1, +-2, +-2), r = 0.15: products are inexact, the float32 reference decides.
    Returns dict(objs=[points], radius, cell, probes=[dict(q=index, on=[indices], inside=[indices])])."""
    rng = np.random.default_rng(seed)
    h = np.float64(f32(h))
    vecs = np.asarray(_int_vectors(m * m), np.float64)
    half = min(3, m - 1)
    pts, probes = [], []
    for k, (u, w) in enumerate(PROBE_PLANES):
        u, w = np.asarray(u, np.float64), np.asarray(w, np.float64)
        q = np.array([64.0 * (k + 1), 32.0 + 3 * k, 80.0 + 5 * k]) * h if h < 0.03 else np.array([1.0 + k, 0.5 + 0.15 * k, 1.25 + 0.25 * k])
        q = q.astype(f32).astype(np.float64)
        normal = np.cross(u, w)
        lat = [q + h * (i * u + j * w) for i in range(-half, half + 1) for j in range(-half, half + 1)
               if 0 < (i * u + j * w) @ (i * u + j * w) < m * m]
        off_plane = vecs[np.abs(vecs @ normal) > 0]
        pick = off_plane[rng.choice(len(off_plane), N_ON + N_IN, replace=False)]
        on = (q + h * pick[:N_ON]).astype(f32)
        inside = (q + h * pick[N_ON:]).astype(f32)
        for t, v in enumerate(pick[N_ON:]):
            a = int(np.argmax(np.abs(v)))
            inside[t, a] = np.nextafter(inside[t, a], f32(q[a]))
        base = sum(len(p) for p in pts)
        group = np.concatenate([[q], np.asarray(lat), on.astype(np.float64), inside.astype(np.float64)]).astype(f32)
        n_lat = 1 + len(lat)
        probes.append(dict(q=base, on=list(range(base + n_lat, base + n_lat + N_ON)),
                           inside=list(range(base + n_lat + N_ON, base + n_lat + N_ON + N_IN))))
        pts.append(group)
    return dict(objs=[np.concatenate(pts)], radius=float(f32(m * h)), cell=CELL, probes=probes)


def exact_radius():
    return radius_scene(2.0 ** -6, 9)


def inexact_radius():
    return radius_scene(0.05, 3)


MINIMAL_COUNTS = [2, 3, 4, 5, 6]
MINIMAL_TRI = f32([[0, 0, 0], [0.05, 0.01, 0], [0.01, 0.04, 0.02]])
MINIMAL_DIR = np.array([1.0, 2.0, -2.0]) / 3.0


def minimal():
    """one object of isolated groups 5 apart: 2 points (NaN), 3 points (their plane), 4 in general position, 5 coincident,
    6 exactly collinear (dyadic steps along (1, 2, -2): exact in float32). Returns groups = [(first index, count)]."""
    at = lambda g: np.array([3.0 + 5 * g, 1.0, 2.0])
    groups = [at(0) + f32([[0, 0, 0], [0.05, 0.02, 0.01]]),
              at(1) + MINIMAL_TRI,
              at(2) + f32([[0, 0, 0], [0.06, 0.01, 0], [0.01, 0.05, 0.02], [0.02, 0.02, 0.07]]),
              np.tile(at(3) + f32([0.01, 0.02, 0.03]), (5, 1)),
              at(4) + np.arange(6)[:, None] * np.array([1.0, 2.0, -2.0]) / 256.0]
    groups = [np.asarray(g, f32) for g in groups]
    start = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    return dict(objs=[np.concatenate(groups)], radius=R_NORMAL, cell=CELL, groups=[(int(start[i]), len(g)) for i, g in enumerate(groups)])


def row_batches():
    """frontend_scenes.normals_scene() unchanged: balls of 65 - 117 cell rows"""
    return dict(objs=fs.normals_scene(), radius=fs.NORMALS_RADIUS, cell=fs.NORMALS_CELL)


WIDE_SIZES = [37, 898, 0, 411, 50, 123, 650, 77, 333, 500, 205]       # 11 objects, largest no multiple of 4; [2] empty, [4] all NaN


def wide():
    """11 small objects (XCD block map: a full group of 8 and a group of 3 + 5 padding slots), one empty, one all NaN"""
    rng = np.random.default_rng(53)
    objs = []
    for o, n in enumerate(WIDE_SIZES):
        if o == 4:
            objs.append(np.full((n, 3), np.nan, f32))
            continue
        s = 0.02 * np.sqrt(max(n, 1))
        shift = np.array([1.5 * o - 6.0, 0.7 * (o % 3) + 0.4, 2.0 - 0.9 * (o % 4)])
        objs.append((_sphere(rng, n, 0.01).astype(np.float64) * s * np.array([1.0, 0.8, 0.6]) + shift).astype(f32))
    return dict(objs=objs, radius=R_NORMAL, cell=CELL)


NORMAL_SCENES = dict(generic=generic, far=far, exact_radius=exact_radius, inexact_radius=inexact_radius, minimal=minimal,
                     row_batches=row_batches, wide=wide)

M2_GROUPS = 90
M2_SPHERE = 2500


def method2():
    """for estimate_normals (frames at every point). Object 0: a noisy unit sphere of 2500 points with 90 isolated 4-point groups
    (frame invalid: 3 neighbours; PCA normal valid: 4 points in the ball) spread evenly through its index range and three NaN points
    among the first 40: k >= 360 invalid frames, so the run of 'first k finite points' crosses waves and 256-thread chunks and
    rank != index. Object 1: a dense sphere, every frame valid (k = 0). Object 2: three points (k = n = 3)."""
    rng = np.random.default_rng(54)
    sph = _sphere(rng, M2_SPHERE, 0.005).astype(np.float64) + np.array([0.3, -0.2, 0.1])
    tetra = np.array([[0, 0, 0], [0.06, 0.01, 0], [0.01, 0.05, 0.02], [0.02, 0.02, 0.07]])
    grp = []
    for g in range(M2_GROUPS):
        at = np.array([3.0 + (g % 10), -4.0 + (g // 10), 2.0 + 0.5 * (g % 3)])
        grp.append(at + tetra * rng.uniform(0.7, 1.0, size=(4, 1)) + 0.003 * rng.normal(size=(4, 3)))
    grp = np.concatenate(grp)
    n = M2_SPHERE + len(grp)
    slots = np.linspace(3, n - 1, len(grp)).astype(int)                 # the groups' points, evenly through the index range
    assert len(np.unique(slots)) == len(grp)
    o0 = np.empty((n, 3))
    is_grp = np.zeros(n, bool); is_grp[slots] = True
    o0[is_grp] = grp
    o0[~is_grp] = sph
    o0 = o0.astype(f32)
    nan_at = [i for i in range(40) if not is_grp[i]][5:35:12]
    o0[nan_at] = np.nan
    o1 = (_sphere(rng, 1500, 0.003).astype(np.float64) * 0.5 + np.array([-1.0, 2.0, 0.5])).astype(f32)
    o2 = (np.array([0.5, 0.5, -3.0]) + MINIMAL_TRI).astype(f32)
    return dict(objs=[o0, o1, o2], radius=R_NORMAL, cell=0.1, nan_at=nan_at, group_at=slots)


# ---------------------------------------------------------------------------------------------- voxel keypoints
def _colors(rng, n):
    return rng.integers(0, 1 << 24, size=n).astype(np.uint32)


def faces(leaf):
    """coordinates that are float32 multiples m * leaf, m = -7..7, and the float32 neighbours just below / above each: the float
    product p * (1 / leaf) decides the voxel, and floor differs from truncation for m <= 0. Object 0: 4000 random triples of those
    45 values per axis; object 1: the full 15^3 lattice, every coordinate independently below / at / above."""
    rng = np.random.default_rng(int(leaf * 1000) + 60)
    mult = (np.arange(-7, 8).astype(f32) * f32(leaf)).astype(f32)
    vals = np.stack([np.nextafter(mult, f32(-100)), mult, np.nextafter(mult, f32(100))], 1)            # [15, 3]
    o0 = vals.reshape(-1)[rng.integers(0, 45, size=(4000, 3))]
    g = np.stack(np.meshgrid(*[np.arange(15)] * 3, indexing="ij"), -1).reshape(-1, 3)
    o1 = vals[g, rng.integers(0, 3, size=g.shape)]
    objs = [o0.astype(f32), o1.astype(f32)]
    return dict(objs=objs, leaf=leaf, rgba=[_colors(rng, len(o)) for o in objs])


def crowded():
    """30 000 points inside ONE voxel (leaf 10, coordinates in [3, 4)) -- atomics contention, a sum 30 000 times the size of a
    term -- and 2000 points spread over [-50, 50). Below 65 000 points per voxel the 8-bit colour sums are exact in float32."""
    rng = np.random.default_rng(61)
    p = np.concatenate([rng.uniform(3, 4, size=(30000, 3)), rng.uniform(-50, 50, size=(2000, 3))]).astype(f32)
    p[:30000] = np.minimum(p[:30000], np.nextafter(f32(4), f32(0)))     # a float64 draw just below 4 must not round up to 4
    p = p[rng.permutation(len(p))]
    return dict(objs=[p], leaf=10.0, rgba=[_colors(rng, len(p))])


def far_voxels():
    rng = np.random.default_rng(62)
    p = (rng.uniform(0, 1, size=(5000, 3)) + fs.FAR_SHIFT).astype(f32)
    return dict(objs=[p], leaf=0.05, rgba=[_colors(rng, len(p))])


def sparse_table():
    """500 points in a 6.4-wide cube at leaf 0.05: a table of ~128^3 entries for 500 occupied ones (k_vox_emit: 8192 scan steps)"""
    rng = np.random.default_rng(63)
    p = rng.uniform(0, 6.4, size=(500, 3)).astype(f32)
    p[0] = 0.001; p[1] = 6.399
    return dict(objs=[p], leaf=0.05, rgba=[_colors(rng, len(p))])


RAGGED_EMPTY, RAGGED_NAN, RAGGED_SINGLE, RAGGED_DUP = 2, 4, 6, (8, 9)
RAGGED_DUP_POINT = f32([0.7234, -1.3377, 2.9001])


def ragged():
    """11 objects: [2] empty, [4] all NaN, [6] a single point, [8] and [9] 4 and 64 copies of ONE point, the rest random clouds with
    non-finite entries. With n a power of two float32(n * p) is exact, so float32(n * p) / n == p and the voxel's centroid is that
    point to the bit; for other n pcl::VoxelGrid's own formula need not return p (3 copies of 0.7234 give 0.72339994 in the oracle
    and on the device alike: fl(fl(3 p) / 3) may miss p by a float32 step)."""
    rng = np.random.default_rng(64)
    sizes = [700, 33, 0, 1200, 40, 257, 1, 512, 4, 64, 999]
    objs = []
    for o, n in enumerate(sizes):
        p = (rng.uniform(-1, 1, size=(n, 3)) * np.array([2.0, 1.0, 0.5]) + np.array([0.3 * o, -0.2 * o, 0.1])).astype(f32)
        if o == RAGGED_NAN:
            p[:] = np.nan
        elif o in RAGGED_DUP:
            p[:] = RAGGED_DUP_POINT
        elif n > 100:
            p[7] = np.nan; p[50, 1] = np.inf
        objs.append(p)
    return dict(objs=objs, leaf=0.3, rgba=[_colors(rng, len(o)) for o in objs])


VOXEL_SCENES = {"faces-0.25": lambda: faces(0.25), "faces-0.1": lambda: faces(0.1), "crowded": crowded, "far": far_voxels,
                "sparse_table": sparse_table, "ragged": ragged}


# ---------------------------------------------------------------------------------------------- built once per process
_built = {}


def normal_scene(name):
    """the scene with 'off', 'P' (flat arrays) and 'ref' (normals_ref.unoriented of it) added; built and computed once, never changed"""
    import normals_ref
    key = ("normals", name)
    if key not in _built:
        s = (method2 if name == "method2" else NORMAL_SCENES[name])()
        s["off"], s["P"] = flat(s["objs"])
        s["ref"] = normals_ref.unoriented(s["off"], s["P"], s["radius"])
        _built[key] = s
    return _built[key]


def voxel_scene(name):
    """the scene with 'ref' (voxel_ref.voxel_ref per object, with colours) added; built once"""
    import voxel_ref
    key = ("voxels", name)
    if key not in _built:
        s = VOXEL_SCENES[name]()
        s["ref"] = [voxel_ref.voxel_ref(p, s["leaf"], c) for p, c in zip(s["objs"], s["rgba"])]
        _built[key] = s
    return _built[key]

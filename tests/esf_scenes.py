"""The scenes of the ESF_LOCAL tests (tests/test_esf_local_cpu.py, tests/test_gpu_esf_local.py), computed once per process. A scene is a
ragged batch dict(pt_off, xyz, kp_off, kp, radius, n_samples). Most scenes are made of CLUSTERS: groups of points 10 units apart, each
with one keypoint whose ball holds exactly that group. n_samples is 1000 or 2000, neither a multiple of the kernel's 256-attempt blocks
(h), and 20000 (the library's constant, 78 blocks and 32) for the two keypoints of `full`.

answer(name) is the restatement esf_ref.py on the MODEL of the scale (esf_ref.scale_model), for the host tests; the device tests run the
restatement again on the device's own scale. transcript(name) is the float32 transcription per keypoint."""
import functools

import numpy as np

import esf_ref as ref

F = np.float32
GAP = 10.0
CAP = 64                        # the staging capacity the device tests force (ISMHIP_ESF_CAP)
COUNTS = [0, 1, 2, 3, 63, 64, 65, 130]


def _batch(objects, radius, n_samples):
    """objects: list of (xyz [n, 3], kp [k, 3])"""
    xyz = [np.asarray(p, F).reshape(-1, 3) for p, _ in objects]; kp = [np.asarray(k, F).reshape(-1, 3) for _, k in objects]
    return dict(pt_off=np.concatenate([[0], np.cumsum([len(p) for p in xyz])]).astype(np.uint32), xyz=np.concatenate(xyz),
                kp_off=np.concatenate([[0], np.cumsum([len(k) for k in kp])]).astype(np.uint32), kp=np.concatenate(kp),
                radius=float(F(radius)), n_samples=int(n_samples))


def _clusters(groups, radius, n_samples):
    """groups: list of (points relative to the cluster centre, keypoint relative to it); cluster g sits at (0, GAP g, 0), so cluster 0
    and the x and z coordinates of every cluster keep exact floats. One object."""
    xyz = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) + [0.0, GAP * g, 0.0] for g, (p, _) in enumerate(groups)])
    kp = np.stack([np.asarray(k, np.float64) + [0.0, GAP * g, 0.0] for g, (_, k) in enumerate(groups)])
    return _batch([(xyz, kp)], radius, n_samples)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _blob(rng, n, spread):
    return _unit(rng, n) * (spread * rng.uniform(0.02, 1.0, size=(n, 1)) ** (1 / 3))


# ---------------------------------------------------------------------------------------------------------------- (a) generic
def generic():
    """two objects of 400 points -- three blobs of different spread and a spherical shell -- with 8 keypoints each: 6 cloud points, one
    next to a cloud point and one far off the cloud (n = 0). 2000 samples."""
    rng = np.random.default_rng(2101)
    objs = []
    for o in range(2):
        centres = rng.uniform(-0.5, 0.5, size=(3, 3))
        p = np.concatenate([centres[0] + _blob(rng, 120, 0.12), centres[1] + _blob(rng, 100, 0.25), centres[2] + _blob(rng, 60, 0.4),
                            centres[0] + 0.3 * _unit(rng, 120)]).astype(F)
        pick = np.concatenate([rng.choice(120, 2, replace=False), 120 + rng.choice(100, 2, replace=False), 220 + rng.choice(60, 1), 280 + rng.choice(120, 1)])
        k = np.concatenate([p[pick], p[[5]] + F(0.01), [[7.0, 7.0, 7.0]]]).astype(F)
        objs.append((p, k[rng.permutation(8)]))
    return _batch(objs, 0.3, 2000)


# ---------------------------------------------------------------------------------------------------------------- (b) counts
def counts():
    """one keypoint per neighbour count of COUNTS: nothing, too few (0, 1, 2), the smallest ball that gives a row (3), one wavefront and
    the forced staging capacity less one, exactly, one more (63, 64, 65), and two capacities and two (130)"""
    rng = np.random.default_rng(2102)
    return _clusters([(_blob(rng, n, 0.1), (0.0, 0.0, 0.0)) for n in COUNTS], 0.3, 1000)


# ---------------------------------------------------------------------------------------------------------------- (c) three points
TRIANGLE = [(2.0, 0.0, 0.0), (-1.0, 1.5, 0.0), (-1.0, -1.5, 0.0)]


def triangle():
    """exactly three points about the keypoint (0, 0, 0): centroid 0, m = 2, so g = (32, 0, 0), (-16, 24, 0), (-16, -24, 0) without any
    rounding. Every sample is this triangle; test_esf_local_cpu.py derives the row by hand."""
    return _clusters([(TRIANGLE, (0.0, 0.0, 0.0))], 3.0, 1000)


# ---------------------------------------------------------------------------------------------------------------- (d) collinear
def collinear():
    """nine points x = -4 .. 4 on the x axis, the keypoint in the middle: c = 0, m = 4, g = 8 x, side lengths multiples of 8: Heron's
    product is 0 in float32 without a rounding. Every attempt is rejected, the cap is reached, the row is NaN. A second cluster holds
    five of them (m = 2), a third the same five along z."""
    line = lambda h: [(float(x), 0.0, 0.0) for x in range(-h, h + 1)]
    return _clusters([(line(4), (0.0, 0.0, 0.0)), (line(2), (0.0, 0.0, 0.0)), ([p[::-1] for p in line(2)], (0.0, 0.0, 0.0))], 4.5, 1000)


# ---------------------------------------------------------------------------------------------------------------- (e) flat disc
def disc():
    """four tilted discs of radius 0.25, each a jittered lattice of spacing 0.014 (under two voxels of the 32 that the radius becomes)
    and a third of a voxel thick, the keypoint near the middle: every line between two points stays inside occupied cells"""
    rng = np.random.default_rng(2105)
    groups = []
    for g in range(4):
        u = np.arange(-18, 19) * 0.014
        xy = np.stack(np.meshgrid(u, u, indexing="ij"), -1).reshape(-1, 2) + rng.uniform(-0.003, 0.003, size=(37 * 37, 2))
        xy = xy[np.linalg.norm(xy, axis=1) < 0.25]
        p = np.concatenate([xy, rng.uniform(-0.0013, 0.0013, size=(len(xy), 1))], 1)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        groups.append((p @ q.T, rng.uniform(-0.002, 0.002, size=3)))
    return _clusters(groups, 0.3, 1000)


# ---------------------------------------------------------------------------------------------------------------- (f) two clusters
def two_clusters():
    """per keypoint a dense blob of 150 points and a tight one of 40, 0.4 apart, the keypoint between them: lines inside the dense blob
    are IN, lines across the gap pass empty cells (MIXED, or OUT where the tight blob's end holds few cells)"""
    rng = np.random.default_rng(2106)
    groups = []
    for g in range(6):
        d = _unit(rng, 1)[0] * 0.2
        p = np.concatenate([d + _blob(rng, 150, 0.06), -d + _blob(rng, 40, 0.012)])
        groups.append((p, rng.uniform(-0.01, 0.01, size=3)))
    return _clusters(groups, 0.3, 1000)


# ---------------------------------------------------------------------------------------------------------------- (g) a copy
def copy():
    """object 0: a blob of 90 points about (0, 0, 0) after 25 far points; object 1: the same 90 points, same order, after 140 far points,
    its keypoints the same coordinates: another object, another index range, the same neighbourhoods"""
    rng = np.random.default_rng(2107)
    blob = _blob(rng, 90, 0.15).astype(F)
    far = (5.0 + rng.uniform(0, 1, size=(140, 3))).astype(F)
    kp = np.concatenate([blob[[3, 40]], [[0.01, 0.0, -0.02]], [[0.05, 0.05, 0.0]]]).astype(F)
    return _batch([(np.concatenate([far[:25], blob]), kp), (np.concatenate([far, blob]), kp)], 0.2, 1000)


# ---------------------------------------------------------------------------------------------------------------- 20000 samples
def full():
    """two keypoints of a 250-point blob at the library's own sample count"""
    rng = np.random.default_rng(2108)
    p = _blob(rng, 250, 0.2).astype(F)
    return _batch([(p, p[[0, 100]])], 0.25, ref.SAMPLES)


SCENES = dict(generic=generic, counts=counts, triangle=triangle, collinear=collinear, disc=disc, two_clusters=two_clusters, copy=copy,
              full=full)


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def answer(name):
    s = scene(name)
    return ref.esf_local(s["pt_off"], s["xyz"], s["kp_off"], s["kp"], s["radius"], s["n_samples"])


@functools.lru_cache(maxsize=None)
def transcript(name):
    """esf32 per keypoint (None where the ball holds fewer than three points) on the model scale"""
    s, a = scene(name), answer(name)
    out = []
    for k in range(len(s["kp"])):
        b = a["balls"][k]
        out.append(None if len(b) < 3 else ref.esf32(s["xyz"][b], a["scale"][k, :3], a["scale"][k, 3], s["n_samples"]))
    return out

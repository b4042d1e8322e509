"""The scenes of the RSD tests (tests/test_rsd_cpu.py, tests/test_gpu_rsd.py) and their answers by the restatement tests/rsd_ref.py,
computed once per process. A scene is a ragged batch: dict(pt_off, xyz, normals, kp_off, kp, radius). Most scenes are made of CLUSTERS:
small groups of points 10 units apart, each with one keypoint whose ball holds exactly that group, so a keypoint's neighbourhood is
written down point by point."""
import functools

import numpy as np

import rsd_ref as ref

F = np.float32
X = (1.0, 0.0, 0.0)
GAP = 10.0                       # between cluster centres: far more than any radius used here


def _one(xyz, normals, kp, radius):
    xyz = np.asarray(xyz, F).reshape(-1, 3); normals = np.asarray(normals, F).reshape(-1, 3); kp = np.asarray(kp, F).reshape(-1, 3)
    assert len(xyz) == len(normals)
    return dict(pt_off=np.array([0, len(xyz)], np.uint32), xyz=xyz, normals=normals, kp_off=np.array([0, len(kp)], np.uint32), kp=kp,
                radius=float(F(radius)))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _clusters(groups, radius):
    """groups: list of (points relative to the cluster centre [m, 3], normals [m, 3], keypoint relative to the centre [3]); cluster g sits
    at (GAP g, 0, 0). The centres are integers, so small relative coordinates keep their low bits only roughly: scenes that need exact
    floats put them in y and z, or use cluster 0."""
    xyz, nrm, kp = [], [], []
    for g, (p, n, k) in enumerate(groups):
        c = np.asarray([GAP * g, 0.0, 0.0])
        p = np.asarray(p, np.float64).reshape(-1, 3)
        xyz.append(p + c); nrm.append(np.asarray(n, np.float64).reshape(-1, 3)); kp.append(np.asarray(k, np.float64) + c)
    return _one(np.concatenate(xyz), np.concatenate(nrm), np.stack(kp), radius)


# ---------------------------------------------------------------------------------------------------------------- (a) generic
def generic():
    """four objects of 300 points (three blobs of 130, 100 and 70 points and different spread each) with unit normals, 16 keypoints each: 12 cloud points, 2 next to
    cloud points, one in the sparse outskirts and one far off the cloud (n = 0)"""
    rng = np.random.default_rng(101)
    xyz, nrm, kp = [], [], []
    for o in range(4):
        centres = rng.uniform(-1.0, 1.0, size=(3, 3))
        sig = np.asarray([0.11, 0.22, 0.45])[:, None]
        p = np.concatenate([centres[b] + sig[b] * rng.normal(size=(m, 3)) for b, m in enumerate((130, 100, 70))]).astype(F)
        n = _unit(rng, 300)
        n[:130] = (_unit(rng, 1) + 0.3 * rng.normal(size=(130, 3))).astype(F)        # a blob of nearly parallel normals: angle bins 0 and 1
        n[:130] /= np.linalg.norm(n[:130], axis=1, keepdims=True)
        pick = np.concatenate([rng.choice(130, 5, replace=False), 130 + rng.choice(100, 4, replace=False), 230 + rng.choice(70, 3, replace=False)])
        k = np.concatenate([p[pick], p[[3, 150]] + F(0.01), p[[250]] + F(0.6), [[7.0, 7.0, 7.0]]]).astype(F)
        xyz.append(p); nrm.append(n); kp.append(k[rng.permutation(16)])
    return dict(pt_off=(np.arange(5) * 300).astype(np.uint32), xyz=np.concatenate(xyz), normals=np.concatenate(nrm).astype(F),
                kp_off=(np.arange(5) * 16).astype(np.uint32), kp=np.concatenate(kp), radius=float(F(0.3)))


# ---------------------------------------------------------------------------------------------------------------- (b) counts
COUNTS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129]


def _ball_cluster(rng, n, spread=0.1):
    d = _unit(rng, n).astype(np.float64) * (spread * rng.uniform(0.05, 1.0, size=(n, 1)) ** (1 / 3))
    return d, _unit(rng, n), (0.0, 0.0, 0.0)


def counts():
    """one keypoint per neighbour count of COUNTS: the empty neighbourhood, the single point, the smallest odd and even circles, and one
    below, on and above one and two wavefronts of neighbours"""
    rng = np.random.default_rng(201)
    return _clusters([_ball_cluster(rng, n) for n in COUNTS], 0.3)


# ---------------------------------------------------------------------------------------------------------------- (c) angle edges
ANGLE_EDGE_KEYPOINTS = []        # (k, side) for the edge keypoints, then the names of the special ones


def angle_edges():
    """two-point neighbourhoods 0.1 apart (distance bin 1 at radius 0.3). The normals are (1, 0, 0) and (x, y, 0): c = (1 * x + 0 * y) + 0 * 0
    = x exactly, so a is the float written here: the float nearest to cos(k pi / 10) and its two neighbours, k = 1..4. Then c = 1, c = -1,
    a c that rounds above 1, and antiparallel generic normals."""
    ANGLE_EDGE_KEYPOINTS.clear()
    groups = []
    pts = [[0.0, -0.05, 0.0], [0.0, 0.05, 0.0]]

    def add(n0, n1, name):
        groups.append((pts, [n0, n1], (0.0, 0.0, 0.0)))
        ANGLE_EDGE_KEYPOINTS.append(name)

    for k in range(1, 5):
        e = F(np.cos(k * np.pi / 10))
        for side, x in (("below", np.nextafter(e, F(-1))), ("at", e), ("above", np.nextafter(e, F(2)))):
            add(X, (float(x), float(np.sqrt(1.0 - float(x) ** 2)), 0.0), (k, side))
    add(X, X, "c = 1")
    add(X, (-1.0, 0.0, 0.0), "c = -1")
    rng = np.random.default_rng(301)
    while True:                                                          # a unit vector (in float) whose float dot with itself exceeds 1
        v = _unit(rng, 1)[0]
        c = F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2]))
        if c > F(1.0):
            break
    add(v, v, "c above 1")
    u = _unit(rng, 1)[0]
    w = _unit(rng, 1)[0]
    add(u, w, "generic")
    add(u, -w, "antiparallel")
    return _clusters(groups, 0.3)


# ---------------------------------------------------------------------------------------------------------------- (d) distance edges
DIST_EDGE_KEYPOINTS = []
DIST_R = 0.5                     # exact in float; k R / 5 is not


def dist_edges():
    """two-point neighbourhoods on the y axis of their cluster, (0, 0, 0) and (0, y, 0): d2 = y * y in float. y: the float nearest to k R / 5
    and its two neighbours, k = 1..4, the keypoint half way. Then, in cluster 0 where the coordinates are exact: -R/2 and +R/2 on the x axis
    about the keypoint (dist == R exactly, both inside the ball: distance bin 4) and the same pair one ulp of R wider (neglected); two
    coincident points (dist 0)."""
    DIST_EDGE_KEYPOINTS.clear()
    n2 = [X, (0.8, 0.6, 0.0)]
    groups = [([[-0.25, 0, 0], [0.25, 0, 0], [-0.25, 3.0, 0], [0.25 + 2.0 ** -24, 3.0, 0], [0.1, 6.0, 0.05], [0.1, 6.0, 0.05]], n2 * 3, (0.0, 0.0, 0.0))]
    DIST_EDGE_KEYPOINTS.append("dist == R")
    for k in range(1, 5):
        e = F(k * DIST_R / 5)
        for side, y in (("below", np.nextafter(e, F(0))), ("at", e), ("above", np.nextafter(e, F(1)))):
            groups.append(([[0, 0, 0], [0, float(y), 0]], n2, (0.0, float(y) / 2, 0.0)))
            DIST_EDGE_KEYPOINTS.append((k, side))
    s = _clusters(groups, DIST_R)
    # the two other keypoints of cluster 0
    s["kp"] = np.concatenate([s["kp"], np.asarray([[0, 3.0, 0], [0.1, 6.0, 0.05]], F)])
    s["kp_off"] = np.array([0, len(s["kp"])], np.uint32)
    DIST_EDGE_KEYPOINTS.extend(["one ulp wider", "coincident"])
    return s


# ---------------------------------------------------------------------------------------------------------------- (e) overflow
OVERFLOW = [64, 65, 130, 200, 256, 257, 300, 520]
OVERFLOW_CAP = 64


def overflow():
    """neighbourhoods about the staging capacity: 64 and 65 (the capacity under ISMHIP_RSD_CAP=64 and one more), 130 and 200 (three and four
    tiles there, the last one partial), 256, 257, 300 and 520 (the native capacity, one more, two and three tiles)"""
    rng = np.random.default_rng(401)
    return _clusters([_ball_cluster(rng, n) for n in OVERFLOW], 0.3)


# ---------------------------------------------------------------------------------------------------------------- (f) radii by hand
RADII_THETA = [(1, 0.2), (1, 0.7), (2, 0.4), (2, 1.2), (3, 0.5), (3, 1.5), (4, 0.8), (4, 1.3)]     # (distance bin, angle)
RADII_R = 0.5


def radii():
    """keypoint 0: 50 points on a plane patch with one normal: every theta is 0, both sums of squares vanish, both radii 1.1f * R.
    Then two-point neighbourhoods whose one pair has the angle theta in distance bin d >= 1 (the points (d + 0.5) R / 5 apart: mid bin):
    bin 0 contributes 0, so Amin2 = Amax2 = theta^2 and both radii are 1.1f * min(f_d / theta, R)."""
    rng = np.random.default_rng(501)
    plane = np.concatenate([rng.uniform(-0.2, 0.2, size=(50, 2)), np.zeros((50, 1))], 1)
    groups = [(plane, np.tile(np.asarray([0.0, 0.0, 1.0]), (50, 1)), (0.0, 0.0, 0.0))]
    for d, th in RADII_THETA:
        y = (d + 0.5) * RADII_R / 5
        groups.append(([[0, 0, 0], [0, y, 0]], [X, (np.cos(th), np.sin(th), 0.0)], (0.0, y / 2, 0.0)))
    return _clusters(groups, RADII_R)


SCENES = {"generic": generic, "counts": counts, "angle_edges": angle_edges, "dist_edges": dist_edges, "overflow": overflow, "radii": radii}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def answer(name):
    """the restatement's dict for the scene (rsd_ref.rsd); treat as read-only"""
    s = scene(name)
    return ref.rsd(s["pt_off"], s["xyz"], s["normals"], s["kp_off"], s["kp"], s["radius"])

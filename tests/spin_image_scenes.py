"""The scenes of the SpinImage tests (tests/test_spin_image_cpu.py, tests/test_gpu_spin_image.py) and their answers by the restatement
tests/spin_image_ref.py, computed once per process. A scene is a ragged batch: dict(pt_off, xyz, normals, kp_off, kp, radius, w).
The axes are always looked up (spin_image_ref.batch_normals), so a scene sets an axis by installing it as the matched point's normal."""
import functools

import numpy as np

import spin_image_ref as ref

F = np.float32
Z = (0.0, 0.0, 1.0)
SQRT2 = float(F(np.sqrt(2.0)))


def _one(xyz, normals, kp, radius, w=8):
    xyz = np.asarray(xyz, F).reshape(-1, 3); normals = np.asarray(normals, F).reshape(-1, 3); kp = np.asarray(kp, F).reshape(-1, 3)
    return dict(pt_off=np.array([0, len(xyz)], np.uint32), xyz=xyz, normals=normals, kp_off=np.array([0, len(kp)], np.uint32), kp=kp,
                radius=float(F(radius)), w=w)


def _sphere_points(seed, n):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)); p /= np.linalg.norm(p, axis=1, keepdims=True)
    return p.astype(F)


def sphere(w=8):
    """(a) 3000 points on the unit sphere, normals = positions, 64 keypoints that are cloud points"""
    p = _sphere_points(11, 3000)
    kp = p[np.random.default_rng(12).choice(len(p), 64, replace=False)]
    return _one(p, p, kp, 0.4, w)


def hand3():
    """(b) centre at the origin, axis +z, radius sqrt(2) (bin 0.125): (0.1875, 0, 0.0625) twice -> alpha / bin = 1.5, beta / bin = 0.5"""
    return _one([[0, 0, 0], [0.1875, 0, 0.0625], [0.1875, 0, 0.0625]], [Z, Z, Z], [[0, 0, 0]], SQRT2)


def off_cloud():
    """(c) keypoints next to cloud points, never on one"""
    p = _sphere_points(21, 800)
    kp = p[:12] * F(1.001)
    return _one(p, p, kp, 0.4)


def twins():
    """(d) point 40 repeats point 7 with another normal; point 7's is handed over"""
    p = _sphere_points(31, 600)
    n = p.copy()
    p[40] = p[7]
    n[40] = np.roll(n[7], 1)
    return _one(p, n, p[[7, 40, 100]], 0.4)


def scaled_axis():
    """(e) two objects with the same points; the centre's installed normal is 1.5 z (a neighbour along it: cosine 1.5) and 0.5 z"""
    rng = np.random.default_rng(41)
    p = np.concatenate([[[0, 0, 0], [0, 0, 0.2]], rng.uniform(-0.3, 0.3, size=(200, 3))]).astype(F)
    n = np.tile(np.asarray(Z, F), (len(p), 1))
    n15, n05 = n.copy(), n.copy()
    n15[0] = (0, 0, 1.5); n05[0] = (0, 0, 0.5)
    return dict(pt_off=np.array([0, len(p), 2 * len(p)], np.uint32), xyz=np.concatenate([p, p]), normals=np.concatenate([n15, n05]),
                kp_off=np.array([0, 1, 2], np.uint32), kp=np.zeros((2, 3), F), radius=0.5, w=8)


COUNT_KEYPOINTS = ["empty ball", "off the grid", "itself only", "outside the cylinder", "keypoint not finite", "normal not finite"]


def counts():
    """(f) one keypoint per case of COUNT_KEYPOINTS, radius 0.4 (lim 0.283)"""
    xyz = [[0, 0, 0], [10, 10, 10], [3, 3, 3], [6, 0, 0], [6.35, 0, 0], [6, 0.35, 0], [1, 1, 1]]
    n = np.tile(np.asarray(Z, F), (len(xyz), 1))
    n[6] = (np.nan, 0, 0)
    kp = [[5, 5, 5], [100, 0, 0], [3, 3, 3], [6, 0, 0], [np.nan, 0, 0], [1, 1, 1]]
    return _one(xyz, n, kp, 0.4)


CYLINDER_PLANTED = 3        # of the six planted neighbours, the three on the inner side


def cylinder():
    """(g) neighbours planted at alpha and |beta| = lim (1 -+ 1e-6) about the origin, axis +z, radius 0.5"""
    _, lim = ref.bin_of(0.5, 8)
    lo, hi = lim * (1.0 - 1e-6), lim * (1.0 + 1e-6)
    xyz = [[0, 0, 0], [lo, 0, 0.01], [hi, 0, 0.01], [0.01, 0, lo], [0.01, 0, hi], [0.01, 0, -lo], [0.01, 0, -hi]]
    return _one(xyz, [Z] * len(xyz), [[0, 0, 0]], 0.5)


RING_ENTRIES = [(2, 9), (3, 9), (2, 10), (3, 10)]


def ring():
    """(h) 4000 points on the ring x^2 + y^2 = (5/16)^2 at height 3/16 -- the eight mirror images of (3/16, 4/16), 500 times each, whose
    float d2 and dot are the same numbers -- about the origin, axis +z, radius sqrt(2): alpha / bin = 2.5, beta / bin = 1.5 for all"""
    a, b, z = 0.1875, 0.25, 0.1875
    eight = [[sx * u, sy * v, z] for u, v in ((a, b), (b, a)) for sx in (1, -1) for sy in (1, -1)]
    xyz = np.concatenate([[[0, 0, 0]], np.tile(np.asarray(eight), (500, 1))])
    return _one(xyz, [Z] * len(xyz), [[0, 0, 0]], SQRT2)


def long_queue():
    """(i) one keypoint with 20 000 neighbours"""
    rng = np.random.default_rng(51)
    d = rng.normal(size=(20000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.concatenate([[[0, 0, 0]], d * (0.38 * rng.uniform(0.02, 1.0, size=(20000, 1)) ** (1 / 3))]).astype(F)
    n = np.tile(np.asarray([0.6, 0.0, 0.8], F), (len(p), 1))
    return _one(p, n, [[0, 0, 0]], 0.4)


def batch():
    """(k) four objects: a sphere, an empty one, one without keypoints, a noisy plane; keypoints in shuffled order, some off the cloud"""
    rng = np.random.default_rng(61)
    s = _sphere_points(62, 1500)
    e = _sphere_points(63, 1200) * np.asarray([1.0, 0.6, 0.35], F)
    pl = np.concatenate([rng.uniform(-1, 1, size=(1000, 2)), 0.02 * rng.normal(size=(1000, 1))], 1).astype(F)
    pn = np.tile(np.asarray(Z, F), (1000, 1))
    k0 = s[rng.permutation(1500)[:21]]
    k3 = np.concatenate([pl[rng.permutation(1000)[:12]], pl[:3] + F(0.003)])[rng.permutation(15)]
    sizes = [1500, 0, 1200, 1000]
    return dict(pt_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32), xyz=np.concatenate([s, e, pl]).astype(F),
                normals=np.concatenate([s, e / np.linalg.norm(e, axis=1, keepdims=True), pn]).astype(F),
                kp_off=np.array([0, 21, 21, 21, 36], np.uint32), kp=np.concatenate([k0, k3]).astype(F), radius=0.4, w=8)


SCENES = {"sphere": sphere, "hand3": hand3, "off_cloud": off_cloud, "twins": twins, "scaled_axis": scaled_axis, "counts": counts,
          "cylinder": cylinder, "ring": ring, "long_queue": long_queue, "batch": batch,
          "sphere_w1": functools.partial(sphere, 1), "sphere_w25": functools.partial(sphere, 25)}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def answer(name):
    """dict(axes, idx, rows, cnt, deposited, undecided) of the restatement; treat as read-only"""
    s = scene(name)
    axes, idx = ref.batch_normals(s["pt_off"], s["xyz"], s["normals"], s["kp_off"], s["kp"])
    a = ref.spin_images(s["pt_off"], s["xyz"], s["kp_off"], s["kp"], axes, s["radius"], s["w"])
    a.update(axes=axes, idx=idx)
    return a

"""The scenes of the USC tests (tests/test_usc_cpu.py, tests/test_gpu_usc.py), computed once per process. A scene is a ragged batch
dict(pt_off, xyz, kp_off, kp, radius, min_radius, density_radius, frame_radius) and, where the frames are part of the construction,
lrf [nkp, 9] (x, y, z rows): the tests then hand these to ismhip_usc instead of the SHOT frames at frame_radius. 300 to 600 points,
8 to 16 keypoints.

  patch     a curved patch (a cap of a sphere of radius 1 with noise), 12 keypoints that are cloud points; frames computed
  off       the same kind of patch, 10 keypoints: six off the cloud by a few hundredths, one whose R ball holds three points and whose
            frame ball none (NaN frame, ball not empty), one inside the cloud's box with an empty ball, one far outside the grid, one
            not finite
  special   identity frames given: keypoint 0 at the origin with, in its ball, a point exactly on the z axis (u = 0: phi = 0), a point at
            r < r_min, a point equal to the keypoint and two more inside the skip rule (|v|^2 = FLT_EPSILON and below), a point just
            beyond it, and a shell of ordinary points; keypoint 1 the same ball seen in a frame turned by 90 degrees about z; keypoint 2
            with a NaN in its frame; five more on a random blob. 8 keypoints
  ragged    four objects: 300 points packed into a ball of radius 0.05 plus 40 scattered ones (densities from 1 to about 300), an EMPTY
            object with two keypoints, an object of one point, a patch; 3 + 2 + 1 + 6 = 12 keypoints
"""
import functools

import numpy as np

F = np.float32
NAMES = ("patch", "off", "special", "ragged")


def _batch(objects, radius, frame_radius, density_radius=0.1, lrf=None):
    xyz = [np.asarray(p, F).reshape(-1, 3) for p, _ in objects]; kp = [np.asarray(k, F).reshape(-1, 3) for _, k in objects]
    r = float(F(radius))
    return dict(pt_off=np.concatenate([[0], np.cumsum([len(p) for p in xyz])]).astype(np.uint32), xyz=np.concatenate(xyz),
                kp_off=np.concatenate([[0], np.cumsum([len(k) for k in kp])]).astype(np.uint32), kp=np.concatenate(kp),
                radius=r, min_radius=float(F(r / 10.0)), density_radius=float(F(density_radius)), frame_radius=float(F(frame_radius)),
                lrf=None if lrf is None else np.asarray(lrf, F).reshape(-1, 9))


def _cap(rng, n, half_angle=0.6, noise=0.004):
    """n points on the cap of the unit sphere around +z, lifted to the origin's height"""
    u = rng.uniform(np.cos(half_angle), 1.0, n); t = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - u * u)
    p = np.stack([s * np.cos(t), s * np.sin(t), u - 1.0], 1)
    return (p * (1.0 + noise * rng.normal(size=(n, 1)))).astype(F)


def patch():
    rng = np.random.default_rng(2601)
    p = _cap(rng, 500)
    k = p[rng.choice(500, 12, replace=False)]
    return _batch([(p, k)], 0.3, 0.2)


def off():
    rng = np.random.default_rng(2602)
    p = _cap(rng, 397)
    lone = np.array([[2.0, 0.0, 0.0], [2.01, 0.0, 0.0], [2.0, 0.01, 0.0]], F)          # three points far from the cap
    p = np.concatenate([p, lone])
    near = p[rng.choice(397, 6, replace=False)] + rng.uniform(-0.03, 0.03, size=(6, 3)).astype(F)
    k = np.concatenate([near,
                        [[2.0, 0.0, 0.25]],                  # R = 0.3 holds the three lone points, the frame ball (0.2) none of them
                        [[1.3, 0.0, -0.1]],                  # inside the box, nothing within 0.3
                        [[7.0, 7.0, 7.0]],                   # outside the grid
                        [[np.nan, 0.0, 0.0]]]).astype(F)
    return _batch([(p, k)], 0.3, 0.2)


def special():
    rng = np.random.default_rng(2603)
    R = 0.25                                                  # r_min = 0.025
    e = float(np.finfo(F).eps)
    hand = np.array([[0.0, 0.0, 0.125],                       # on the z axis: u = 0, phi = 0, theta = 0
                     [0.0, 0.0, -0.0625],                     # on the axis below: theta = 180, the last elevation bin
                     [0.01, 0.005, 0.002],                    # r < r_min: radial bin 0
                     [0.0, 0.0, 0.0],                         # the keypoint itself: skipped
                     [2.0 ** -12, 2.0 ** -12, 0.0],           # |v|^2 = 2^-23 = FLT_EPSILON: skipped (<=)
                     [2.0 ** -13, 0.0, 0.0],                  # below: skipped
                     [2.0 ** -11, 2.0 ** -12, 2.0 ** -12]], np.float64)   # just beyond: kept, radial bin 0 (off the equator: 90 degrees is an edge)
    assert hand[4, 0] ** 2 * 2 == e
    d = rng.normal(size=(250, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = d * rng.uniform(0.03, 0.24, size=(250, 1))
    blob = np.array([1.5, 0.0, 0.0]) + rng.normal(size=(150, 3)) * 0.08
    p = np.concatenate([hand, shell, blob]).astype(F)
    kb = p[len(hand) + 250 + rng.choice(150, 5, replace=False)]
    k = np.concatenate([[[0, 0, 0], [0, 0, 0], [0, 0, 0]], kb]).astype(F)
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F)
    turned = np.array([0, 1, 0, -1, 0, 0, 0, 0, 1], F)        # x' = y, y' = -x: the azimuth of every point drops by 90 degrees
    bad = ident.copy(); bad[4] = np.nan                        # a NaN in the y axis, which the row never reads: still a NaN row
    # five frames for the blob: random rotations, rounded to float (orthonormal to 1e-7; the definition takes them as they are)
    rot = []
    for _ in range(5):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        rot.append(q.reshape(9))
    lrf = np.stack([ident, turned, bad] + rot).astype(F)
    return _batch([(p, k)], R, 0.15, lrf=lrf)


def ragged():
    rng = np.random.default_rng(2604)
    d = rng.normal(size=(300, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    dense = d * 0.05 * rng.uniform(0, 1, size=(300, 1)) ** (1 / 3)
    sparse = rng.uniform(-0.6, 0.6, size=(40, 3)) + [0.0, 0.0, 0.9]
    a = np.concatenate([dense, sparse]).astype(F)
    ka = np.stack([a[10], a[310], a[320] + F(0.02)])
    empty = np.zeros((0, 3), F)
    ke = np.array([[0, 0, 0], [1, 1, 1]], F)
    one = np.array([[0.5, 0.5, 0.5]], F)
    ko = np.array([[0.5, 0.5, 0.6]], F)
    c = _cap(rng, 200, half_angle=0.5)
    kc = c[rng.choice(200, 6, replace=False)]
    return _batch([(a, ka), (empty, ke), (one, ko), (c, kc)], 0.3, 0.2)


@functools.lru_cache(maxsize=None)
def scene(name):
    s = dict(patch=patch, off=off, special=special, ragged=ragged)[name]()
    n, k = len(s["xyz"]), len(s["kp"])
    assert 300 <= n <= 600 and 8 <= k <= 16, (name, n, k)
    return s

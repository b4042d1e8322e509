"""Scenes of the ISS3D tests (tests/test_iss3d_cpu.py, tests/test_gpu_iss3d.py, tests/test_gpu_iss3d_host.py) and their restatement
answers (tests/iss3d_ref.py), computed once per process and shared.

The bumpy ellipsoid gives a non-trivial number of keypoints: semi-axes 0.5 / 0.35 / 0.25, radial bumps
1 + 0.25 sin(5 u_x) cos(4 u_y) + 0.15 sin(7 u_z) on the unit direction u, Gaussian noise 0.002. A smooth ellipsoid has e2 / e1 close to 1
nearly everywhere and fails the first ratio test; the bumps break that, and the noise keeps exact ties away."""
import functools

import numpy as np

import iss3d_ref as ref

GAMMA, MIN_NEIGHBORS = 0.975, 5
# (points, SalientRadius, NonMaxRadius, seed)
SCENES = ((2048, 0.1, 0.06, 1), (2048, 0.06, 0.04, 2), (700, 0.15, 0.1, 3))
GAMMAS = ((0.975, 0.975), (0.6, 0.5))


def bumpy_ellipsoid(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    bump = 1.0 + 0.25 * np.sin(5.0 * u[:, 0]) * np.cos(4.0 * u[:, 1]) + 0.15 * np.sin(7.0 * u[:, 2])
    p = u * np.array([0.5, 0.35, 0.25]) * bump[:, None] + rng.normal(scale=0.002, size=(n, 3))
    return p.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(k):
    n, _rs, _rn, seed = SCENES[k]
    xyz = bumpy_ellipsoid(n, seed)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def answer(k, gammas=GAMMAS[0]):
    """the restatement on scene k (read only)"""
    _n, rs, rn, _seed = SCENES[k]
    return ref.iss3d(scene(k), rs, rn, gammas[0], gammas[1], MIN_NEIGHBORS)


def plane(n_side=24, step=0.01):
    """an exact z = 0 plane: e3 is exactly 0 at every point, no keypoints"""
    g = np.arange(n_side, dtype=np.float32) * np.float32(step)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(n_side * n_side, np.float32)], 1).astype(np.float32)


def small_cluster():
    """four points: below MinNeighbors 5 whatever the radius"""
    return np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [0, 0, 0.01]], np.float32)


def lattice(n_side=9):
    """dyadic lattice of spacing 1 / 64: with radius 4 / 64 the points at exactly d2 == r2 (offsets (4, 0, 0), ...) are NOT neighbours"""
    g = np.arange(n_side, dtype=np.float32) / np.float32(64)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)


LATTICE_RADIUS = 4.0 / 64.0


def lattice_counts(n_side=9):
    """neighbour counts of lattice(n_side) at LATTICE_RADIUS by integer arithmetic: offsets with dx^2 + dy^2 + dz^2 < 16"""
    idx = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    off = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    off = off[(off * off).sum(1) < 16]
    q = idx[:, None, :] + off[None, :, :]
    return ((q >= 0) & (q < n_side)).all(-1).sum(1)

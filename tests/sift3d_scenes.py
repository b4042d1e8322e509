"""Scenes of the SIFT3D tests (tests/test_sift3d_cpu.py, tests/test_gpu_sift3d.py) and their restatement answers (tests/sift3d_ref.py),
computed once per process and shared.

The surface is the bumpy ellipsoid of the ISS3D scenes; the intensity is a smooth field with a little noise, 0.5 + 0.3 sin(9 x) cos(7 y) +
0.2 sin(11 z) + N(0, 0.02): the smooth part gives extrema at several scales, the noise keeps exact ties away (differences of neighbouring
dog values are around 1e-3, their bounds around 1e-7)."""
import functools

import numpy as np

import sift3d_ref as ref
from iss3d_scenes import bumpy_ellipsoid

NR_SCALES = 3
# (points, base scale, seed)
SCENES = ((2048, 0.04, 11), (1500, 0.03, 12), (700, 0.045, 13))


def field(xyz, seed):
    rng = np.random.default_rng(seed + 100)
    x, y, z = (xyz[:, i].astype(np.float64) for i in range(3))
    return (0.5 + 0.3 * np.sin(9.0 * x) * np.cos(7.0 * y) + 0.2 * np.sin(11.0 * z) + rng.normal(scale=0.02, size=len(xyz))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(k):
    """(xyz float32 [n, 3], intensity float32 [n], scales float32 [NR_SCALES + 3]), read only"""
    n, base, seed = SCENES[k]
    xyz = bumpy_ellipsoid(n, seed)
    inten = field(xyz, seed)
    sc = ref.scales(base, NR_SCALES)
    for a in (xyz, inten, sc):
        a.setflags(write=False)
    return xyz, inten, sc


@functools.lru_cache(maxsize=None)
def answer(k):
    """the restatement on scene k (read only): dog, bound, count, flags, undecided, nn"""
    xyz, inten, sc = scene(k)
    D, B, cnt = ref.dog(xyz, inten, sc)
    flags, und, nn = ref.extrema(xyz, D, B)
    return dict(dog=D, bound=B, count=cnt, flags=flags, undecided=und, nn=nn)


def undecided_share(a):
    inner = a["undecided"][:, 1:-1]
    return float(inner.sum()) / max(inner.size, 1)


def plane_with_bump(sign, n_side=41, step=0.01, s0=None, sc=None):
    """an exact z = 0 lattice with the intensity sign * exp(-r^2 / (2 s0^2)) about its centre point -> (xyz, intensity, centre index)"""
    g = (np.arange(n_side, dtype=np.float64) - n_side // 2) * step
    x, y = np.meshgrid(g, g, indexing="ij")
    xyz = np.stack([x.ravel(), y.ravel(), np.zeros(n_side * n_side)], 1).astype(np.float32)
    r2 = x.ravel() ** 2 + y.ravel() ** 2
    inten = (sign * np.exp(-r2 / (2.0 * s0 * s0))).astype(np.float32)
    return xyz, inten, (n_side // 2) * n_side + n_side // 2


def lattice(n_side=7):
    """dyadic lattice of spacing 1 / 64. With a scale of 1 / 64 the six neighbours at offsets (3, 0, 0), ... lie at exactly d2 == 9 s2 =
    9 / 4096 (every difference, square and sum is exact in float32) and DO count: the rule is d2 <= 9 s2"""
    g = np.arange(n_side, dtype=np.float32) / np.float32(64)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)


LATTICE_SCALE = 1.0 / 64.0


def lattice_counts(n_side=7, reach2=9):
    """neighbour counts of lattice(n_side) for a scale whose bound is reach2 / 4096, by integer arithmetic: offsets with |o|^2 <= reach2"""
    idx = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    r = int(np.ceil(np.sqrt(reach2)))
    off = np.stack(np.meshgrid(*[np.arange(-r, r + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    off = off[(off * off).sum(1) <= reach2]
    q = idx[:, None, :] + off[None, :, :]
    return ((q >= 0) & (q < n_side)).all(-1).sum(1)

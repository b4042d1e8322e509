"""Scenes of the RIFT tests (tests/test_rift_cpu.py, tests/test_gpu_rift.py) and their restatement answers (tests/rift_ref.py), computed
once per process and shared (read only).

The bumpy ellipsoids of iss3d_scenes.py, 700 points at radius 0.15 and 2048 points at radius 0.1, with float32 PCA normals computed here
and oriented away from the centroid, the texture R, G, B = rint(128 + 100 (sin 9x, cos 7y, sin 11z)), and as keypoints every 16th point
plus every 64th point scaled by 0.97, which lies off the surface."""
import functools

import numpy as np

import iss3d_scenes
import rift_ref as ref

# (iss3d scene, points, Radius)
SCENES = ((2, 700, 0.15), (0, 2048, 0.1))
BINS = ((8, 16), (4, 8))
MAX_UNDECIDED_POINTS, MAX_UNDECIDED_KEYPOINTS = 0.01, 0.05


def texture(xyz):
    """packed 0x00RRGGBB as int32"""
    p = np.asarray(xyz, np.float64)
    c = np.rint(128.0 + 100.0 * np.stack([np.sin(9.0 * p[:, 0]), np.cos(7.0 * p[:, 1]), np.sin(11.0 * p[:, 2])], 1)).astype(np.int64)
    assert not len(c) or (c.min() >= 0 and c.max() <= 255)
    return ((c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]).astype(np.int32)


def pca_normals(xyz, radius):
    """float32 unit normals: the eigenvector of the smallest eigenvalue of the ball's covariance, pointing away from the centroid"""
    p = np.asarray(xyz, np.float64)
    nb, _near = ref.balls(np.asarray(xyz, np.float32), np.asarray(xyz, np.float32), radius)
    cen = p.mean(0)
    out = np.zeros((len(p), 3))
    for i, l in enumerate(nb):
        d = p[l] - p[l].mean(0)
        _w, V = np.linalg.eigh(d.T @ d)
        n = V[:, 0]
        out[i] = n if n @ (p[i] - cen) >= 0 else -n
    return out.astype(np.float32)


def keypoints(xyz):
    return np.concatenate([xyz[::16], (xyz[::64].astype(np.float64) * 0.97).astype(np.float32)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(k):
    """-> (xyz, normals, rgba, keypoints, radius)"""
    src, n, radius = SCENES[k]
    xyz = iss3d_scenes.scene(src)
    assert len(xyz) == n
    out = (xyz, pca_normals(xyz, radius), texture(xyz), keypoints(xyz), radius)
    for a in out[:4]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gradient_answer(k):
    xyz, nrm, rgba, _kp, radius = scene(k)
    return ref.gradients(xyz, nrm, rgba, radius)


@functools.lru_cache(maxsize=None)
def row_answer(k, bins=BINS[0]):
    """the restatement end to end: its own gradients, rounded to float32 as the device stores them"""
    xyz, _nrm, _rgba, kp, radius = scene(k)
    ga = gradient_answer(k)
    return ref.rift(xyz, ga["grad"].astype(np.float32), kp, radius, bins[0], bins[1], undecided_points=ga["undecided"])

"""Inputs of the MVBB tests (ismhip_region_mvbb): the smallest clouds at which each part can still go wrong,
seeded, float32. fixture_scenes() are the clouds whose answers by the real libgdiam-1.3 are recorded in tests/golden/mvbb_gdiam.json;
write_fixture_inputs() writes them as raw little-endian doubles for the driver that made that file (the inputs themselves are not
stored: checksum() ties a recorded answer to the bytes it was computed from)."""
import hashlib
import os

import numpy as np

PAIR_TILE = 256                     # mvbb.hip stages 256 column points per tile of its pair search
LDS_SURVIVORS = 768                 # and up to 768 survivors of its pre-filter in LDS (MVBB_LDS_PTS)
WORK_BUFFER_SCENES = ("circle_1000", "ellipsoid_surface")


def rotation(seed):
    """a proper rotation matrix (float64) from a seed"""
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def box_cloud(n, extents, seed, rot=None, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) - 0.5) * np.asarray(extents, dtype=np.float64)
    if rot is not None:
        p = p @ rot.T
    return (p + np.asarray(offset)).astype(np.float32)


def ellipsoid_cloud(n, radii, seed, rot=None, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    p = v * rng.random((n, 1)) ** (1.0 / 3.0) * np.asarray(radii, dtype=np.float64)
    if rot is not None:
        p = p @ rot.T
    return (p + np.asarray(offset)).astype(np.float32)


def fixture_scenes():
    """name -> float32 [n, 3]: random points in rotated boxes and ellipsoids (generic position: unique diameters)"""
    s = {}
    for k, (n, ext) in enumerate([(200, (3.0, 2.0, 1.0)), (500, (1.0, 0.9, 0.8)), (1000, (5.0, 1.0, 0.3)), (1500, (2.0, 2.5, 0.7))]):
        s[f"box{k}"] = box_cloud(n, ext, 100 + k, rotation(200 + k), offset=(0.3 * k, -0.2 * k, 0.1))
    for k, (n, rad) in enumerate([(200, (1.0, 0.6, 0.3)), (500, (2.0, 1.9, 1.8)), (1000, (0.5, 0.1, 0.05)), (1500, (3.0, 1.0, 2.0))]):
        s[f"ellipsoid{k}"] = ellipsoid_cloud(n, rad, 300 + k, rotation(400 + k), offset=(-0.1 * k, 0.5, 0.2 * k))
    return s


# Fixture scenes on which the restatement ends in another box than libgdiam: a SMALLER one. Both follow the same rounds until the box
# has converged; there libgdiam's rectangle (tan / atan2 arithmetic) comes out a few 1e-9 smaller than the box it already holds, it
# takes it, and its axes change places so that the rounds left never visit the third axis again. The restatement's rectangle
# reproduces the held volume to the last bits, keeps its axis order, visits the third axis and improves.
FIXTURE_OTHER_BOX = ("box3", "ellipsoid1")


def as_doubles(points):
    return np.ascontiguousarray(np.asarray(points, dtype=np.float32).astype("<f8"))


def checksum(points):
    return hashlib.sha256(as_doubles(points).tobytes()).hexdigest()


def write_fixture_inputs(directory):
    os.makedirs(directory, exist_ok=True)
    for name, p in fixture_scenes().items():
        as_doubles(p).tofile(os.path.join(directory, name + ".f64"))


KNOWN_BOX_ROT = rotation(7)
KNOWN_BOX_SIZE = (3.0, 2.0, 1.0)


def known_box_corners():
    """the eight corners of a rotated 3 x 2 x 1 box"""
    c = np.array([[sx, sy, sz] for sx in (-0.5, 0.5) for sy in (-0.5, 0.5) for sz in (-0.5, 0.5)]) * np.asarray(KNOWN_BOX_SIZE)
    return (c @ KNOWN_BOX_ROT.T + np.array([0.5, -1.0, 2.0])).astype(np.float32)


def objects():
    """name -> float32 [n, 3], in the order the batch packs them"""
    o = {}
    o["rotated_box"] = box_cloud(400, (3.0, 2.0, 1.0), 1, rotation(3))                  # the axis-aligned box loses at C
    o["aligned_box"] = box_cloud(300, (2.0, 1.0, 0.5), 3)                               # C takes it
    o["one_point"] = np.array([[0.25, -1.5, 3.0]], np.float32)
    o["two_points"] = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, -0.5]], np.float32)
    t = np.linspace(-1.0, 2.0, 50)[:, None]
    o["collinear"] = (t * np.array([[0.6, -0.3, 0.74]]) + np.array([[0.1, 0.2, 0.3]])).astype(np.float32)
    o["coincident"] = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (5, 1))
    rot = rotation(5)
    rng = np.random.default_rng(6)
    flat = np.concatenate([(rng.random((300, 2)) - 0.5) * [2.0, 1.0], np.zeros((300, 1))], axis=1)
    o["planar_patch"] = (flat @ rot.T).astype(np.float32)                               # every volume is (nearly) 0
    a = np.arange(300) * (2.0 * np.pi / 300.0)
    o["circle"] = (np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], axis=1) @ rotation(8).T * 0.8).astype(np.float32)
    # more survivors than the kernel stages in LDS (LDS_SURVIVORS): their lists, the rank sort, the chain and the edge scan run in the
    # work buffer. On the circle every point is a hull vertex; the points ON an ellipsoid crowd the rim of every projection, where the
    # eight-direction pre-filter keeps about a quarter of them, and its box has a volume the restatement can decide
    a = np.arange(1000) * (2.0 * np.pi / 1000.0)
    o["circle_1000"] = (np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], axis=1) @ rotation(14).T * 0.9 + [0.2, -0.1, 0.4]).astype(np.float32)
    v = np.random.default_rng(15).standard_normal((4000, 3))
    o["ellipsoid_surface"] = (v / np.linalg.norm(v, axis=1, keepdims=True) * [1.0, 0.7, 0.4] @ rotation(16).T).astype(np.float32)
    o["two_tiles_37"] = ellipsoid_cloud(2 * PAIR_TILE + 37, (1.0, 0.7, 0.4), 9, rotation(10))
    p = box_cloud(220, (1.0, 2.0, 0.6), 11, rotation(12))
    p[::11] = np.nan                                                                    # 20 points that are not finite
    p[5, 1] = np.inf
    o["with_nan"] = p
    o.update(fixture_scenes())
    rng = np.random.default_rng(13)                                                     # a wide ragged batch of small generic clouds
    for k in range(96):
        n = int(rng.integers(8, 121))
        o[f"ragged{k}"] = ellipsoid_cloud(n, rng.random(3) + 0.2, 500 + k, rotation(600 + k), offset=rng.standard_normal(3))
    return o


def batch():
    """-> dict(names, points [N, 3] float32, pt_off [n_obj + 1] uint32, regions: list of (name, object, centre or None, radius or None))"""
    o = objects()
    names = list(o)
    pts = np.concatenate([o[k] for k in names]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([o[k].shape[0] for k in names])]).astype(np.uint32)
    regions = [(k, i, None, None) for i, k in enumerate(names)]
    rb = names.index("rotated_box")
    regions += [("ball_a", rb, (0.5, 0.2, 0.0), 0.9), ("ball_b", rb, (-0.6, -0.3, 0.1), 0.7),           # two regions on one object
                ("ball_all", rb, (0.0, 0.0, 0.0), 50.0),                                                    # a ball that contains the object
                ("ball_empty", rb, (100.0, 0.0, 0.0), 0.5),
                ("ball_tiles", names.index("two_tiles_37"), (0.1, 0.0, 0.0), 0.6),
                ("ball_nan", names.index("with_nan"), (0.0, 0.0, 0.0), 0.8),
                ("object_below", -1, None, None), ("object_above", len(names), None, None)]
    return dict(names=names, objects=o, points=pts, pt_off=off, regions=regions)


def region_points(b, region):
    """the object's points of a region ([0, 3] for an object index out of range), centre, radius"""
    _, obj, cen, rad = region
    if obj < 0 or obj >= len(b["names"]):
        return np.zeros((0, 3), np.float32), cen, rad
    return b["objects"][b["names"][obj]], cen, rad

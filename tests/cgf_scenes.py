"""The scenes of the CGF tests (tests/test_cgf_cpu.py, tests/test_gpu_cgf.py). A scene is a ragged batch dict(pt_off, xyz, kp_off, kp,
radius, names): every object is one ISLAND with a purpose, named in `names`, so a keypoint's ball is written down point by point.

Scene 0 uses Radius 0.625: rmin = 0.03125, the LRF radius 0.46875 and the normal radius 0.0625 are then exact binary fractions, and
the islands with an identity frame (fewer than 5 points inside the LRF radius) put points exactly ON the bin edges. Scene 1 uses a
Radius with more than six decimals (0.4371234567 -> "0.437123") on generic blobs."""
import functools

import numpy as np

import cgf_ref as ref

F = np.float32
R0 = 0.625
RMIN0 = 0.03125
MAX_UNDECIDED = 0.05                 # share of a scene's keypoints the restatement may leave undecided

# the edge island of scene 0: offsets from the keypoint (0, 0, 0) with an identity frame, and the bins (r, theta, phi) worked out by hand
# (tests/test_cgf_cpu.py derives them). The first point is the nearest one: the skip rule takes it out.
EDGE_POINTS = [
    ((2.0 ** -7, 2.0 ** -7, 2.0 ** -7), None),                       # the nearest point: skipped
    ((RMIN0, 0.0, 0.0), (1, 5, 6)),                                   # r = rmin on +x: theta 90, phi 0
    ((0.0, RMIN0 * (1 - 2.0 ** -23), 0.0), (0, 5, 9)),                # r just below rmin on +y: phi 90
    ((0.0, 0.25, 0.0), (12, 5, 9)),
    ((0.0, 0.0, 0.5), (15, 0, 6)),                                    # theta 0 (phi = atan2(0, 0) = 0)
    ((0.0, 0.0, -0.5), (15, 10, 6)),                                  # theta 180
    ((-0.5, 0.0, 0.0), (15, 5, 11)),                                  # phi +180: y = +0
    ((-0.5, -(2.0 ** -100), 0.0), (15, 5, 0)),                        # phi -180: y below zero by nothing that r or theta can see
    ((R0 * (1 - 2.0 ** -10), 0.0, 0.0), (16, 5, 6)),                  # just inside the ball: the last radial bin
]


def _ball(rng, n, centre, spread):
    v = rng.normal(size=(n, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * (spread * rng.uniform(0.02, 1.0, size=(n, 1)) ** (1 / 3))
    return (v + np.asarray(centre)).astype(F)


def _patch(rng, centre, n=300, n_kp=10):
    """a paraboloid bowl opening towards +z, `n` points inside a disc of radius 0.6, and n_kp keypoints (6 cloud points, 4 next to cloud
    points), each with five more surface points within 0.03 of it so that its 0.0625 ball holds a normal"""
    def surf(xy):
        return np.concatenate([xy, 0.8 * (xy ** 2).sum(1, keepdims=True)], 1)
    rad = 0.6 * np.sqrt(rng.uniform(0, 1, n)); ang = rng.uniform(0, 2 * np.pi, n)
    xy = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    pick = np.flatnonzero(rad < 0.3)[:n_kp]
    extra = np.concatenate([xy[i] + rng.uniform(-0.02, 0.02, size=(5, 2)) for i in pick])
    pts = (surf(np.concatenate([xy, extra])) + np.asarray(centre)).astype(F)
    kp = pts[pick].copy()
    kp[6:] += F(0.004)
    return pts, kp


@functools.lru_cache(maxsize=None)
def scene(k):
    rng = np.random.default_rng(4100 + k)
    objs, names = [], []
    if k == 0:
        o = np.zeros((1, 3), F)
        objs.append((F([[5, 5, 5], [5.1, 5, 5], [5, 5.1, 5]]), o)); names.append("empty ball")
        objs.append((F([[0.25, 0, 0]]), o)); names.append("one point")
        objs.append((F([[0.125, 0, 0], [0, 0.25, 0]]), o)); names.append("two points")
        objs.append((np.asarray([p for p, _ in EDGE_POINTS], np.float64).astype(F), o)); names.append("edges")
        objs.append((F([[0, 0, 0], [1e-8, 0, 0], [0.25, 0.125, 0]]), o)); names.append("coincident")     # d2 = 0 (nearest) and d2 = 1e-16
        objs.append((F([[0.0625, 0, 0], [0.0625, 0, 0], [0, 0.25, 0.125]]), o)); names.append("duplicate nearest")
        for n in (63, 64, 65):
            c = F([0.3, -0.2, 0.5])
            objs.append((_ball(rng, n, c, 0.6), c[None, :])); names.append("ball %d" % n)
        for cz, nm in ((3.0, "patch above the origin"), (-3.0, "patch below the origin")):
            objs.append(_patch(rng, (0.0, 0.0, cz))); names.append(nm)
        radius = R0
    else:
        for _ in range(2):
            centres = rng.uniform(-1.0, 1.0, size=(3, 3))
            p = np.concatenate([centres[b] + s * rng.normal(size=(m, 3)) for b, (m, s) in enumerate(((130, 0.11), (100, 0.22), (70, 0.45)))]).astype(F)
            pick = np.concatenate([rng.choice(130, 5, replace=False), 130 + rng.choice(100, 4, replace=False), 230 + rng.choice(70, 3, replace=False)])
            kp = np.concatenate([p[pick], p[[3, 150]] + F(0.01), p[[250]] + F(0.6), [[7.0, 7.0, 7.0]]]).astype(F)
            objs.append((p, kp[rng.permutation(16)])); names.append("blobs")
        radius = 0.4371234567
    return dict(pt_off=np.cumsum([0] + [len(p) for p, _ in objs]).astype(np.uint32), xyz=np.concatenate([p for p, _ in objs]),
                kp_off=np.cumsum([0] + [len(q) for _, q in objs]).astype(np.uint32), kp=np.concatenate([q for _, q in objs]).astype(F),
                radius=radius, names=names)


N_SCENES = 2


def keypoint_normals(s):
    """the float64 keypoint normals of a scene, object by object -> (normals [nkp, 3], count, gap)"""
    R, _, _ = ref.radii(s["radius"])
    out = [ref.pca_normal(s["xyz"][s["pt_off"][o]:s["pt_off"][o + 1]], s["kp"][s["kp_off"][o]:s["kp_off"][o + 1]], 0.1 * R)
           for o in range(len(s["pt_off"]) - 1)]
    return tuple(np.concatenate([t[i] for t in out]) for i in range(3))


def answer(s, lrf, normals):
    """the restatement's rows of a scene given float32 frames [nkp, 9] and keypoint normals [nkp, 3] -> dict(rows, counts, sum,
    undecided, ball, kind, skipped (object-local))"""
    parts = []
    for o in range(len(s["pt_off"]) - 1):
        a, b = s["kp_off"][o], s["kp_off"][o + 1]
        parts.append(ref.raw(s["xyz"][s["pt_off"][o]:s["pt_off"][o + 1]], s["kp"][a:b], lrf[a:b], normals[a:b], s["radius"]))
    out = {key: np.concatenate([p[key] for p in parts]) for key in ("rows", "counts", "sum", "undecided", "ball", "skipped")}
    out["kind"] = sum((p["kind"] for p in parts), [])
    return out


def object_of(s, name):
    """(first keypoint, one past the last) of the first object called `name`"""
    o = s["names"].index(name)
    return int(s["kp_off"][o]), int(s["kp_off"][o + 1])


MLP_NNZ = 8                          # non-zero weights per output of the sparse nets below


def random_layers(rng, widths, nnz=0):
    """seeded weights of both signs, b ~ N(0, 0.1^2), ReLU on every layer but the last. nnz = 0: dense, W ~ N(0, 1 / in). nnz > 0: every
    output reads nnz random inputs with weights ~ N(0, 1 / nnz) and zeros elsewhere.

    Why both. The bound of cgf_ref.mlp is a worst case over signs and summation orders: a layer multiplies the incoming error by the
    column sums of |W|, about 0.8 sqrt(in) = 18 for a dense 512-wide layer and 0.8 sqrt(nnz) = 2.3 for a sparse one, while the values
    themselves pass at about 0.7. Through the real shape 2244 -> 512^4 -> 40 the dense bound ends far above the outputs (it holds, and says
    little); the sparse one ends near 1 % of what the outputs owe to the input, so a wrong element anywhere shows."""
    layers = []
    for i, (n_in, n_out) in enumerate(zip(widths[:-1], widths[1:])):
        if nnz and nnz < n_in:
            W = np.zeros((n_in, n_out), F)
            for j in range(n_out):
                W[rng.choice(n_in, nnz, replace=False), j] = rng.normal(size=nnz) / np.sqrt(nnz)
        else:
            W = (rng.normal(size=(n_in, n_out)) / np.sqrt(n_in)).astype(F)
        b = (0.1 * rng.normal(size=n_out)).astype(F)
        layers.append((W, b, i + 2 < len(widths)))
    return layers

"""Seeded scenes for the SHOTNA reference frame, built from the pieces of frontend_scenes.py (numpy only). test_shotna_cpu.py proves on
the host, with the restatement shotna_ref.py, that each scene reaches the branch it is named for; test_gpu_shotna.py runs the kernels on
the same bytes. Restatement results are computed once per scene and shared."""
import numpy as np

import frontend_scenes as fs
import shotna_ref as ref

f32 = np.float32
_cache = {}


class Scene:
    def __init__(self, name, objs, kps, radius, cell):
        self.name, self.objs, self.kps, self.radius, self.cell = name, objs, kps, radius, cell

    def soa(self):
        return fs.soa(self.objs, self.kps)

    def reference(self, normal_votes=True, normals=None):
        """the restatement's frames of this scene (cached unless other normals are supplied)"""
        pt_off, p, n, kp_off, kp = self.soa()
        if normals is not None:
            return ref.frames(pt_off, p, np.asarray(normals, f32), kp_off, kp, self.radius, normal_votes)
        key = (self.name, normal_votes)
        if key not in _cache:
            _cache[key] = ref.frames(pt_off, p, n, kp_off, kp, self.radius, normal_votes)
        return _cache[key]


# ---------------------------------------------------------------------------------------------- generic: a convex surface
GENERIC_RADIUS = 0.3
GENERIC_CELL = 0.12


def generic(negated=False, shift=(0.0, 0.0, 0.0)):
    """3000-point ellipsoid with outward normals, 64 keypoints at 0.98 of a surface point (inside the surface: the position rule turns
    z inward, the normal rule outward), the first one exactly ON a surface point"""
    rng = np.random.default_rng(71)
    p, n = fs.ellipsoid(rng, 3000)
    kp = (p[rng.choice(3000, 64, replace=False)] * f32(0.98)).astype(f32)
    kp[0] = p[7]
    sh = np.asarray(shift, f32)
    name = "generic" + ("-negated" if negated else "") + ("" if not sh.any() else "-shifted")
    return Scene(name, [((p + sh).astype(f32), -n if negated else n)], [(kp + sh).astype(f32)], GENERIC_RADIUS, GENERIC_CELL)


# ---------------------------------------------------------------------------------------------- ragged batch of 11 objects
RAGGED_RADIUS = 0.3
RAGGED_CELL = 0.12
RAGGED_NAN_BALL = (1, 0)           # (object, keypoint): the ball that holds three NaN normals


def ragged():
    """11 objects (>= 8 and no multiple of 8: the XCD block map deals a full and a partial group): spheres and planes of 500 to 3000
    points, an EMPTY object with a keypoint, a 4-point object, a keypoint 30 units away, a NaN keypoint, an object with every 97th
    point NaN, three NaN normals inside one ball"""
    rng = np.random.default_rng(72)

    def sphere(n, scale, shift, noise=0.01):
        d = fs._unit(rng.normal(size=(n, 3)))
        return ((d * (1 + noise * rng.normal(size=(n, 1)))) * scale + shift).astype(f32), d.astype(f32)

    def plane(n, noise=0.02):
        p = np.concatenate([rng.uniform(-1, 1, size=(n, 2)), noise * rng.normal(size=(n, 1))], axis=1)
        up = fs._unit(np.array([[0.0, 0.0, 1.0]]) + 0.2 * rng.normal(size=(n, 3)))
        return p.astype(f32), up.astype(f32)

    e_p, e_n = fs.ellipsoid(rng, 2500)
    e_p[::97] = np.nan
    objs = [sphere(3000, 1.0, 0.0), sphere(2000, 0.8, [2.0, 1.0, -1.0]), (np.zeros((0, 3), f32), np.zeros((0, 3), f32)), plane(2000),
            sphere(4, 1.0, 0.0, 0.0), (e_p, e_n), plane(700), sphere(500, 0.3, [3.0, -2.0, 1.0]), sphere(1500, 0.8, [-40.0, 25.0, 60.0]),
            plane(1200), sphere(1000, 0.6, [0.0, 5.0, 0.0])]
    n_kp = [12, 9, 1, 7, 4, 11, 5, 3, 10, 6, 8]
    kps = []
    for o, (p, _) in enumerate(objs):
        if len(p) == 0:
            kps.append(f32([[0.1, 0.2, 0.3]]))
            continue
        ok = np.isfinite(p).all(1)
        sel = p[ok][rng.choice(ok.sum(), min(n_kp[o], ok.sum()), replace=False)]
        c = p[ok].astype(np.float64).mean(0)
        k = (c + (sel.astype(np.float64) - c) * 0.98).astype(f32)
        k[0] = sel[0]                                                       # the first one sits on a surface point
        if o == 0:
            k[-2] = [30.0, 0, 0]; k[-1] = [np.nan, 0, 0]
        kps.append(k)
    o, j = RAGGED_NAN_BALL
    p, n = objs[o]
    near = np.argsort(((p.astype(np.float64) - kps[o][j]) ** 2).sum(1))[3:6]   # three neighbours well inside the ball
    n = n.copy(); n[near[0]] = np.nan; n[near[1], 1] = np.nan; n[near[2], 2] = np.nan
    objs[o] = (p, n)
    return Scene("ragged", objs, kps, RAGGED_RADIUS, RAGGED_CELL)


# ---------------------------------------------------------------------------------------------- mirror clouds: counts exact to a vote
MIRROR_M = [400, 641, 4097]        # 800 / 1282 / 8194 neighbours: register, LDS and global-scratch key paths of k_lrf_tie
MIRROR_SETS = ["one-way", "mirrored", "half", "half-minus", "half-plus"]
MIRROR_U = np.array([0.1, 0.2, 0.97]) / np.linalg.norm([0.1, 0.2, 0.97])


def mirror(m, kind):
    """fs.mirror_cloud(m) with the keypoint at the origin (every x sum is exactly 0) and one of five normal sets: all along u (z by
    the normals, x by the medians) | n_i on p_i and -n_i on -p_i (plusN == 0) | +-u, a random half each (plusN == 0) | that set with
    one more -u (plusN == -2) | with one more +u (plusN == +2); the signs are meant relative to u, the frame's z ends along +-u"""
    pts = fs.mirror_cloud(m)
    rng = np.random.default_rng(73 + m)
    if kind == "one-way":
        n = np.tile(MIRROR_U, (2 * m, 1))
    elif kind == "mirrored":
        h = fs._unit(rng.normal(size=(m, 3)))
        n = np.concatenate([h, -h])
    else:
        sgn = np.ones(2 * m); sgn[rng.permutation(2 * m)[:m]] = -1
        if kind == "half-minus":
            sgn[np.nonzero(sgn > 0)[0][0]] = -1
        elif kind == "half-plus":
            sgn[np.nonzero(sgn < 0)[0][0]] = 1
        n = sgn[:, None] * MIRROR_U[None, :]
    return Scene(f"mirror-{m}-{kind}", [(pts, n.astype(f32))], [np.zeros((1, 3), f32)], fs.MIRROR_RADIUS, fs.MIRROR_CELL)


# ---------------------------------------------------------------------------------------------- dense object: several windows
DENSE_DEALS = {"tie": 0, "plus": 2, "minus": -2}


def dense(deal=None):
    """fs.dense_object(FUSED_SURFACE) at DENSE_RADIUS: 40 keypoints, balls of thousands of neighbours, single cell rows longer than a
    candidate window. deal = None: its own normals. Otherwise the normals of every point in the FIRST keypoint's ball are +-u, u the
    coordinate axis nearest that keypoint's v3 (|u . v3| >= 0.57), dealt at random so that the first keypoint's plusN is 0 / +2 / -2
    relative to u."""
    pts, nrm, kp = fs.dense_object(fs.FUSED_SURFACE)
    if deal is not None:
        base = Scene("dense", [(pts, nrm)], [kp], fs.DENSE_RADIUS, fs.DENSE_CELL).reference()
        v3 = base["frame"][0, 6:9].astype(np.float64)
        u = np.zeros(3); u[np.argmax(np.abs(v3))] = 1.0
        d = (pts - kp[0][None, :]).astype(f32)
        d2 = ((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32)
        d2 = (d2 + (d[:, 2] * d[:, 2]).astype(f32)).astype(f32)
        ball = np.nonzero(d2 < f32(np.float64(f32(fs.DENSE_RADIUS)) ** 2))[0]
        nb = len(ball)
        assert nb % 2 == 0 and not (pts[ball] == kp[0]).all(1).any()          # valid == in_ball and even: a tie can be dealt
        n_pos = (nb + DENSE_DEALS[deal]) // 2
        sgn = -np.ones(nb); sgn[np.random.default_rng(74).permutation(nb)[:n_pos]] = 1
        nrm = nrm.copy(); nrm[ball] = (sgn[:, None] * u[None, :]).astype(f32)
    return Scene("dense" + ("" if deal is None else "-" + deal), [(pts, nrm)], [kp], fs.DENSE_RADIUS, fs.DENSE_CELL)


_scenes = {}


def get(builder, *args):
    """scenes are built once"""
    key = (builder.__name__,) + args
    if key not in _scenes:
        _scenes[key] = builder(*args)
    return _scenes[key]


def gpu_scenes():
    """every scene test_gpu_shotna.py runs (the one with device-estimated normals is checked against its own normals there)"""
    out = [get(generic, False), get(generic, True), get(ragged)]
    out += [get(mirror, m, kind) for m in MIRROR_M for kind in MIRROR_SETS]
    out += [get(dense, None)] + [get(dense, d) for d in DENSE_DEALS]
    return out

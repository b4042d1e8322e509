"""Scenes for ismhip_global_cvfh: small ragged batches (100 to 700 points per object) with whole-object regions, ball regions, two regions
on one object and an empty region. A case: dict(name, objs [(points, normals)], regions [(object, centre or None, radius or None)],
cell, params dict(cluster_tolerance, normal_radius, min_points), max_rows, exact). The EXACT cases are built so that the restatement
cvfh_ref.py finds no undecided link (test_cvfh_cpu.py checks it): lattices whose distances stay far from the tolerance, angles of 0, 6,
14 and 90 degrees against the threshold of 10. Every object sits near z = 2: the viewpoint (0, 0, 0) sees it from outside."""
import numpy as np

import cvfh_ref as cr

f32 = np.float32
H = 1.0 / 16.0                       # lattice spacing: exact in float32, as are its squared distances
TOL = 0.1                            # links at H and H * sqrt(2) (0.088), not at 2 H
MIN_POINTS = 30
DOWN = f32([0, 0, -1])               # towards the viewpoint


def lattice(nx, ny, origin=(0.0, 0.0, 2.0), skip=()):
    """an nx x ny lattice in the plane z = origin.z, x fastest, normals DOWN; skip: lattice indices left out"""
    ij = [(i, j) for j in range(ny) for i in range(nx)]
    p = f32([[origin[0] + i * H, origin[1] + j * H, origin[2]] for k, (i, j) in enumerate(ij) if k not in skip])
    return p, np.tile(DOWN, (len(p), 1))


def join(*parts):
    return np.concatenate([p for p, _ in parts]).astype(f32), np.concatenate([n for _, n in parts]).astype(f32)


def turned(obj, angle=0.37, axis=(1.0, 2.0, 3.0), pivot=(0.0, 0.0, 2.0)):
    """the object turned about an axis through pivot by a generic angle: distances and angles stay, the lattice directions leave the
    coordinate axes, and with them the descriptor's deposits leave the bin edges that an axis-aligned lattice sits on"""
    p, n = obj
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    return f32((p.astype(np.float64) - pivot) @ R.T + pivot), f32(n.astype(np.float64) @ R.T)


def shuffled(obj, seed):
    p, n = obj
    order = np.random.default_rng(seed).permutation(len(p))
    return p[order], n[order]


def hand_case():
    plane = lattice(12, 10)                                                       # 120 points: one cluster
    two = join(lattice(8, 8), lattice(8, 8, (8 * H + 0.25, 0.0, 2.0)))            # 64 + 64, a gap of 0.25 + H: two clusters
    sizes = join(lattice(6, 5), lattice(6, 5, (1.0, 0.0, 2.0), skip=(29,)),       # 30 kept, 29 dropped
                 lattice(10, 5, (2.0, 0.0, 2.0)))                                 # filler: 50, kept
    sparse_p, sparse_n = lattice(5, 5)                                            # no kept cluster: the fallback row
    sparse_p = (sparse_p * f32([4, 4, 1])).astype(f32)                            # spacing 0.25 > TOL: no links at all
    sparse_n = sparse_n.copy(); sparse_n[3] = np.nan; sparse_n[17] = np.nan
    sparse = join((sparse_p, sparse_n), lattice(5, 5, (3.0, 0.0, 2.0)), lattice(5, 4, (3.0, 1.0, 2.0)), lattice(5, 5, (3.0, 2.0, 2.0)),
                  lattice(5, 5, (3.0, 3.0, 2.0)))                                 # 25 sparse + 25 + 20 + 25 + 25: every component below 30
    objs = [plane, shuffled(two, 1), sizes, sparse]
    regions = [(0, None, None), (1, None, None), (2, None, None), (3, None, None),
               (1, (3.5 * H, 3.5 * H, 2.0), 0.4),                                 # the first patch of `two` only: second region on object 1
               (0, (0.0, 0.0, 2.0), 0.33),                                        # a quarter disc of the plane: 5.28 H
               (0, (9.0, 9.0, 9.0), 0.5),                                         # empty
               (2, (2.0 + 2 * H, 2 * H, 2.0), 0.2)]                               # 3.2 H round a lattice point: fewer than 30 points: fallback
    return dict(name="hand", objs=objs, regions=regions, cell=0.2, max_rows=4, exact=True,
                params=dict(cluster_tolerance=TOL, normal_radius=0.0, min_points=MIN_POINTS))


def cylinder(radius, step_deg, n_angles, n_axial, dz=0.05, lengths=None):
    """lattice on a cylinder round the y axis through (0, 0, 2): angle index major; lengths[a]: axial points of line a"""
    p, n = [], []
    for a in range(n_angles):
        t = np.deg2rad(step_deg * a)
        for k in range(n_axial if lengths is None else lengths[a]):
            y = k * dz + 0.004 * np.sin(1.7 * k + a)               # uneven steps of 0.042 .. 0.058: off the distance block's bin edges
            p.append([radius * np.sin(t), y, 2.0 - radius * np.cos(t)])
            n.append([np.sin(t), 0.0, -np.cos(t)])
    return f32(p), f32(n)


CYL14_LENGTHS = [32, 20, 32, 31, 30, 32, 8, 32, 29, 32]


def curved_case():
    """cylinder lattices: 6 degree steps chain into ONE cluster across 306 degrees; at 14 degree steps only axial neighbours link"""
    cyl6 = cylinder(0.5, 6.0, 52, 6)                                              # chord 0.0523, diagonal 0.0724 < 0.08 < 2 chords
    cyl14 = shuffled(cylinder(0.25, 14.0, 10, 0, lengths=CYL14_LENGTHS), 2)       # chord 0.0609 < 0.08, but 14 degrees
    filler = lattice(12, 10)
    return dict(name="cylinders", objs=[cyl6, cyl14, filler], regions=[(0, None, None), (1, None, None), (2, None, None), (1, (0.0, 0.4, 2.0), 0.45)],
                cell=0.15, max_rows=8, exact=True, params=dict(cluster_tolerance=0.08, normal_radius=-1.0, min_points=MIN_POINTS))


def crease_objs():
    """two lattice planes meeting at a right angle along x = 0.5: z = 2 (normal DOWN) and x = 0.5 rising towards the viewer's side"""
    floor = lattice(9, 8)                                                         # x = 0 .. 0.5
    wall_p = f32([[0.5 + 0.3 * H, j * H, 2.0 - 1.19 * k * H] for j in range(8) for k in range(1, 9)])   # off the floor's lattice: no |dx| = |dz| ties, no floor point in the wall's plane
    wall = (wall_p, np.tile(f32([-1, 0, 0]), (len(wall_p), 1)))
    return [shuffled(turned(join(floor, wall)), 3), lattice(12, 10), turned(lattice(10, 11, (0.3, 0.2, 2.5)), 0.21, (3.0, 1.0, 2.0))]


def crease_case(estimated):
    return dict(name="crease-estimated" if estimated else "crease", objs=crease_objs(), regions=[(0, None, None), (1, None, None), (2, None, None)],
                cell=0.2, max_rows=4, exact=True,
                params=dict(cluster_tolerance=TOL, normal_radius=0.11 if estimated else 0.0, min_points=MIN_POINTS))


def many_case():
    """more kept clusters than max_rows = 4: six, five and (exactly the capacity) four patches"""
    def patches(k):
        return join(*[lattice(6, 5, (0.6 * i, 0.0, 2.0)) for i in range(k)])
    return dict(name="many", objs=[shuffled(patches(6), 4), patches(5), patches(4)], regions=[(0, None, None), (1, None, None), (2, None, None)],
                cell=0.25, max_rows=4, exact=True, params=dict(cluster_tolerance=TOL, normal_radius=0.0, min_points=MIN_POINTS))


def random_case():
    """a seeded curved surface z = 2 + 0.15 sin(3x) cos(2y) with analytic normals, a noisy sphere cap and a flat jittered patch; the
    clustering normals are re-estimated. Not exact: links may be undecided."""
    rng = np.random.default_rng(20)
    def surface(k, f):
        xy = rng.random((k, 2)) * 1.2
        z, gx, gy = f(xy[:, 0], xy[:, 1])
        n = np.stack([gx, gy, -np.ones(k)], 1)
        return f32(np.column_stack([xy, z])), f32(n / np.linalg.norm(n, axis=1, keepdims=True))
    wave = surface(600, lambda x, y: (2 + 0.15 * np.sin(3 * x) * np.cos(2 * y), 0.45 * np.cos(3 * x) * np.cos(2 * y), -0.3 * np.sin(3 * x) * np.sin(2 * y)))
    flat = surface(300, lambda x, y: (2 + 0 * x, 0 * x, 0 * x))
    u = rng.normal(size=(400, 3)); u[:, 2] = -np.abs(u[:, 2]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    cap = (f32(u * 0.6 + [0, 0, 2.2]), f32(u))
    return dict(name="random", objs=[wave, cap, flat], regions=[(0, None, None), (1, None, None), (2, None, None), (0, (0.6, 0.6, 2.0), 0.45)],
                cell=0.2, max_rows=8, exact=False, params=dict(cluster_tolerance=0.09, normal_radius=0.14, min_points=20))


def all_cases():
    return [hand_case(), curved_case(), crease_case(False), crease_case(True), many_case(), random_case()]


_refs = {}


def reference(case):
    """cvfh_ref.region of every region of a case, once"""
    if case["name"] not in _refs:
        pr = case["params"]
        _refs[case["name"]] = [cr.region(case["objs"][o][0], case["objs"][o][1], c, r, pr["cluster_tolerance"], pr["normal_radius"], pr["min_points"])
                               for o, c, r in case["regions"]]
    return _refs[case["name"]]

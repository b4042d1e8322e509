"""Seeded scenes for the VFH region descriptor, numpy only: the smallest shapes at which the one-workgroup-per-region kernel can go
wrong. A case is a dict as in global_scenes.py:
  objs     list of (points [n, 3], normals [n, 3]) float32, one per object (non-finite points and normals allowed)
  regions  list of (object, centre xyz or None, radius or None); None / None = the whole object
  cell     the grid cell of the cloud (the region kernel does not use the grid; the cloud needs one)"""
import numpy as np

import global_ref as gr

f32 = np.float32
BALL_SIZES = [0, 1, 2, 5, 63, 64, 65, 257, 4099]
BALL_CENTRE = (0.15, 0.0, 0.05)
N_SURFACE = 16384
BIG_N = 70000                     # above GRID_FUSED_MAX_PTS (65 536)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def blob(rng, n, scale=(1.0, 0.6, 0.35), shift=(0.0, 0.0, 0.0), bias=(0.0, 0.0, 0.6)):
    """n points of a skewed anisotropic blob; unit normals scattered round `bias`, so that the normal centroid is clear of zero"""
    p = rng.normal(size=(n, 3))
    p[:, 0] = rng.exponential(size=n)
    p[:, 2] = 0.5 * rng.exponential(size=n) + 0.3 * p[:, 2]
    p = p * np.asarray(scale) * 0.2 + np.asarray(shift)
    return p.astype(f32), _unit(rng.normal(size=(max(n, 1), 3)) + np.asarray(bias))[:n].astype(f32)


def ball_radius(p, centre, count):
    """a selection radius that the rule d2 < (float)((double)r * r) gives exactly `count` points of p round `centre`: halfway (in d)
    between the count-th and the next distance"""
    d2, _ = gr._sqdist(p, centre)
    d = np.sort(np.sqrt(d2.astype(np.float64)))
    if count == 0:
        return float(d[0]) * 0.5
    r = 0.5 * (d[count - 1] + d[count])
    assert int((d2 < gr.r2_of(r)).sum()) == count
    return float(r)


def balls_case(seed=201):
    """one blob of 6 000 points cut by ball regions of exactly BALL_SIZES selected points"""
    rng = np.random.default_rng(seed)
    p, n = blob(rng, 6000)
    regions = [(0, BALL_CENTRE, ball_radius(p, BALL_CENTRE, k)) for k in BALL_SIZES]
    return dict(name="balls", objs=[(p, n)], regions=regions, cell=0.1)


def ellipsoid_case(seed=202):
    """a closed ellipsoid with outward normals, unevenly sampled: the normal centroid is small but not zero"""
    rng = np.random.default_rng(seed)
    u = _unit(rng.normal(size=(N_SURFACE, 3)) + [0.15, 0.0, 0.05])
    ax = np.array([0.5, 0.3, 0.2])
    return dict(name="ellipsoid", objs=[((u * ax).astype(f32), _unit(u / ax).astype(f32))], regions=[(0, None, None)], cell=0.1)


def half_shell_case(seed=203):
    """the partial view: the half of a sphere of radius 0.4 round (0, 0, 2) that faces the origin, normals outward (towards the sensor)"""
    rng = np.random.default_rng(seed)
    u = _unit(rng.normal(size=(N_SURFACE, 3)))
    u[:, 2] = -np.abs(u[:, 2])
    return dict(name="half_shell", objs=[((u * 0.4 + [0.0, 0.0, 2.0]).astype(f32), u.astype(f32))], regions=[(0, None, None)], cell=0.1)


def big_case(seed=204):
    rng = np.random.default_rng(seed)
    return dict(name="big", objs=[blob(rng, BIG_N)], regions=[(0, None, None), (0, (0.2, 0.0, 0.1), 0.25)], cell=0.1)


def mixed_case(seed=205):
    """three objects with non-finite points and non-finite normals; regions in reverse object order; one region whose object index is
    out of range; one that selects nothing"""
    rng = np.random.default_rng(seed)
    a, an = blob(rng, 700)
    b, bn = blob(rng, 3000, shift=(2.0, -1.0, 0.5))
    c, cn = blob(rng, 150, shift=(-3.0, 0.0, 0.0))
    a[0, 0], a[17, 1], a[699, 2] = np.nan, np.inf, -np.inf
    b[5, 2], b[1500, 0] = np.nan, np.nan
    c[149, 1] = np.nan
    an[3, 0], an[40, 2], an[41] = np.nan, np.inf, np.nan
    bn[7, 1], bn[2999, 0] = -np.inf, np.nan
    cn[::3] = np.nan                                           # a third of object 2's normals
    regions = [(2, None, None), (1, (2.1, -1.0, 0.55), 0.12), (7, None, None), (1, None, None), (0, None, None),
               (0, (50.0, 50.0, 50.0), 0.3), (2, (-3.0, 0.0, 0.0), 0.5)]
    return dict(name="mixed", objs=[(a, an), (b, bn), (c, cn)], regions=regions, cell=0.1)


def plane_case(seed=206):
    """a tilted planar patch round (0, 0, 1.5) with identical normals (0.6, 0, -0.8), perpendicular to it: every viewpoint deposit lands
    in ONE bin (n . d = 0.8: raw 115.2). nc equals the normal bit for bit, so the two cosines of every pair are the same float: an exact
    tie of the role swap, in which both assignments give f1 = 0, f2 = 0 and f3 = 0 up to rounding noise -- raw 22.5, the middle of bin
    22 of each block: the same-address case for three of the four shape blocks as well"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-0.3, 0.3, size=(4000, 2)) * [1.0, 0.6]
    p = np.stack([xy[:, 0], xy[:, 1], 1.5 + 0.75 * xy[:, 0]], 1)           # the plane 0.6 x - 0.8 (z - 1.5) = 0
    n = np.broadcast_to(f32([0.6, 0.0, -0.8]), (4000, 3)).copy()
    return dict(name="plane", objs=[(p.astype(f32), n)], regions=[(0, None, None)], cell=0.1)


def centred_case(seed=207):
    """{p, -p} on a dyadic lattice plus the origin itself: the float centroid is exactly (0, 0, 0), the centre point's pair is rejected
    (f4 == 0) and its viewpoint deposit still counts; the normals are scattered round (0.3, 0.2, 0.5), so nc != 0"""
    rng = np.random.default_rng(seed)
    base = np.round(rng.normal(size=(1500, 3)) * [0.3, 0.18, 0.1] * 65536.0) / 65536.0
    base = base[(base != 0).any(1)]
    p = np.concatenate([base, -base, np.zeros((1, 3))]).astype(f32)
    n = _unit(rng.normal(size=(len(p), 3)) + [0.3, 0.2, 0.5]).astype(f32)
    return dict(name="centred", objs=[(p, n)], regions=[(0, None, None)], cell=0.5)


def all_cases():
    return [balls_case(), ellipsoid_case(), half_shell_case(), big_case(), mixed_case(), plane_case(), centred_case()]


def finite_points(case, o):
    if not 0 <= o < len(case["objs"]):
        return np.zeros((0, 3), f32), np.zeros((0, 3), f32)
    p, n = case["objs"][o]
    ok = np.isfinite(p).all(1)
    return p[ok], n[ok]


def selected(case, region):
    """(points, normals) the region selects, by the restatement's rule"""
    o, centre, radius = region
    p, n = finite_points(case, o)
    if radius is None or len(p) == 0:
        return p, n
    d2, _ = gr._sqdist(p, centre)
    keep = d2 < gr.r2_of(radius)
    return p[keep], n[keep]

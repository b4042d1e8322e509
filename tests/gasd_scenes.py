"""Seeded scenes for the GASD region descriptor, numpy only: the smallest shapes at which the one-workgroup-per-region kernel can go
wrong. A case is a dict as in vfh_scenes.py with colours:
  objs     list of (points [n, 3], normals [n, 3]) float32, one per object (non-finite points and normals allowed)
  rgba     list of packed colours 0x00RRGGBB [n] uint32, one per object
  regions  list of (object, centre xyz or None, radius or None); None / None = the whole object
  cell     the grid cell of the cloud (the region kernel does not use the grid; the cloud needs one)"""
import itertools

import numpy as np

import global_ref as gr
import vfh_scenes as vs

f32 = np.float32
BALL_SIZES = vs.BALL_SIZES            # 0, 1, 2, 5, 63, 64, 65, 257, 4099 selected points
N_SKEWED = 16384
BIG_N = vs.BIG_N                      # 70 000: above GRID_FUSED_MAX_PTS (65 536)
TIE_POINTS = f32([[3, 0, 0], [-3, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 1], [0, 0, -1]])
TIE_COLOURS = np.array([0xff0000, 0x00ff00, 0x0000ff, 0x808080, 0xff8000, 0x00ffff], np.uint32)
COINCIDENT = f32([5.0, 5.0, 5.0])
# the hues 0, 30, .. 330 at chroma 254 (127 / 254 = 1 / 2 exactly): each sits on the face between two of the 12 hue bins
HUES_30 = [(254, 0, 0), (254, 127, 0), (254, 254, 0), (127, 254, 0), (0, 254, 0), (0, 254, 127), (0, 254, 254), (0, 127, 254), (0, 0, 254),
           (127, 0, 254), (254, 0, 254), (254, 0, 127)]


def colours(rng, n):
    return rng.integers(0, 1 << 24, size=n).astype(np.uint32)


def _case(name, objs, regions, cell, rng, rgba=None):
    return dict(name=name, objs=objs, rgba=rgba if rgba is not None else [colours(rng, len(o[0])) for o in objs], regions=regions, cell=cell)


def balls_case(seed=301):
    """the blob of vfh_scenes.py (6 000 points) cut by ball regions of exactly BALL_SIZES selected points"""
    c = vs.balls_case()
    return _case("balls", c["objs"], c["regions"], c["cell"], np.random.default_rng(seed))


def skewed_case(seed=302):
    """a whole-object skewed blob: exponential along its longest axis, so clearly more points on one side of the centroid than on the other"""
    rng = np.random.default_rng(seed)
    return _case("skewed", [vs.blob(rng, N_SKEWED)], [(0, None, None)], 0.1, rng)


def big_case(seed=303):
    rng = np.random.default_rng(seed)
    return _case("big", [vs.blob(rng, BIG_N)], [(0, None, None), (0, (0.2, 0.0, 0.1), 0.25)], 0.1, rng)


def mixed_case(seed=304):
    """the three objects of vfh_scenes.mixed_case with non-finite points and normals, an object index out of range, an empty ball"""
    c = vs.mixed_case()
    return _case("mixed", c["objs"], c["regions"], c["cell"], np.random.default_rng(seed))


def facing_case(seed=305):
    """object 0: a flat skewed blob above the origin; object 1: the same points mirrored in z (z -> -z). Whatever sign the solver gives
    the smallest-eigenvalue axis, it faces the view direction (0, 0, 1) in exactly one of the two and is negated there: with M =
    diag(1, 1, -1) the frames are related by x' = M x, y' = M y, z' = -M z"""
    rng = np.random.default_rng(seed)
    p, n = vs.blob(rng, 3000, scale=(1.0, 0.6, 0.12), shift=(0.1, -0.2, 1.0))
    m = f32([1, 1, -1])
    rgba = colours(rng, len(p))
    return _case("facing", [(p, n), ((p * m).astype(f32), (n * m).astype(f32))], [(0, None, None), (1, None, None)], 0.1, rng, [rgba, rgba.copy()])


def ties_case(seed=306):
    """six points on the axes: the covariance is diag(18, 8, 2) exactly, the axes exact, one point on either side of x: a sign tie"""
    n = np.tile(f32([0, 0, 1]), (6, 1))
    return _case("ties", [(TIE_POINTS.copy(), n)], [(0, None, None)], 1.0, np.random.default_rng(seed), [TIE_COLOURS.copy()])


def plane_case(seed=307):
    """a tilted planar patch through its own centroid: t.z is rounding noise round 0, the face between z cells 2 and 3 (1 and 2 of the
    colour grid): z is undecided for (nearly) every deposit, and every point lands in one of two z layers: the same-address case"""
    c = vs.plane_case()
    return _case("plane", c["objs"], c["regions"], c["cell"], np.random.default_rng(seed))


def coincident_case(seed=308):
    """a blob, and far from it two equal points that a ball region selects alone: zero covariance, max_coord = 0, a NaN row"""
    rng = np.random.default_rng(seed)
    p, n = vs.blob(rng, 500)
    p = np.concatenate([p, COINCIDENT[None, :], COINCIDENT[None, :]]).astype(f32)
    n = np.concatenate([n, n[:2]]).astype(f32)
    return _case("coincident", [(p, n)], [(0, tuple(float(v) for v in COINCIDENT), 0.1), (0, None, None)], 0.1, rng)


def ramp_colours(n):
    """greys (max == min), every ordering of r, g and b, the hues 0, 30, .. 330 exactly, then a ramp through the cube"""
    fixed = [(v, v, v) for v in (0, 1, 127, 128, 255)]
    fixed += list(itertools.permutations((10, 120, 250))) + list(itertools.permutations((200, 200, 40))) + list(itertools.permutations((40, 40, 200)))
    fixed += HUES_30
    i = np.arange(n, dtype=np.int64)
    ramp = np.stack([(i * 7) % 256, (i * 13 + 64) % 256, (i * 29 + 128) % 256], 1)
    rgb = np.concatenate([np.asarray(fixed, np.int64), ramp])[:n]
    return ((rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]).astype(np.uint32)


def ramp_case(seed=309):
    rng = np.random.default_rng(seed)
    p, n = vs.blob(rng, 2500)
    return _case("ramp", [(p, n)], [(0, None, None), (0, (0.15, 0.0, 0.05), 0.12)], 0.1, rng, [ramp_colours(len(p))])


def all_cases():
    return [balls_case(), skewed_case(), big_case(), mixed_case(), facing_case(), ties_case(), plane_case(), coincident_case(), ramp_case()]


def selected(case, region):
    """(points, colours) the region selects, by the restatement's rule"""
    o, centre, radius = region
    if not 0 <= o < len(case["objs"]):
        return np.zeros((0, 3), f32), np.zeros(0, np.uint32)
    p, c = case["objs"][o][0], case["rgba"][o]
    ok = np.isfinite(p).all(1)
    p, c = p[ok], c[ok]
    if radius is None or len(p) == 0:
        return p, c
    d2, _ = gr._sqdist(p, centre)
    keep = d2 < gr.r2_of(radius)
    return p[keep], c[keep]

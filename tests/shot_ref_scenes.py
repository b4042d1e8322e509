"""Small seeded scenes on which SHOT-352 / CSHOT-1344 of the device are held to the float64 restatement shot_ref.py (numpy only).
Small, because the restatement loops over neighbours in Python. Every scene is one object; `frames` holds the frames a scene
supplies itself (None: the frame estimate's, with `fixed_frames` overriding single keypoints). test_shot_ref_cpu.py proves the
properties each scene is built for; test_gpu_shot_ref.py runs the kernels on the same bytes."""
from collections import namedtuple

import numpy as np

import lab_ref
import shot_ref

f32 = np.float32
IDENTITY = f32([1, 0, 0, 0, 1, 0, 0, 0, 1])
Scene = namedtuple("Scene", "name points normals rgba keypoints kp_rgba radius cell frames fixed_frames")


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def decided_colours(rng, n):
    """n random 24-bit colours whose CIELab table entries no float32 evaluation can take differently (lab_ref.convert(...).decided)"""
    c = rng.integers(0, 1 << 24, size=2 * n + 64).astype(np.uint32)
    c = c[lab_ref.convert(c).decided]
    assert len(c) >= n
    return c[:n]


def colour_steps(kp_colour, colours):
    """(step_c, decided) of CSHOT's colour bin of `colours` against the keypoint colour, as shot_ref takes them"""
    both = lab_ref.convert(np.concatenate([np.asarray(colours, np.uint32).reshape(-1), [np.uint32(kp_colour)]]))
    e = both.e_norm + shot_ref.U * np.abs(both.norm)
    cd = shot_ref.color_distance32(both.norm[-1], both.norm[:-1]).astype(np.float64)
    es = e[:-1] + e[-1]
    d_cd = (es[:, 0] + (es[:, 1] + es[:, 2]) / 2) / 3 + 8 * shot_ref.U
    t = cd * 30 + 0.5
    same = (np.asarray(colours, np.uint32).reshape(-1) & 0xffffff) == (int(kp_colour) & 0xffffff)
    dec = (both.decided[:-1] & both.decided[-1] & (np.abs(t - np.rint(t)) > 30 * d_cd)) | same
    return np.floor(t).astype(int), dec


# ---------------------------------------------------------------------------------------------- sphere
SPHERE_RADIUS = 0.35
SPHERE_POINTS = 3000
SPHERE_ON_POINT, SPHERE_FAR, SPHERE_NAN, SPHERE_FOUR = 20, 21, 22, 23


def sphere(seed=71):
    """3000 points of a noisy unit sphere, outward normals, decided colours; 24 keypoints: 20 at 0.98 x a surface point, one ON a cloud
    point, one far away, one non-finite, and one above the surface with EXACTLY 4 points inside its ball (identity frame supplied:
    the frame estimate refuses it, and it is the descriptor's own count < 5 that is to answer)"""
    rng = np.random.default_rng(seed)
    d = _unit(rng.normal(size=(SPHERE_POINTS, 3)))
    p = (d * (1 + 0.01 * rng.normal(size=(SPHERE_POINTS, 1)))).astype(f32)
    kp = np.zeros((24, 3), f32)
    kp[:20] = (p[rng.choice(SPHERE_POINTS, 20, replace=False)] * f32(0.98)).astype(f32)
    kp[SPHERE_ON_POINT] = p[7]
    kp[SPHERE_FAR] = [30.0, 0, 0]
    kp[SPHERE_NAN] = [np.nan, 0, 0]
    for s in np.arange(1.20, 1.36, 0.0005):                     # walk outwards along one direction until 4 points are left in the ball
        q = (d[11] * s).astype(f32)
        if (((p.astype(np.float64) - q) ** 2).sum(1) < SPHERE_RADIUS ** 2).sum() == 4:
            kp[SPHERE_FOUR] = q
            break
    else:
        raise AssertionError("no keypoint with 4 neighbours")
    return Scene("sphere", p, d.astype(f32), decided_colours(rng, SPHERE_POINTS), kp, decided_colours(rng, 24), SPHERE_RADIUS, 0.1, None,
                 {SPHERE_FOUR: IDENTITY})


# ---------------------------------------------------------------------------------------------- pole and seams
POLE_RADIUS = 0.5


def pole_and_seams(seed=72):
    """one keypoint at the origin, identity frame: 200 neighbours within 1e-4 .. 1e-2 rad of +-z, 200 within the same of the equator,
    200 within 1e-6 relative of |x| = |y|, of x = 0 and of y = 0 -- BESIDE the hard decisions, never on them; distances spread over the
    four radial cases. Where the float elevation (1 / sqrt(1 - ic^2)) and azimuth are worst conditioned."""
    rng = np.random.default_rng(seed)

    def spherical(theta, phi, rho):
        return np.stack([rho * np.sin(theta) * np.cos(phi), rho * np.sin(theta) * np.sin(phi), rho * np.cos(theta)], -1)

    rho = lambda n: np.resize([0.06, 0.2, 0.3, 0.45], n) * rng.uniform(0.9, 1.05, size=n)     # < r/4, r/4..r/2, r/2..3r/4, > 3r/4
    small = lambda n: 10.0 ** rng.uniform(-4, -2, size=n) * rng.choice([-1.0, 1.0], size=n)
    th = np.abs(small(200)); th[::2] = np.pi - th[::2]
    pole = spherical(th, rng.uniform(-np.pi, np.pi, 200), rho(200))
    equator = spherical(np.pi / 2 + small(200), rng.uniform(-np.pi, np.pi, 200), rho(200))
    phi0 = np.resize(np.arange(8) * np.pi / 4, 200)                                            # the diagonals and the axes of the xy plane
    seam = spherical(rng.uniform(0.3, 2.8, 200), phi0 + 1e-6 * rng.choice([-1.0, 1.0], size=200) * rng.uniform(0.3, 1.0, 200), rho(200))
    p = np.concatenate([pole, equator, seam]).astype(f32)
    n = _unit(rng.normal(size=(len(p), 3))).astype(f32)
    return Scene("pole_and_seams", p, n, decided_colours(rng, len(p)), np.zeros((1, 3), f32), decided_colours(rng, 1), POLE_RADIUS, 0.125,
                 IDENTITY.reshape(1, 9), {})


# ---------------------------------------------------------------------------------------------- palette
PALETTE_RADIUS = 0.5
PALETTE_POINTS = 400
WHITE, BLACK, GREY = 0xffffff, 0x000000, 0x6b8e23
GRID17 = np.arange(0, 256, 17)


def palette_pool():
    """the cube's corners, edges and a 16^3 lattice of it (step 17: 0, 17 .. 255): 4096 colours"""
    r, g, b = np.meshgrid(GRID17, GRID17, GRID17, indexing="ij")
    return ((r.astype(np.uint32) << 16) | (g.astype(np.uint32) << 8) | b.astype(np.uint32)).reshape(-1)


def palette_max_step(kp_colour):
    """the largest colour step the lattice of palette_pool() reaches from kp_colour, decided or not (test_lab_cpu.py: the whole cube reaches
    no further from white and from black)"""
    return int(colour_steps(kp_colour, palette_pool())[0].max())


def palette(kp_colour, seed=73, uniform=False):
    """one keypoint of colour kp_colour at the origin, 400 neighbours in generic position whose colours hit EVERY colour step from 0 to
    the largest the cube reaches from kp_colour (each step at least 4 times; decided colours only). uniform: every neighbour has the
    keypoint's colour instead (cd = 0: all colour weight in step 0, every other colour bin receives exactly 0)."""
    rng = np.random.default_rng(seed)
    p = (_unit(rng.normal(size=(PALETTE_POINTS, 3))) * rng.uniform(0.03, 0.49, size=(PALETTE_POINTS, 1))).astype(f32)
    n = _unit(rng.normal(size=(PALETTE_POINTS, 3))).astype(f32)
    if uniform:
        rgba = np.full(PALETTE_POINTS, kp_colour, np.uint32)
    else:
        pool = np.concatenate([palette_pool(), decided_colours(rng, 4000)])
        step, dec = colour_steps(kp_colour, pool)
        top = palette_max_step(kp_colour)
        picks = []
        for s in range(top + 1):
            have = pool[dec & (step == s)]
            assert len(have) >= 1, (hex(kp_colour), s)
            picks.append(np.resize(have, 4))
        picks = np.concatenate(picks)
        rest = pool[dec][rng.integers(0, dec.sum(), size=PALETTE_POINTS - len(picks))]
        rgba = np.concatenate([picks, rest]).astype(np.uint32)
    name = "palette_%06x%s" % (kp_colour, "_uniform" if uniform else "")
    return Scene(name, p, n, rgba, np.zeros((1, 3), f32), np.uint32([kp_colour]), PALETTE_RADIUS, 0.125, IDENTITY.reshape(1, 9), {})


# ---------------------------------------------------------------------------------------------- dense
DENSE_RADIUS = 0.5
DENSE_POINTS = 20000


def dense(seed=74):
    """one keypoint, 20 000 neighbours inside its ball, FOUR colours (one of them the keypoint's): the largest same-address contention per
    colour bin (5 000 neighbours share each colour step) and the longest fixed-point sums"""
    rng = np.random.default_rng(seed)
    p = (_unit(rng.normal(size=(DENSE_POINTS, 3))) * (0.49 * rng.uniform(0.001, 1.0, size=(DENSE_POINTS, 1)) ** (1 / 3))).astype(f32)
    n = _unit(rng.normal(size=(DENSE_POINTS, 3))).astype(f32)
    four = decided_colours(rng, 64)
    step, dec = colour_steps(four[0], four)
    four = four[dec][:4]
    assert len(four) == 4 and len(set(step[dec][:4].tolist())) >= 3
    return Scene("dense", p, n, four[rng.integers(0, 4, size=DENSE_POINTS)], np.zeros((1, 3), f32), four[:1].copy(), DENSE_RADIUS, 0.125,
                 IDENTITY.reshape(1, 9), {})


BUILDERS = {"sphere": sphere, "pole_and_seams": pole_and_seams, "palette_white": lambda: palette(WHITE), "palette_black": lambda: palette(BLACK),
            "palette_uniform": lambda: palette(GREY, uniform=True), "dense": dense}
_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = BUILDERS[name]()
    return _scenes[name]


def with_fixed_frames(s, frames):
    """the frames a scene is described on: its own, or `frames` (the frame estimate's) with the scene's fixed ones put in"""
    if s.frames is not None:
        return s.frames.astype(f32)
    fr = np.array(frames, f32).reshape(-1, 9)
    for k, f in s.fixed_frames.items():
        fr[k] = f
    return fr


def reference(s, frames):
    """shot_ref.cshot1344 of every keypoint on `frames` -> list of shot_ref.Row (the shape half of each is SHOT-352's row)"""
    return [shot_ref.cshot1344(s.points, s.normals, s.rgba, k, c, f, s.radius) for k, c, f in zip(s.keypoints, s.kp_rgba, frames)]


def sector_sums(rows):
    """per row and sector: the sum of the 11 shape bins and of the 31 colour bins of a CSHOT row [n, 1344] -> two [n, 32] float64 arrays"""
    r = np.asarray(rows, np.float64)
    return r[:, :352].reshape(-1, 32, 11).sum(2), r[:, 352:].reshape(-1, 32, 31).sum(2)


def sector_sum_bound(shape_sums, colour_sums):
    """Bound [n, 32] on |shape sector sum - colour sector sum| of a DEVICE CSHOT row, from the row alone (u = 2^-24).
    Of one neighbour, the side deposits (radial, elevation, azimuth) are the same float value in both channels, rounded to the same
    multiple of 2^-28: they cancel. Its home sector receives |off| and fl(fl(1 - |off|) + winc) at the channel's own step, in exact
    arithmetic 1 + winc in either channel; in float the subtraction is off by <= u (a value <= 1), the sum by <= 2 u (half an ulp of
    a value < 4) and the two fixed-point roundings by 2^-29 each = u / 16: 3.0625 u per neighbour and channel, 6.125 u between the
    channels. A home neighbour adds 1 + winc >= 1 to the sector's sum, so the n_s neighbours of sector s move the unnormalised
    difference by <= 6.125 u n_s <= 6.125 u (sector sum): the relation survives the division by the joint norm. Each output is
    fl(fl(h 2^-28) / fn): 2 u relative per value, 2 u (sector sum) per channel. Total 10.125 u * the larger of the two sector sums."""
    return 10.125 * shot_ref.U * shot_ref.SLACK * np.maximum(np.abs(shape_sums), np.abs(colour_sums))


def oracle_sector_sum_bound(shape_sums, colour_sums, count):
    """The same for the float CPU oracle, which ADDS every deposit to a float bin like the reference: a bin built by m additions of
    non-negative terms is off by <= m u (bin) (each deposit's own float cast included), m <= 5 per neighbour (2 home, <= 3 side);
    two channels -> 2 (5 n + 4) u * the larger sector sum (the 4: norm, cast and divide of the output)."""
    n = np.asarray(count, np.float64).reshape(-1, 1)
    return 2 * (5 * n + 4) * shot_ref.U * np.maximum(np.abs(shape_sums), np.abs(colour_sums))

"""The cases of the SHORT_CSHOT tests, shared by the CPU tests (which prove on the restatement that no neighbour of any case sits within
a libm difference of a hard geometric bin decision of either grid) and the GPU tests (which run ismhip_short_cshot on exactly the
same bytes). The geometry is that of short_shot_scenes.py (mid, thin, queue, lattice); this module adds seeded random 24-bit colours per
point and keypoint, a palette object, and the colour edge list on the lattice. numpy only.

A case wraps a short_shot_scenes.Case (objects, keypoints, cell, radius, shape bins, frames, minimum-radius options) and adds the colour
grid, the colour histogram size and the colours."""
from dataclasses import dataclass

import numpy as np

import frontend_scenes as fs
import short_cshot_ref as scr
import short_shot_scenes as sss

f32 = np.float32
DEFAULT = ((2, 2, 8), (2, 2, 8), 15)                           # 32 + 32 * 15 = 512 bins
# (shape bins, colour grid, H): the default; single-bin axes everywhere (16 bins, no c2, no r2, no theta2); the long row (1216 bins, a
# colour grid that differs from the shape grid); 15 + 8 * 7 = 71 bins, no multiple of 4, grids that differ
MID_CONFIGS = [DEFAULT, ((1, 1, 8), (1, 1, 8), 1), ((8, 4, 8), (2, 4, 8), 15), ((1, 3, 5), (1, 1, 8), 7)]
WHITE, BLACK = 0xFFFFFF, 0x000000

# Neighbour colours whose raw_c = float32(colour distance to EDGE_KP_COLOR * 15) sits ON a hard decision of the colour bin or on the
# float32 beside it: (colour, kind, n) with kind "half" (raw_c == n + 0.5: decimals <= 0.5f holds with equality), "half-below" /
# "half-above" (the adjacent float32 values), "int" (raw_c == n >= 1: the truncation) and "int-below". Made as frontend_scenes.EDGE_COLORS
# was: a vectorised numpy scan of all 2^24 colours (the two LUTs filled by libm's powf, which makes the numpy copy of Appendix A.3's
# formulas bit-equal to the oracle's rgb2lab) with short_cshot_ref.color_distance, every hit confirmed through the oracle's rgb2lab;
# test_short_cshot_cpu.py confirms the list itself. All five kinds exist among the 2^24 colours; the largest raw_c against this
# keypoint colour is 8.76, so n stops at 8.
EDGE_KP_COLOR = fs.EDGE_KP_COLOR
EDGE_H = 15
EDGE_COLORS = [(12639578, "half", 0), (13495970, "int-below", 1), (4819200, "half", 2), (12162319, "int", 2), (443158, "int-below", 2),
               (1730841, "half", 3), (16622234, "int", 3), (3976118, "int-below", 3), (13310214, "half-above", 4), (2070508, "half-below", 4),
               (3886098, "int", 4), (10430281, "half", 5), (4946407, "half-above", 5), (2980326, "half-below", 5), (14052539, "int-below", 5),
               (7229867, "int", 6), (2243176, "int-below", 6), (336530, "half", 7), (1316599, "half-below", 8), (6947543, "int", 8),
               (1445008, "int-below", 8)]


def edge_value(kind, n):
    """the float32 raw_c an EDGE_COLORS entry stands for"""
    v = f32(n + 0.5) if kind.startswith("half") else f32(n)
    return np.nextafter(v, f32(-1)) if kind.endswith("below") else np.nextafter(v, f32(99)) if kind.endswith("above") else v


def edge_raw_c(rgb2lab, colors, kp_color=EDGE_KP_COLOR, hist_size=EDGE_H):
    """raw_c of the restatement for neighbour colours against kp_color -> float32 [n]"""
    lab = scr.lab_table(rgb2lab, list(colors) + [kp_color])
    return (scr.color_distance(lab[-1], lab[:-1]).astype(np.float64) * hist_size).astype(f32)


@dataclass
class ColorCase:
    geo: sss.Case
    color_bins: tuple
    hist_size: int
    rgba: list                      # per object: uint32 [n_points]
    kp_rgba: list                   # per object: uint32 [n_keypoints]
    tag: str = ""

    @property
    def name(self):
        opts = (f"-min{self.geo.min_radius_relative}" if self.geo.use_min_radius else "") + ("-log" if self.geo.log_radius else "")
        return f"{self.geo.name}-{self.color_bins}-{self.hist_size}{opts}{self.tag}"

    @property
    def dim(self):
        return scr.total_dims(self.geo.bins, self.color_bins, self.hist_size)

    def reference(self, rgb2lab, frames):
        pt_off, p, _, kp_off, kp = self.geo.soa()
        return scr.short_cshot_ref(rgb2lab, pt_off, p, np.concatenate(self.rgba), kp_off, kp, np.concatenate(self.kp_rgba), frames, self.geo.radius,
                                   self.geo.bins, self.color_bins, self.hist_size, self.geo.min_radius, self.geo.log_radius)


_colors = {}


def random_colors(geo, seed):
    """seeded random 24-bit colours for every point and keypoint of a geometry (one draw per scene, shared by its cases)"""
    key = (id(geo.objs), seed)
    if key not in _colors:
        rng = np.random.default_rng(seed)
        _colors[key] = ([rng.integers(0, 1 << 24, size=len(p)).astype(np.uint32) for p, _ in geo.objs],
                        [rng.integers(0, 1 << 24, size=len(k)).astype(np.uint32) for k in geo.kps])
    return _colors[key]


def _colored(geo, color_bins, hist_size, seed, tag=""):
    rgba, kp_rgba = random_colors(geo, seed)
    return ColorCase(geo, color_bins, hist_size, rgba, kp_rgba, tag)


def mid_case(cfg=DEFAULT, **kw):
    return _colored(sss.mid_case(cfg[0], **kw), cfg[1], cfg[2], 71)


def thin_case(cfg=DEFAULT):
    return _colored(sss.thin_case(cfg[0]), cfg[1], cfg[2], 72)


def queue_case(cfg=DEFAULT, **kw):
    return _colored(sss.queue_case(cfg[0], **kw), cfg[1], cfg[2], 73)


def palette_case(cfg=DEFAULT):
    """the mid object in three colours: a third of the points carry the colour every keypoint has (cd = 0 exactly, raw_c = 0, bin 0 with
    share 0.5 and no secondary colour bin), the others are black or white"""
    geo = sss.mid_case(cfg[0])
    key = (id(geo.objs), "palette")
    if key not in _colors:
        rng = np.random.default_rng(74)
        own = fs.EDGE_KP_COLOR
        _colors[key] = ([np.asarray([own, BLACK, WHITE], np.uint32)[rng.integers(0, 3, size=len(p))] for p, _ in geo.objs],
                        [np.full(len(k), own, np.uint32) for k in geo.kps])
    rgba, kp_rgba = _colors[key]
    return ColorCase(geo, cfg[1], cfg[2], rgba, kp_rgba, "-palette")


def lattice_case(cfg=DEFAULT, radius=0.5):
    """the dyadic lattice in two frames; its 26 points nearest the keypoint (inside every radius, off the keypoint) carry the 21 edge
    colours, placed as frontend_scenes.lattice_colors places its own list; the keypoints have EDGE_KP_COLOR"""
    geo = sss.lattice_case(cfg[0], radius)
    rgba = []
    for p, _ in geo.objs:
        c = fs.lattice_colors(p)                               # random elsewhere
        d2 = (p.astype(np.float64) ** 2).sum(1)
        near = np.argsort(d2, kind="stable")[1:1 + len(EDGE_COLORS)]
        c[near] = [col for col, _, _ in EDGE_COLORS]
        rgba.append(c.astype(np.uint32))
    return ColorCase(geo, cfg[1], cfg[2], rgba, [np.array([EDGE_KP_COLOR], np.uint32) for _ in geo.objs], "-edges")


def parity_cases():
    """the cases of the GPU parity test: the smallest that reach each path"""
    return ([mid_case(c) for c in MID_CONFIGS] + [thin_case(), queue_case(),
            queue_case(use_min_radius=True, min_radius_relative=0.4), queue_case(use_min_radius=True, min_radius_relative=0.9),
            mid_case(log_radius=True), lattice_case(), palette_case()])

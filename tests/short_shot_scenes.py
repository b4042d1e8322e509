"""The cases of the SHORT_SHOT tests, shared by the CPU tests (which prove on the restatement that no neighbour of any case sits
within a libm difference of a hard bin decision) and the GPU tests (which run ismhip_short_shot on exactly the same bytes).
The scenes are those of frontend_scenes.py; this module only picks keypoints, radii and grids. numpy only.

A case is a Case below. Frames: `lrf(case)` of the caller (the oracle's on the CPU, capi.shot_lrf on the GPU: equal to 1e-5, so the
margins of one carry over to the other only statistically -- the GPU tests therefore exempt nothing and compare every keypoint)
fills the frames of the cases with frames=None; `override` then replaces single rows (identity where the frame estimate has no
neighbours but the descriptor must run, NaN for the NaN-frame row)."""
from dataclasses import dataclass, field

import numpy as np

import frontend_scenes as fs
import short_shot_ref as ssr

f32 = np.float32
GRIDS = [(2, 2, 8), (1, 1, 8), (8, 4, 8), (1, 3, 5)]           # auto 32, auto 8, auto 256, a manual grid of 15 bins (no multiple of 4)
IDENTITY = f32([1, 0, 0, 0, 1, 0, 0, 0, 1])
NAN_FRAME = np.full(9, np.nan, f32)
MID_RADIUS, MID_CELL = 0.25, 0.1
MID_ON_POINT, MID_NAN_FRAME, MID_EMPTY_BALL, MID_OFF_GRID = 0, 5, 24, 25      # keypoint rows of the mid scene


@dataclass
class Case:
    name: str
    objs: list                      # [(points, normals)]
    kps: list                       # [keypoints]
    cell: float
    radius: float
    bins: tuple
    frames: np.ndarray = None       # [nkp, 9] supplied frames; None: estimated (radius `radius`)
    override: dict = field(default_factory=dict)   # keypoint row -> frame
    use_min_radius: bool = False
    min_radius_relative: float = 0.0
    log_radius: bool = False

    @property
    def min_radius(self):
        return float(ssr.min_radius_of(self.radius, self.use_min_radius, self.min_radius_relative, self.log_radius))

    def soa(self):
        return fs.soa(self.objs, self.kps)

    def frames_from(self, estimated):
        fr = np.array(self.frames if self.frames is not None else estimated, f32).reshape(-1, 9)
        for row, f in self.override.items():
            fr[row] = f
        return fr

    def reference(self, frames):
        pt_off, p, _, kp_off, kp = self.soa()
        return ssr.short_shot_ref(pt_off, p, kp_off, kp, frames, self.radius, self.bins, self.min_radius, self.log_radius)


_built = {}


def _mid():
    """the mid object with 24 keypoints just inside its surface (row 0 ON a cloud point, row 5 gets a NaN frame), one at the
    ellipsoid's centre (inside the grid, empty ball) and one far outside the grid"""
    if "mid" not in _built:
        p, n, rng = fs.mid_object()
        kp = (p[rng.choice(6000, 24, replace=False)] * f32(0.98)).astype(f32)
        kp[MID_ON_POINT] = p[7]
        kp = np.concatenate([kp, f32([[0, 0, 0], [30, 0, 0]])])
        _built["mid"] = ([(p, n)], [kp])
    return _built["mid"]


_MID_OVERRIDE = {MID_NAN_FRAME: NAN_FRAME, MID_EMPTY_BALL: IDENTITY, MID_OFF_GRID: IDENTITY}


def _thin():
    """the thin batch with every fifth keypoint of its two dense objects (balls of up to 54 000 neighbours: the restatement stays
    quick), plus five more copies of its small sphere with 3, 1, 2, 0 and 3 keypoints: nine objects, so the XCD block map deals one
    full group of eight and a second group with padding blocks, over ragged keypoint runs, an empty one included"""
    if "thin" not in _built:
        b = fs.thin_batch()
        objs, kps = list(b["objs"]), [b["kps"][0][::5], b["kps"][1][::5], b["kps"][2][:5], b["kps"][3]]
        sp = objs[3][0]
        for j, n in enumerate((3, 1, 2, 0, 3)):
            objs.append(objs[3])
            kps.append((sp[10 * j + 5:10 * j + 5 + n] * f32(0.97)).astype(f32).reshape(-1, 3))
        _built["thin"] = (objs, kps)
    return _built["thin"]


def _queue():
    if "queue" not in _built:
        pts, nrm, kps, frames, counts = fs.queue_clusters()
        _built["queue"] = ([(pts, nrm)], [kps], frames, counts)
    return _built["queue"]


def mid_case(bins, **kw):
    objs, kps = _mid()
    return Case(f"mid-{bins}", objs, kps, MID_CELL, MID_RADIUS, bins, override=dict(_MID_OVERRIDE), **kw)


def thin_case(bins):
    objs, kps = _thin()
    return Case(f"thin-{bins}", objs, kps, fs.THIN_CELL, fs.THIN_RADIUS, bins)


def queue_case(bins, **kw):
    """the scene's own random frames: the frame estimate refuses the 4-neighbour clusters, the descriptor must not"""
    objs, kps, frames, _ = _queue()
    return Case(f"queue-{bins}", objs, kps, 0.12, fs.QUEUE_RADIUS, bins, frames=frames, **kw)


def lattice_case(bins, radius):
    """the dyadic lattice in the identity frame and in one rotated frame: local coordinates, r and (linear) raw_r are exact, so
    neighbours sit EXACTLY on radial bin boundaries and on the radial switch (r = 3/8 with radius 1/2 and two bins: raw_r = 1.5)"""
    frames = np.stack([fs.LATTICE_FRAMES[0], fs.LATTICE_FRAMES[1]])
    objs = [fs.lattice(fr) for fr in frames]
    return Case(f"lattice-{bins}-{radius}", objs, [np.zeros((1, 3), f32)] * 2, 0.125, radius, bins, frames=frames)


def grid_cases():
    """the four grids on the three scenes"""
    return [mk(b) for mk in (mid_case, thin_case, queue_case) for b in GRIDS]


def option_cases():
    """log radius (default minimum radius, and an explicit one), UseMinRadius, and a minimum radius above every neighbour"""
    return [mid_case((2, 2, 8), log_radius=True), mid_case((8, 4, 8), log_radius=True, use_min_radius=True, min_radius_relative=0.3),
            queue_case((2, 2, 8), use_min_radius=True, min_radius_relative=0.4), queue_case((2, 2, 8), use_min_radius=True, min_radius_relative=0.9)]


def lattice_cases():
    return [lattice_case(b, r) for b in ((2, 2, 8), (8, 4, 8)) for r in (0.5, 0.75)]


def all_cases():
    return grid_cases() + option_cases() + lattice_cases()

"""Voxel-grid keypoints of voxel.hip against pcl::VoxelGrid with exact sums (voxel_ref.py), -m gpu, on the scenes of
prepath_scenes.py: points on voxel faces (negative ones too), one voxel of 30 000 points, an object far from the origin, a table
of 2 M entries for 500 points, a ragged batch with empty, all-NaN, single-point and duplicate-point objects.

kp_off, voxel order and colours are exact. Every coordinate lies within 2^-22 |exact| + 2^-39 maxabs of the exact mean (maxabs: the
object's largest |coordinate|): twice the derived bound -- fixed-point rounding <= 2^-40 maxabs, one float32 rounding of the sum
and one float32 division, 2^-24 each."""
import numpy as np
import pytest

import prepath_scenes as ps
import voxel_ref as vr

pytestmark = pytest.mark.gpu


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("name", list(ps.VOXEL_SCENES))
def test_voxel_keypoints_match_exact_means(pkg, gpu, name, color):
    """Largest error measured on the MI355X, in units of the bound (the same with and without colour): faces 0.31 (leaf 0.25) and
    0.36 (leaf 0.1), crowded 0.37 (one voxel of 30 003 points), far 0.32, sparse_table 0 (one point per voxel), ragged 0.37."""
    ctx, dev = gpu
    s = ps.voxel_scene(name)
    off, P = ps.flat(s["objs"])
    rgba = np.concatenate(s["rgba"]).astype(np.uint32)
    ko, kx, ky, kz, kc = pkg.capi.voxel_keypoints(ctx, off, *[T(P[:, a].copy(), dev) for a in range(3)], s["leaf"],
                                                  rgba=T(rgba.view(np.int32), dev) if color else None)
    got = np.stack([kx.cpu().numpy(), ky.cpu().numpy(), kz.cpu().numpy()], 1).astype(np.float64)
    assert (kc is not None) == color
    want_off = np.concatenate([[0], np.cumsum([len(r["key"]) for r in s["ref"]])])
    assert np.array_equal(np.asarray(ko, np.int64), want_off), (ko, want_off)
    worst = 0.0
    for o, ref in enumerate(s["ref"]):
        a, b = int(want_off[o]), int(want_off[o + 1])
        if a == b:
            continue
        # a centroid in the wrong voxel or out of order is off by a leaf, a million times the bound
        units = np.abs(got[a:b] - ref["xyz"]) / vr.bound(ref["xyz"], ref["maxabs"])
        worst = max(worst, float(units.max()))
        if color:
            assert np.array_equal(kc.cpu().numpy()[a:b].view(np.uint32), ref["rgba"]), o
    print(f"{name}, colour {color}: {int(want_off[-1])} keypoints, largest error {worst:.3g} of the bound, largest voxel {max(int(r['count'].max()) for r in s['ref'] if len(r['count']))} points")
    assert worst <= 1.0, worst
    if name == "ragged":
        n_kp = np.diff(want_off)
        assert n_kp[ps.RAGGED_EMPTY] == 0 and n_kp[ps.RAGGED_NAN] == 0 and n_kp[ps.RAGGED_SINGLE] == 1
        assert np.array_equal(got[want_off[ps.RAGGED_SINGLE]].astype(np.float32), s["objs"][ps.RAGGED_SINGLE][0])
        for o in ps.RAGGED_DUP:
            assert n_kp[o] == 1 and np.array_equal(got[want_off[o]].astype(np.float32), ps.RAGGED_DUP_POINT), (o, got[want_off[o]])

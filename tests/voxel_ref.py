"""pcl::VoxelGrid keypoints of ONE object with exact sums (numpy only).

Voxel index in float32, as k_vox_accum and PCL form it: inv = float32(1) / float32(leaf), i_a = int(floor(float32(p_a * inv)) -
float32(minb_a)), minb / div from the float32 bounding box of the finite points; output in ascending i0 + i1 * div0 + i2 * div0 * div1.
Centroid: the exact mean (float64 sums of float32 data; exact to 2^-53 for the inputs of the tests). Colour: per channel
uint8(float32(sum) / float32(count)) with integer sums."""
import numpy as np

f32 = np.float32


def voxel_index(p, leaf):
    """-> (key [n] int64, minb [3], div [3]) of finite float32 points p [n, 3]"""
    inv = f32(1) / f32(leaf)
    cell = lambda a: np.floor((np.asarray(a, f32) * inv).astype(f32))
    minb, maxb = cell(p.min(0)).astype(np.int64), cell(p.max(0)).astype(np.int64)
    div = maxb - minb + 1
    i = (cell(p) - minb.astype(f32)).astype(f32).astype(np.int64)
    return i[:, 0] + i[:, 1] * div[0] + i[:, 2] * div[0] * div[1], minb, div


def on_face(p, leaf):
    """[n, 3] bool: float32(p * inv) is an integer, i.e. the coordinate sits on a voxel face as the kernel sees it"""
    t = (np.asarray(p, f32) * (f32(1) / f32(leaf))).astype(f32)
    return t == np.floor(t)


def voxel_ref(xyz, leaf, rgba=None):
    """-> dict(key, count, xyz [m, 3] float64, rgba [m] uint32 or None, maxabs, n_table)"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    fin = np.isfinite(xyz).all(1)
    p = xyz[fin]
    if len(p) == 0:
        return dict(key=np.zeros(0, np.int64), count=np.zeros(0, np.int64), xyz=np.zeros((0, 3)), maxabs=0.0, n_table=0,
                    rgba=None if rgba is None else np.zeros(0, np.uint32))
    key, _, div = voxel_index(p, leaf)
    uniq, inv_idx, count = np.unique(key, return_inverse=True, return_counts=True)
    inv_idx = inv_idx.reshape(-1)
    mean = np.stack([np.bincount(inv_idx, weights=p[:, a].astype(np.float64), minlength=len(uniq)) for a in range(3)], 1) / count[:, None]
    out = dict(key=uniq, count=count, xyz=mean, rgba=None, maxabs=float(np.abs(p).max()), n_table=int(div.prod()))
    if rgba is not None:
        c = np.asarray(rgba, np.uint32)[fin]
        col = np.zeros(len(uniq), np.uint32)
        for shift in (16, 8, 0):
            s = np.bincount(inv_idx, weights=((c >> shift) & 0xff).astype(np.float64), minlength=len(uniq)).astype(np.int64)
            assert s.max() < 1 << 24                               # the integer sum is exact in float32, as voxel.hip assumes
            ch = (s.astype(f32) / count.astype(f32)).astype(f32).astype(np.uint8)
            col |= ch.astype(np.uint32) << shift
        out["rgba"] = col
    return out


def bound(exact, maxabs):
    """per coordinate: twice (fixed-point rounding 2^-40 maxabs + one float32 rounding of the sum + one float32 division, 2^-24 each)"""
    return 2.0 ** -22 * np.abs(exact) + 2.0 ** -39 * maxabs

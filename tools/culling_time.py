"""VoxelGridCulling keypoints on the device -- the measurement of DESIGN.md 4.18.
Workload of tools/iss3d_time.py: --objects bumpy ellipsoids of --points points each (tests/iss3d_scenes.bumpy_ellipsoid, about one unit
across) with the normals and colours of tests/culling_scenes.py, LeafSize --leaf. On the same cloud in the same process, device events (the
library timers), --warmup runs, then --reps repetitions of
  ismhip_principal_curvatures   timer "culling_pc" (dense: one value pair per surface point; needed by kpq only)
  ismhip_culling_scores         timer "culling_scores", per method: curvature, kpq, colordistance, and kpq + colordistance in one sweep
  ismhip_culling_select         timer "culling_select" and the wall time of the whole call (it synchronises: the per-object scan, the
                                offsets' round trip and the gather of the ordered compaction)
and beside them, in the same run, the yardsticks
  ismhip_iss3d_keypoints        timers "iss3d_saliency" (the same kind of dense sweep, SalientRadius = leaf) and "iss3d_nms"
  ismhip_voxel_keypoints        timer "voxel_keypoints" (the keypoints every method starts from)
Reported as median [min .. max] milliseconds; every figure is measured. The outputs of all repetitions are compared bit for bit.

    python tools/culling_time.py [--objects 256] [--points 16384] [--reps 20] [--warmup 3] [--leaf 0.1]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge      # noqa: E402
import culling_scenes as scenes   # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.1)
    args = ap.parse_args()
    capi = ge.load_package().capi

    import torch
    dev = torch.device("cuda:0")
    n_obj, n, leaf = args.objects, args.points, args.leaf
    objs = [scenes.make(n, 100 + o) for o in range(n_obj)]
    off, xyz, nrm, rgba = scenes.concat(objs)
    t = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (xyz, nrm) for i in range(3)]
    c = torch.as_tensor(rgba.view(np.int32)).to(dev)
    print(f"{n_obj} objects of {n} points, LeafSize {leaf}, FilterCutoffRatio 0.5, MaxSimilarColorDistance 0.05 (all figures measured)")
    ctx = capi.Ctx(0)
    cloud = capi.Cloud(ctx, off, *t, 0.4 * leaf, rgba=c)
    ctx.timers_enable(True)

    def timed(label, names, call):
        ms, wall, first = {k: [] for k in names}, [], None
        for rep in range(args.warmup + args.reps):
            ctx.sync(); ctx.timers_reset()
            t0 = time.perf_counter()
            out = call()
            ctx.sync()
            dt = (time.perf_counter() - t0) * 1e3
            if first is None:
                first = [o.clone() for o in out]
            for a, b in zip(first, out):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: outputs differ between two runs"
            if rep >= args.warmup:
                wall.append(dt)
                for k in names:
                    ms[k].append(ctx.timer(k)[0])
        for k in names:
            print(f"{label} timer {k}: {spread(ms[k])} ms")
        print(f"{label} whole call (wall): {spread(wall)} ms")
        return first

    def voxel():
        ko, kx, ky, kz, kc = capi.voxel_keypoints(ctx, off, *t[:3], leaf, rgba=c)
        return [torch.as_tensor(ko.astype(np.int32)), kx, ky, kz, kc]
    ko_t, kx, ky, kz, kc = timed("voxel_keypoints", ("voxel_keypoints",), voxel)
    ko = ko_t.numpy().astype(np.uint32)
    pc1, pc2, cnt = timed("principal_curvatures", ("culling_pc",), lambda: list(capi.principal_curvatures(ctx, cloud, leaf)))
    print(f"voxel keypoints {int(ko[-1])} ({int(ko[-1]) / n_obj:.1f} per object), neighbours per surface point mean {float(cnt.float().mean()):.1f} max {int(cnt.max())}")
    for geometry, color in (("curvature", "none"), ("kpq", "none"), ("none", "colordistance"), ("kpq", "colordistance")):
        label = f"culling_scores {geometry} + {color}"
        geo, col, kcnt = timed(label, ("culling_scores",), lambda: list(capi.culling_scores(ctx, cloud, ko, kx, ky, kz, kc, leaf, geometry, color, 0.05, pc1, pc2)))

        def select():
            r = capi.culling_select(ctx, ko, geo, col, kx, ky, kz, kc, geometry != "none", color != "none")
            return [torch.as_tensor(r["kp_offsets"].astype(np.int32)), r["kx"], r["keep"].to(torch.int32), r["thresholds"]]
        kept = timed(f"culling_select after {geometry} + {color}", ("culling_select",), select)
        print(f"{label}: ball points per keypoint mean {float(kcnt.float().mean()):.1f} max {int(kcnt.max())}, kept {int(kept[0][-1])} of {int(ko[-1])}")

    def iss():
        o, x, y, z, _kc, src = capi.iss3d_keypoints(ctx, cloud, leaf, leaf / 2)
        return [torch.as_tensor(o.astype(np.int32)), x, y, z, src]
    timed(f"iss3d_keypoints (SalientRadius {leaf}, NonMaxRadius {leaf / 2})", ("iss3d_saliency", "iss3d_nms"), iss)
    ctx.timers_enable(False)
    cloud.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""SIFT3D keypoints on the device -- the measurement of DESIGN.md 4.23.
Workload: --objects bumpy ellipsoids of --points points each (tests/iss3d_scenes.bumpy_ellipsoid, about one unit across). On the same cloud
in the same process, device events (the library timers), --warmup runs, then --reps repetitions of
  ismhip_normal_curvature     timer "normal_curvature" at --normal-radius: the intensity the detector reads
  ismhip_sift3d_keypoints     timers "voxel_downsample_xyzi", "grid", "sift3d_scale_space", "sift3d_extrema", "sift3d_emit" (summed over the
                              octaves) and the wall time of the whole call (it synchronises once per octave for the sizes and counts)
  ismhip_iss3d_keypoints      timers "iss3d_saliency", "iss3d_nms" and the wall time: the dense sibling
  ismhip_voxel_keypoints      timer "voxel_keypoints" and the wall time at leaf --radius: the cheapest detector, one octave's first step
Reported as median [min .. max] milliseconds. The outputs of all repetitions are compared bit for bit.

    python tools/sift3d_time.py [--objects 256] [--points 16384] [--reps 20] [--warmup 3] [--radius 0.05] [--normal-radius 0.05]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge   # noqa: E402
import iss3d_scenes as scenes  # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--normal-radius", type=float, default=0.05)
    args = ap.parse_args()
    capi = ge.load_package().capi

    import torch
    dev = torch.device("cuda:0")
    n_obj, n = args.objects, args.points
    p = np.concatenate([scenes.bumpy_ellipsoid(n, 100 + o) for o in range(n_obj)])
    off = (np.arange(n_obj + 1) * n).astype(np.uint32)
    t = [torch.as_tensor(np.ascontiguousarray(p[:, i])).to(dev) for i in range(3)] + [torch.zeros(len(p), dtype=torch.float32, device=dev) for _ in range(3)]
    print(f"{n_obj} objects of {n} points, Radius {args.radius}, 4 octaves of 3 scales, NormalRadius {args.normal_radius}")
    ctx = capi.Ctx(0)
    cloud = capi.Cloud(ctx, off, *t, 0.4 * args.radius)
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

    curv = timed("normal_curvature", ("normal_curvature",), lambda: [capi.normal_curvature(ctx, cloud, args.normal_radius, want_counts=False)[0]])[0]
    print(f"curvature: {int(torch.isfinite(curv).sum())} of {len(curv)} points finite")

    def sift():
        ko, kx, ky, kz, ks, sizes = capi.sift3d_keypoints(ctx, cloud, curv, args.radius)
        return [torch.as_tensor(ko.astype(np.int32)), kx, ky, kz, ks, torch.as_tensor(sizes.astype(np.int32))]
    kp = timed("sift3d_keypoints", ("voxel_downsample_xyzi", "grid", "sift3d_scale_space", "sift3d_extrema", "sift3d_emit"), sift)
    print(f"keypoints {int(kp[0][-1])} ({int(kp[0][-1]) / n_obj:.1f} per object), mean octave sizes {kp[5].float().mean(0).tolist()}")

    def iss():
        ko, kx, ky, kz, _kc, src = capi.iss3d_keypoints(ctx, cloud, 0.1, 0.05)
        return [torch.as_tensor(ko.astype(np.int32)), kx, ky, kz, src]
    timed("iss3d_keypoints (0.1 / 0.05)", ("iss3d_saliency", "iss3d_nms"), iss)

    def voxel():
        ko, kx, ky, kz, _ = capi.voxel_keypoints(ctx, off, *t[:3], args.radius)
        return [torch.as_tensor(ko.astype(np.int32)), kx, ky, kz]
    timed(f"voxel_keypoints (leaf {args.radius})", ("voxel_keypoints",), voxel)
    ctx.timers_enable(False)
    cloud.close()
    ctx.close()


if __name__ == "__main__":
    main()

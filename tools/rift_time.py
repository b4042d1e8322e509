"""RIFT beside its siblings on the bench-sized coloured batch (256 objects x 16 384 points x 1024 keypoints, radius 0.4) -- the measurement
of DESIGN.md 4.19. Device events (the library timers) around single calls, median [min .. max] of --reps calls after --warmup warm-ups:
  "intensity_gradients" (k_rift_intensity + k_rift_gradient): the dense sweep, one thread per cloud point, 13 integer moments and a 3 x 3
                        eigen-solve per point
  "iss3d_saliency"      (k_iss_saliency) at the same radius: the sibling dense sweep, 6 integer moments and the same solve
  "rift"                (k_rift_gmax + k_rift): one wave per keypoint, 8 x 16 bins
  "cshot1344"           (k_shot<true>) on the same cloud, keypoints and radius: the sibling colour descriptor on the same balls
with the gather model of the RIFT kernel, sum_k M_k * (16 + 12) + K (12 + 512) bytes (M_k = candidates of the ball: the 16-byte position
record; its 12-byte gradient only for the points inside, counted for all; the centre, the row), and its share of the 8 TB/s HBM peak.

    python tools/rift_time.py [--objects 256] [--reps 20] [--warmup 3]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge   # noqa: E402
import bench                   # noqa: E402  (generate_batches: objects made by forked workers before the GPU is touched)

HBM_PEAK = 8e12


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, pipeline, synthetic = pkg.capi, pkg.pipeline, pkg.synthetic
    test = synthetic.Dataset(args.classes, args.objects, split=1, n_points=16384, n_keypoints=1024, with_color=True)
    pool = multiprocessing.get_context("fork").Pool(max(1, min(16, len(os.sched_getaffinity(0)))))
    host = bench.generate_batches(synthetic, [(test, list(range(args.objects)))], pool)
    pool.close(); pool.join()

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    b = pipeline.DeviceBatch(host[0], dev)
    base = pipeline.IsmConfig(n_classes=args.classes)
    radius = base.radius
    cloud = capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, min(radius, base.lrf_radius) * 0.4, rgba=b.rgba)
    kp = (b.kp_off, b.kx, b.ky, b.kz)
    lrf = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
    grad, pcnt = capi.intensity_gradients(ctx, cloud, radius, want_counts=True)
    rows, ball = capi.rift(ctx, cloud, *kp, radius, grad, want_counts=True)
    ctx.sync()
    mk, nkp, npts = float(ball.float().mean()), int(b.kp_off[-1]), int(b.pt_off[-1])
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints, radius {radius}: {float(pcnt.float().mean()):.0f} ball points per cloud point, "
          f"{mk:.0f} per keypoint; NaN gradients {int(torch.isnan(grad).any(1).sum())} of {npts}, NaN rows {int(torch.isnan(rows).any(1).sum())} of {nkp}")
    ctx.timers_enable(True)

    def timed(name, call):
        for _ in range(args.warmup):
            call()
        ctx.sync()
        ms = []
        for _ in range(args.reps):
            ctx.timers_reset()
            call()
            ctx.sync()
            ms.append(ctx.timer(name)[0])
        return ms

    tg = timed("intensity_gradients", lambda: capi.intensity_gradients(ctx, cloud, radius))
    ti = timed("iss3d_saliency", lambda: capi.iss3d_saliency(ctx, cloud, radius, want_eig=False, want_counts=False))
    tr = timed("rift", lambda: capi.rift(ctx, cloud, *kp, radius, grad))
    tc = timed("cshot1344", lambda: capi.cshot1344(ctx, cloud, *kp, b.kp_rgba, lrf, radius))
    ctx.timers_enable(False)
    model = nkp * (mk * 28 + 12 + 4 * capi.RIFT_DIM)
    rate = model / (np.median(tr) * 1e-3)
    print(f"intensity_gradients (k_rift_intensity + k_rift_gradient): {spread(tg)} ms per call")
    print(f"iss3d_saliency (k_iss_saliency), same radius:             {spread(ti)} ms per call; intensity_gradients / iss3d_saliency = "
          f"{np.median(tg) / np.median(ti):.2f}")
    print(f"rift (k_rift_gmax + k_rift), 8 x 16 bins:                 {spread(tr)} ms per call; model {model / 1e9:.2f} GB -> {rate / 1e9:.0f} GB/s, "
          f"{100 * rate / HBM_PEAK:.1f} % of the 8 TB/s peak")
    print(f"cshot1344 (k_shot<true>), same inputs:                    {spread(tc)} ms per call; rift / cshot1344 = {np.median(tr) / np.median(tc):.2f}")
    cloud.close()


if __name__ == "__main__":
    main()

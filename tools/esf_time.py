"""ESF_LOCAL beside SHOT-352 and FPFH-33 on the bench-sized batch (256 objects x 16 384 points x 1024 keypoints that are cloud points,
radius 0.4: the inputs of tools/rsd_time.py) -- the measurement of DESIGN.md 4.21. Device events (the library timers) around single
calls, median [min .. max] of --reps calls after 2 warm-ups:
  "esf_local" (k_esf_local):  640 floats per keypoint at the library's sample count and seed
  "shot352", "fpfh33":        the siblings on the same cloud, keypoints and radius
with the mean neighbour count n, the share of keypoints whose ball exceeds the LDS staging (read through the work list), and the
MODELLED work: the bins of the device's own counts give the samples per keypoint (A3 holds three sixths per sample); a line visits at
most 63 cells and a sample has three lines in the second pass, so samples x 3 x 63 bounds the voxel look-ups per call from above.

    python tools/esf_time.py [--objects 256] [--reps 20] [--samples 20000]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge   # noqa: E402
import bench                   # noqa: E402  (generate_batches: objects made by forked workers before the GPU is touched)

STAGED = 1024                  # ESF_CAP of esf.hip
LDS_BYTES = 51776              # static LDS of k_esf_local (modelled: the sum of its arrays)


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.4)
    ap.add_argument("--samples", type=int, default=0, help="0: the library's ISMHIP_ESF_SAMPLES")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, pipeline, synthetic = pkg.capi, pkg.pipeline, pkg.synthetic
    args.samples = args.samples or capi.ESF_SAMPLES
    test = synthetic.Dataset(args.classes, args.objects, split=1, n_points=16384, n_keypoints=1024)
    pool = multiprocessing.get_context("fork").Pool(max(1, min(16, len(os.sched_getaffinity(0)))))
    host = bench.generate_batches(synthetic, [(test, list(range(args.objects)))], pool)
    pool.close(); pool.join()
    nb = dict(host[0])
    rng = np.random.default_rng(7)
    po = np.asarray(nb["pt_off"], np.int64)
    pick = np.concatenate([po[o] + rng.choice(po[o + 1] - po[o], 1024, replace=False) for o in range(args.objects)])
    nb["kp"] = nb["xyz"][pick].copy()
    nb["kp_off"] = (np.arange(args.objects + 1) * 1024).astype(np.uint32)

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    b = pipeline.DeviceBatch(nb, dev)
    base = pipeline.IsmConfig(n_classes=args.classes)
    cell = min(args.radius, base.lrf_radius) * 0.4
    cloud = capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, cell)
    kp = (b.kp_off, b.kx, b.ky, b.kz)
    lrf = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
    rows, cnt, bins = capi.esf_local(ctx, cloud, *kp, args.radius, n_samples=args.samples, want_counts=True, want_bins=True)
    ctx.sync()
    n = cnt.cpu().numpy().astype(np.float64)
    samples = float(bins[:, :192].sum().item()) / 3.0
    nan_rows = int(torch.isnan(rows[:, 0]).sum().item())
    del rows, bins
    nkp = int(b.kp_off[-1])
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints (cloud points), radius {args.radius}, {args.samples} samples: mean n {n.mean():.0f} "
          f"(max {n.max():.0f}), {100 * (n > STAGED).mean():.1f} % of the balls above the {STAGED} staged points (measured), {nan_rows} NaN rows")
    print(f"samples per call {samples:.3e} (measured); at most {samples * 3 * 63:.3e} voxel look-ups per call (modelled: 3 lines of at most "
          f"63 cells); {LDS_BYTES} bytes of LDS per workgroup, 3 workgroups per CU (modelled)")
    ctx.timers_enable(True)

    def timed(name, call):
        for _ in range(2):
            call()
        ctx.sync()
        ms = []
        for _ in range(args.reps):
            ctx.timers_reset()
            call()
            ctx.sync()
            ms.append(ctx.timer(name)[0])
        return ms

    es = timed("esf_local", lambda: capi.esf_local(ctx, cloud, *kp, args.radius, n_samples=args.samples))
    t = np.median(es) * 1e-3
    print(f"esf_local (k_esf_local):       {spread(es)} ms per call (measured); {samples / t:.3e} samples/s (measured)")
    sh = timed("shot352", lambda: capi.shot352(ctx, cloud, *kp, lrf, args.radius))
    fp = timed("fpfh33", lambda: capi.fpfh33(ctx, cloud, *kp, args.radius))
    ctx.timers_enable(False)
    print(f"shot352, same inputs:          {spread(sh)} ms per call (measured)")
    print(f"fpfh33, same inputs:           {spread(fp)} ms per call (measured)")
    cloud.close()


if __name__ == "__main__":
    main()

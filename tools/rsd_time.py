"""RSD beside FPFH-33 and SHOT-352 on the bench-sized batch (256 objects x 16 384 points x 1024 keypoints that are cloud points, the
inputs and the radius of tools/spin_image_time.py) -- the measurement of DESIGN.md 4.16. Device events (the library timers) around
single calls, median [min .. max] of --reps calls after 2 warm-ups:
  "rsd"     (k_rsd<true>):  the 25-bin pair histogram
  "rsd"     (k_rsd<false>): the two principal radii
  "fpfh33", "shot352":      the siblings on the same cloud, keypoints and radius
with the mean neighbour count n, the pairs sum_k n_k (n_k - 1) / 2 per call and per second, and the VALU model: VALU_PER_PAIR vector
instructions per pair step of 64 lanes (counted in the compiled inner loop of the circular sweep, fast path) x pairs / the chip's lane
rate (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz), and the fraction of that model the measured time achieves.

    python tools/rsd_time.py [--objects 256] [--reps 5]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge   # noqa: E402
import bench                   # noqa: E402  (generate_batches: objects made by forked workers before the GPU is touched)

LANE_RATE = 256 * 4 * 16 * 2.4e9
VALU_PER_PAIR = {True: 85, False: 90}       # v_* instructions of one trip of the inner loop off the guard bands (histogram, radii)


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, pipeline, synthetic = pkg.capi, pkg.pipeline, pkg.synthetic
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
    cell = min(base.radius, base.lrf_radius) * 0.4
    cloud = capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, cell)
    kp = (b.kp_off, b.kx, b.ky, b.kz)
    lrf = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
    _, cnt = capi.rsd(ctx, cloud, *kp, base.radius, want_counts=True)
    ctx.sync()
    n = cnt.cpu().numpy().astype(np.float64)
    pairs, nkp = float((n * (n - 1) / 2).sum()), int(b.kp_off[-1])
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints (cloud points), radius {base.radius}: mean n {n.mean():.0f} "
          f"(max {n.max():.0f}), {pairs:.3e} pairs per call")
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

    for full, label in ((True, "rsd, histogram (k_rsd<true>): "), (False, "rsd, radii (k_rsd<false>):    ")):
        ms = timed("rsd", lambda: capi.rsd(ctx, cloud, *kp, base.radius, full_histogram=full))
        t = np.median(ms) * 1e-3
        model = VALU_PER_PAIR[full] * pairs / LANE_RATE
        print(f"{label}{spread(ms)} ms per call (measured); {pairs / t:.3e} pairs/s (measured); VALU model {VALU_PER_PAIR[full]} "
              f"instructions per pair -> {model * 1e3:.1f} ms (modelled), achieved {100 * model / t:.0f} % of the model")
    fp = timed("fpfh33", lambda: capi.fpfh33(ctx, cloud, *kp, base.radius))
    sh = timed("shot352", lambda: capi.shot352(ctx, cloud, *kp, lrf, base.radius))
    ctx.timers_enable(False)
    print(f"fpfh33, same inputs:           {spread(fp)} ms per call (measured)")
    print(f"shot352, same inputs:          {spread(sh)} ms per call (measured)")
    cloud.close()


if __name__ == "__main__":
    main()

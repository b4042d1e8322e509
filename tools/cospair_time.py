"""CoSPAIR beside CSHOT-1344 on the bench-sized coloured batch of short_cshot_time.py (16 384 points, 1024 keypoints per object; the same
cloud, keypoints and radius) -- the measurement of DESIGN.md 4.10. Device events (the library timers) around single calls, mean
[min .. max] of --reps calls after 3 warm-ups:
  "cospair" on a cloud that holds its colour codes already: k_cospair_snap + k_cospair
  "cospair" on a freshly created cloud: + k_cospair_codes (the difference is the colour-code build)
  "cospair" on the same geometry with ONE colour on every point: every colour deposit of a wave hits three counters per level -- the
      same-address worst case of the LDS counters, against the random colours above
  "cshot1344" (k_shot<true>) on the same inputs, the yardstick: both sweep the same balls
with the gather model sum_k M_k (16 + 16 + 2) + K (12 + 1512) bytes and its share of the 8 TB/s HBM peak. The split of "cospair" into
its kernels is read from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/cospair_time.py --reps 3).

    python tools/cospair_time.py [--objects 256] [--reps 5]
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
    return f"{v.mean():.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
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
    cell = min(base.radius, base.lrf_radius) * 0.4
    one_colour = torch.full_like(b.rgba, 0x336699)
    new_cloud = lambda rgba: capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, cell, rgba=rgba)
    cloud, uni = new_cloud(b.rgba), new_cloud(one_colour)
    kp = (b.kp_off, b.kx, b.ky, b.kz)
    lrf = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
    _, cnt = capi.cospair(ctx, cloud, *kp, base.radius, want_counts=True)
    _, ball = capi.shot352(ctx, cloud, *kp, lrf, base.radius, want_counts=True)
    mk, pairs, nkp = float(ball.float().mean()), float(cnt.float().mean()), int(b.kp_off[-1])
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints, radius {base.radius}, mean ball population M_k {mk:.0f}, mean CoSPAIR pairs {pairs:.0f}")
    ctx.timers_enable(True)

    def timed(name, call, before=None):
        for _ in range(3):
            if before:
                before()
            call()
        ctx.sync()
        ms = []
        for _ in range(args.reps):
            if before:
                before()
            ctx.sync()
            ctx.timers_reset()
            call()
            ctx.sync()
            ms.append(ctx.timer(name)[0])
        return ms

    fresh = {}

    def recreate():                                    # a destroyed cloud is recycled: its colour codes are built again by the next call
        if "c" in fresh:
            fresh["c"].close()
        fresh["c"] = new_cloud(b.rgba)

    warm = timed("cospair", lambda: capi.cospair(ctx, cloud, *kp, base.radius))
    cold = timed("cospair", lambda: capi.cospair(ctx, fresh["c"], *kp, base.radius), before=recreate)
    same = timed("cospair", lambda: capi.cospair(ctx, uni, *kp, base.radius))
    shot = timed("cshot1344", lambda: capi.cshot1344(ctx, cloud, *kp, b.kp_rgba, lrf, base.radius))
    ctx.timers_enable(False)
    model = nkp * (mk * 34 + 12 + 1512)
    cmodel = nkp * (mk * 28 + 52 + 4 * 1344)
    rate, crate = model / (np.mean(warm) * 1e-3), cmodel / (np.mean(shot) * 1e-3)
    print(f"cospair, codes cached (k_cospair_snap + k_cospair): {spread(warm)} ms per call; model {model / 1e9:.2f} GB -> {rate / 1e9:.0f} GB/s, "
          f"{100 * rate / HBM_PEAK:.1f} % of the 8 TB/s peak")
    print(f"cospair on a fresh cloud (+ k_cospair_codes):        {spread(cold)} ms per call; colour-code build {np.mean(cold) - np.mean(warm):.3f} ms")
    print(f"cospair, ONE colour on every point:                  {spread(same)} ms per call ({np.mean(same) / np.mean(warm):.3f} x the random colours)")
    print(f"cshot1344 (k_shot<true>), same inputs:               {spread(shot)} ms per call; model {cmodel / 1e9:.2f} GB -> {crate / 1e9:.0f} GB/s, "
          f"{100 * crate / HBM_PEAK:.1f} % of the 8 TB/s peak; cospair / cshot1344 = {np.mean(warm) / np.mean(shot):.2f}")
    for c in (cloud, uni, fresh["c"]):
        c.close()


if __name__ == "__main__":
    main()

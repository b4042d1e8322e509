"""SpinImage beside SHOT-352 on the bench-sized batch (256 objects x 16 384 points x 1024 keypoints; the keypoints are CLOUD POINTS, as
ISS3D's are, so that every keypoint finds its normal) -- the measurement of DESIGN.md 4.15. Device events (the library timers) around
single calls, median [min .. max] of --reps calls after 3 warm-ups:
  "keypoint_normals" (k_keypoint_normals): the lookup of the keypoints' normals, one thread per keypoint on the keypoint's own cell
  "spin_image"       (k_spin_image):       the descriptor about those normals, image width 8 (153 floats)
  "shot352"          (k_shot<false>)       on the same cloud, keypoints and radius, the sibling: both sweep the same balls
with the gather model sum_k M_k * 16 + K (24 + 612) bytes of the spin image and its share of the 8 TB/s HBM peak.

    python tools/spin_image_time.py [--objects 256] [--reps 20]
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
    ax, ay, az, idx = capi.keypoint_normals(ctx, cloud, *kp, want_index=True)
    _, ball = capi.spin_image(ctx, cloud, *kp, ax, ay, az, base.radius, want_counts=True)
    ctx.sync()
    mk, nkp = float(ball.float().mean()), int(b.kp_off[-1])
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints (cloud points; {int((idx >= 0).sum())} found their normal), radius {base.radius}, "
          f"mean ball population M_k {mk:.0f}")
    ctx.timers_enable(True)

    def timed(name, call):
        for _ in range(3):
            call()
        ctx.sync()
        ms = []
        for _ in range(args.reps):
            ctx.timers_reset()
            call()
            ctx.sync()
            ms.append(ctx.timer(name)[0])
        return ms

    look = timed("keypoint_normals", lambda: capi.keypoint_normals(ctx, cloud, *kp))
    spin = timed("spin_image", lambda: capi.spin_image(ctx, cloud, *kp, ax, ay, az, base.radius))
    shot = timed("shot352", lambda: capi.shot352(ctx, cloud, *kp, lrf, base.radius))
    ctx.timers_enable(False)
    model = nkp * (mk * 16 + 24 + 4 * capi.SPIN_IMAGE_DIM)
    smodel = nkp * (mk * 24 + 48 + 4 * 352)
    rate, srate = model / (np.median(spin) * 1e-3), smodel / (np.median(shot) * 1e-3)
    print(f"keypoint_normals (k_keypoint_normals): {spread(look)} ms per call")
    print(f"spin_image (k_spin_image), width 8:    {spread(spin)} ms per call; model {model / 1e9:.2f} GB -> {rate / 1e9:.0f} GB/s, "
          f"{100 * rate / HBM_PEAK:.1f} % of the 8 TB/s peak")
    print(f"shot352 (k_shot<false>), same inputs:  {spread(shot)} ms per call; model {smodel / 1e9:.2f} GB -> {srate / 1e9:.0f} GB/s, "
          f"{100 * srate / HBM_PEAK:.1f} % of the 8 TB/s peak; spin_image / shot352 = {np.median(spin) / np.median(shot):.2f}")
    cloud.close()


if __name__ == "__main__":
    main()

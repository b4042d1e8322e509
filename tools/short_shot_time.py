"""SHORT_SHOT beside SHOT-352 on one bench-sized batch (16 384 points, 1024 keypoints per object) -- the measurement of DESIGN.md's
SHORT_SHOT subsection. Per kernel: the library timer ("short_shot" at 32 and 256 bins, "shot352") of single launches on the same
cloud, keypoints, frames and radius, after warm-up, as median [min .. max] over --reps launches, with the bytes-per-keypoint model
M_k * 16 + 48 + 4 D (SHOT: M_k * 24 + 48 + 4 * 352). End to end: the detection step of pipeline.py (features -> kNN -> votes -> maxima)
with feature SHOT and SHORT_SHOT (32 bins) on codebooks of one word per training feature, wall clock around a device synchronise,
and the library timers of one more step (the parts of "knn" are listed after it).

    python tools/short_shot_time.py [--objects 256] [--train-per-class 10] [--reps 10] [--no-e2e]
"""
import argparse
import multiprocessing
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge   # noqa: E402
import bench                   # noqa: E402  (generate_batches: objects made by forked workers before the GPU is touched)


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return f"{np.median(v):.3f} [{v[0]:.3f} .. {v[-1]:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--train-per-class", type=int, default=10)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, pipeline, synthetic = pkg.capi, pkg.pipeline, pkg.synthetic
    C, n_train = args.classes, args.classes * args.train_per_class
    test = synthetic.Dataset(C, args.objects, split=1, n_points=16384, n_keypoints=1024)
    train = synthetic.Dataset(C, n_train, split=0, n_points=16384, n_keypoints=1024)
    order = sorted(range(n_train), key=lambda i: (train.label(i), i))
    pool = multiprocessing.get_context("fork").Pool(max(1, min(16, len(os.sched_getaffinity(0)))))
    jobs = [(test, list(range(args.objects)))] + ([] if args.no_e2e else [(train, order[s:s + 32]) for s in range(0, n_train, 32)])
    host = bench.generate_batches(synthetic, jobs, pool)
    pool.close(); pool.join()

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    b = pipeline.DeviceBatch(host[0], dev)
    base = pipeline.IsmConfig(n_classes=C)
    cell = min(base.radius, base.lrf_radius) * 0.4
    cloud = capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, cell)
    kp = (b.kp_off, b.kx, b.ky, b.kz)
    lrf = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
    _, cnt = capi.shot352(ctx, cloud, *kp, lrf, base.radius, want_counts=True)
    mk = float(cnt.float().mean())
    nkp = int(b.kp_off[-1])
    kernels = [("shot352", 352, 24, lambda: capi.shot352(ctx, cloud, *kp, lrf, base.radius)),
               ("short_shot", 32, 16, lambda: capi.short_shot(ctx, cloud, *kp, lrf, base.radius, bins=(2, 2, 8))),
               ("short_shot", 256, 16, lambda: capi.short_shot(ctx, cloud, *kp, lrf, base.radius, bins=(8, 4, 8)))]
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints, radius {base.radius}, mean neighbours M_k {mk:.0f}")
    ctx.timers_enable(True)
    for name, dim, per_nb, call in kernels:
        for _ in range(3):
            call()
        ctx.sync()
        ms = []
        for _ in range(args.reps):
            ctx.timers_reset()
            call()
            ctx.sync()
            ms.append(ctx.timer(name)[0])
        model = nkp * (mk * per_nb + 48 + 4 * dim)
        print(f"{name} D={dim}: {spread(ms)} ms per launch; model {model / 1e9:.2f} GB -> {model / 1e6 / np.median(ms):.0f} GB/s at the median")
    ctx.timers_enable(False)
    cloud.close()
    if args.no_e2e:
        return
    tb = [pipeline.DeviceBatch(h, dev) for h in host[1:]]
    for kw in (dict(feature="SHOT"), dict(feature="SHORT_SHOT", short_shot_dims=32)):
        rec = pipeline.Recognizer(capi.Ctx(0), pipeline.IsmConfig(k=1, n_classes=C, max_maxima=16, **kw))
        cb = rec.train(tb)
        for _ in range(2):
            out = rec.detect(b)
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(3, args.reps // 2)):
            t0 = time.perf_counter()
            out = rec.detect(b)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        acc = float((out["class_score"].argmax(1).cpu().numpy() == host[0]["labels"]).mean())
        rec.ctx.timers_enable(True); rec.ctx.timers_reset()          # where one step's device time goes
        rec.detect(b)
        rec.ctx.sync()
        parts = {n: rec.ctx.timer(n)[0] for n in ("grid", "lrf", "shot352", "short_shot", "knn", "knn_rotate", "knn_stage2", "knn_rerank", "knn_fallback", "cast_votes", "maxima")}
        counters = {n: int(rec.ctx.timer(n)[0]) for n in ("knn_stage2_queries", "knn_flagged_queries", "knn_pca_launches")}
        rec.ctx.timers_enable(False)
        print("  device ms: " + ", ".join(f"{n} {v:.2f}" for n, v in parts.items() if v > 0) + "; " + ", ".join(f"{n} {v}" for n, v in counters.items()))
        print(f"detect step, feature {kw['feature']} (dim {rec.cfg.dim}, {cb['words'].shape[0]} words): {spread(ms)} ms per {args.objects} objects; "
              f"top-1 on the synthetic split {acc:.3f}")


if __name__ == "__main__":
    main()

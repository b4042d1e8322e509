"""USC beside SHOT-352 and CSHOT-1344 on the bench-sized batch (256 objects x 16 384 points x 1024 keypoints that are cloud points), and
the codeword search of its 1960-float rows beside the same call at 1344 floats -- the measurement of DESIGN.md 4.26. Device events (the
library timers) around single calls, median [min .. max] of --reps calls after 2 warm-ups:
  "point_density" (k_point_density): the density of every cloud point at USC_POINT_DENSITY_RADIUS, once per cloud
  "usc"           (k_usc):           the descriptor in SHOT frames at Radius - 0.1, minimal radius Radius / 10 (1960 floats)
  "shot352", "cshot1344"             on the same cloud, keypoints and radius: the siblings sweep the same balls
  "knn"                              --knn-queries of those rows against --words of them as the codebook (the exact wide scan), and
                                     the same call on CSHOT-1344 rows and words (the three-stage search): squared L2, K = 1,
                                     --knn-reps calls each

    python tools/usc_time.py [--objects 256] [--reps 20] [--words 10000] [--knn-queries 16384] [--knn-reps 20]

The exact wide scan reads every codeword row for every query: a call with all 262 144 rows as queries against 10 000 words takes whole
seconds, 22 of them minutes. The default therefore searches the first 16 384 rows (64 query tiles, still above the sizes at which the
1344-float search goes to the matrix cores), for both row lengths; --knn-queries 262144 measures the whole batch (size the time limit
of the run by the per-query figure the default prints).
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge   # noqa: E402
import bench                   # noqa: E402  (generate_batches: objects made by forked workers before the GPU is touched)


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--words", type=int, default=10000)
    ap.add_argument("--knn-queries", type=int, default=16384)
    ap.add_argument("--knn-reps", type=int, default=20)
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, pipeline, synthetic = pkg.capi, pkg.pipeline, pkg.synthetic
    test = synthetic.Dataset(args.classes, args.objects, split=1, n_points=16384, n_keypoints=1024, with_color=True)
    pool = multiprocessing.get_context("fork").Pool(max(1, min(16, len(os.sched_getaffinity(0)))))
    host = bench.generate_batches(synthetic, [(test, list(range(args.objects)))], pool)
    pool.close(); pool.join()
    nb = dict(host[0])
    rng = np.random.default_rng(7)
    po = np.asarray(nb["pt_off"], np.int64)
    pick = np.concatenate([po[o] + rng.choice(po[o + 1] - po[o], 1024, replace=False) for o in range(args.objects)])
    nb["kp"] = nb["xyz"][pick].copy()
    nb["kp_rgba"] = nb["rgba"][pick].copy()
    nb["kp_off"] = (np.arange(args.objects + 1) * 1024).astype(np.uint32)

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    b = pipeline.DeviceBatch(nb, dev)
    base = pipeline.IsmConfig(n_classes=args.classes)
    R = base.radius
    cell = min(R, base.lrf_radius) * 0.4
    cloud = capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, cell, rgba=b.rgba)
    kp = (b.kp_off, b.kx, b.ky, b.kz)
    lrf = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
    usc_lrf = capi.shot_lrf(ctx, cloud, *kp, 0.1 if R <= 0.1 else R - 0.1)
    dens = capi.point_density(ctx, cloud, capi.USC_POINT_DENSITY_RADIUS)
    rows, ball = capi.usc(ctx, cloud, *kp, usc_lrf, R, R / 10.0, dens, want_counts=True)
    ctx.sync()
    mk, nkp = float(ball.float().mean()), int(b.kp_off[-1])
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints (cloud points), radius {R}, mean ball population M_k {mk:.0f}, "
          f"density at {capi.USC_POINT_DENSITY_RADIUS}: mean {float(dens.float().mean()):.1f}, max {int(dens.max())}")
    ctx.timers_enable(True)

    def timed(name, call, reps):
        for _ in range(2):
            call()
        ctx.sync()
        ms = []
        for _ in range(reps):
            ctx.timers_reset()
            call()
            ctx.sync()
            ms.append(ctx.timer(name)[0])
        return ms

    den = timed("point_density", lambda: capi.point_density(ctx, cloud, capi.USC_POINT_DENSITY_RADIUS), args.reps)
    usc = timed("usc", lambda: capi.usc(ctx, cloud, *kp, usc_lrf, R, R / 10.0, dens), args.reps)
    shot = timed("shot352", lambda: capi.shot352(ctx, cloud, *kp, lrf, R), args.reps)
    cshot = timed("cshot1344", lambda: capi.cshot1344(ctx, cloud, *kp, b.kp_rgba, lrf, R), args.reps)
    model = nkp * (mk * 36 + 64 + 4 * capi.USC_DIM)
    print(f"point_density (k_point_density):      {spread(den)} ms per call")
    print(f"usc (k_usc), 1960 floats:             {spread(usc)} ms per call; gather model {model / 1e9:.2f} GB -> {model / (np.median(usc) * 1e-3) / 1e9:.0f} GB/s")
    print(f"shot352 (k_shot<false>), same inputs: {spread(shot)} ms per call; usc / shot352 = {np.median(usc) / np.median(shot):.2f}")
    print(f"cshot1344 (k_shot<true>), same inputs: {spread(cshot)} ms per call; usc / cshot1344 = {np.median(usc) / np.median(cshot):.2f}")

    def search(name, feats):
        ok = ~torch.isnan(feats[:, 0])
        feats = feats[ok]
        nw, nq = min(args.words, feats.shape[0]), min(args.knn_queries, feats.shape[0])
        words = feats[torch.linspace(0, feats.shape[0] - 1, nw, device=dev).long()].cpu().numpy()
        cb = capi.Codebook(ctx, words, np.arange(nw + 1, dtype=np.uint32), np.zeros((nw, 3), np.float32), np.zeros(nw, np.uint32), np.zeros(nw, np.uint32), 1,
                           np.ones(1, np.float32))
        q = feats[:nq].contiguous()
        ms = timed("knn", lambda: capi.knn(ctx, cb, capi.METRIC_L2SQ, q, 1), args.knn_reps)
        print(f"knn, {name}: {nq} queries x {nw} words x {feats.shape[1]} floats, squared L2, K = 1: {spread(ms)} ms per call, "
              f"{1e3 * np.median(ms) / nq:.3f} us per query")
        cb.close()
        return np.median(ms)

    if args.knn_reps > 0:
        t_usc = search("USC rows (exact wide scan, knn_wide.hip)", rows)
        crow = capi.cshot1344(ctx, cloud, *kp, b.kp_rgba, lrf, R)
        t_cs = search("CSHOT-1344 rows (three-stage search)", crow)
        print(f"knn at 1960 / knn at 1344 = {t_usc / t_cs:.1f}")
    ctx.timers_enable(False)
    cloud.close()


if __name__ == "__main__":
    main()

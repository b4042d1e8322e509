"""The exact binary search beside the float search on B-SHOT rows -- the measurement of DESIGN.md 4.11 that decides the host's route.
Queries: the BSHOT rows of --objects bench-sized objects (16 384 points, 1 024 keypoints each; 256 objects = 262 144 queries). Codebook:
the BSHOT rows of --words / 1024 objects of a disjoint split (102 400 words). K = 1. On the same buffers in the same process, device
events (the library timers), 3 warm-ups, then --reps interleaved repetitions of
  ismhip_knn_binary                 timer "knn_binary" (packing the queries, k_knn_binary, the merge)
  ismhip_knn, ISMHIP_METRIC_L2SQ    timer "knn"
  ismhip_knn, ISMHIP_METRIC_CHI2    timer "knn"
reported as median [min .. max]; the three answers are compared bit for bit first. The route stays on for a metric only if the binary
search's maximum is below the float search's minimum. Also "bshot" (the binarisation kernel) beside "shot352" for one ismhip_bshot352.
Integer operations issued = 2 x padded queries x padded words x padded dim, against the 8-bit matrix-core peak (2 x the 2.5 PF of
bf16, dense).

    python tools/bshot_time.py [--objects 256] [--words 102400] [--reps 5]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge   # noqa: E402
import bench                   # noqa: E402  (generate_batches: objects made by forked workers before the GPU is touched)

I8_PEAK = 5.0e15


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--words", type=int, default=102400)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, pipeline, synthetic = pkg.capi, pkg.pipeline, pkg.synthetic
    n_train = (args.words + 1023) // 1024
    test = synthetic.Dataset(args.classes, args.objects, split=1, n_points=16384, n_keypoints=1024)
    train = synthetic.Dataset(args.classes, n_train, split=0, n_points=16384, n_keypoints=1024)
    pool = multiprocessing.get_context("fork").Pool(max(1, min(16, len(os.sched_getaffinity(0)))))
    host = bench.generate_batches(synthetic, [(test, list(range(args.objects))), (train, list(range(n_train)))], pool)
    pool.close(); pool.join()

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    base = pipeline.IsmConfig(n_classes=args.classes)
    cell = min(base.radius, base.lrf_radius) * 0.4

    def rows_of(np_batch, timed=False):
        b = pipeline.DeviceBatch(np_batch, dev)
        cloud = capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, cell)
        kp = (b.kp_off, b.kx, b.ky, b.kz)
        lrf = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
        rows = capi.bshot352(ctx, cloud, *kp, lrf, base.radius)
        ms = None
        if timed:
            ctx.timers_enable(True)
            ms = {"shot352": [], "bshot": []}
            for i in range(3 + args.reps):
                ctx.sync(); ctx.timers_reset()
                capi.bshot352(ctx, cloud, *kp, lrf, base.radius)
                ctx.sync()
                if i >= 3:
                    for name in ms:
                        ms[name].append(ctx.timer(name)[0])
            ctx.timers_enable(False)
        ctx.sync()
        cloud.close()
        return rows, ms

    q, front = rows_of(host[0], timed=True)
    words = rows_of(host[1])[0][:args.words].cpu().numpy()
    nq, n_words, dim = q.shape[0], len(words), q.shape[1]
    ones = float(q.mean())
    print(f"{nq} queries, {n_words} words, dim {dim}; share of ones in the query rows {ones:.3f}; rows of 352 ones (NaN SHOT rows): "
          f"{int((q.sum(1) == dim).sum())}")
    print(f"ismhip_bshot352 on {nq} keypoints: shot352 {spread(front['shot352'])} ms, bshot {spread(front['bshot'])} ms per call")
    off = np.arange(n_words + 1, dtype=np.uint32)
    cb = capi.Codebook(ctx, words, off, np.zeros((n_words, 3), np.float32), np.zeros(n_words, np.uint32), np.zeros(n_words, np.uint32),
                       args.classes, np.ones(args.classes, np.float32))
    cb.make_binary()

    calls = {"knn_binary": ("knn_binary", lambda: capi.knn_binary(ctx, cb, q, 1)),
             "knn L2SQ": ("knn", lambda: capi.knn(ctx, cb, capi.METRIC_L2SQ, q, 1)),
             "knn CHI2": ("knn", lambda: capi.knn(ctx, cb, capi.METRIC_CHI2, q, 1))}
    out = {k: c[1]() for k, c in calls.items()}
    ctx.sync()
    for k in ("knn L2SQ", "knn CHI2"):
        same = torch.equal(out[k][0], out["knn_binary"][0]) and torch.equal(out[k][1].view(torch.int32), out["knn_binary"][1].view(torch.int32))
        print(f"{k}: idx and dist bit-equal to knn_binary: {same}")
        assert same
    ctx.timers_enable(True)
    for _ in range(3):
        for name, call in calls.values():
            call()
    ctx.sync()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):                                     # interleaved: one call of each per repetition
        for k, (name, call) in calls.items():
            ctx.sync(); ctx.timers_reset()
            call()
            ctx.sync()
            ms[k].append(ctx.timer(name)[0])
    ctx.timers_enable(False)
    pad = lambda n, m: (n + m - 1) // m * m
    ops = 2.0 * pad(nq, 128) * pad(n_words, 128) * pad(dim, 128)
    b = np.asarray(ms["knn_binary"])
    print(f"knn_binary: {spread(b)} ms per call; {ops / 1e12:.2f} T integer operations issued -> {ops / (np.median(b) * 1e-3) / 1e15:.3f} P/s, "
          f"{100 * ops / (np.median(b) * 1e-3) / I8_PEAK:.1f} % of the 5 P/s 8-bit peak")
    for k in ("knn L2SQ", "knn CHI2"):
        f = np.asarray(ms[k])
        on = b.max() < f.min()
        print(f"{k}:   {spread(f)} ms per call; float median / binary median = {np.median(f) / np.median(b):.2f}; "
              f"binary max {b.max():.3f} {'<' if on else '>='} float min {f.min():.3f} -> route {'ON' if on else 'OFF'}")
    cb.close()


if __name__ == "__main__":
    main()

"""Feature ranking on the device -- the measurement of DESIGN.md 4.12.
Workload: --rows SHOT-like rows (non-negative, sparse, unit L2 norm, 352 floats; every class scatters around its own prototype) in
--classes equal classes, KSearch 10. On the same buffers in the same process, device events (the library timers), one warm-up, then
--reps repetitions of, per ranking type,
  ismhip_rank_scores     timer "rank_scores" (search-only codebooks, the searches, the score kernels), and of it the timers "knn" /
                         "knn_large_k" of the searches it issued; the rest is codebook construction and the score kernels, the
                         latter under the timer "rank_score_kernels"
  ismhip_rank_select     timer "rank_select"
and of the bare searches the types issue, on codebooks built once outside the timed region:
  all rows in all rows, K = KSearch + 1           (KNNActivation, Incremental)
  all rows in every class's rows, K = KSearch     (Strangeness, NaiveBayes: --classes searches)
reported as median [min .. max] milliseconds. The scores of the two runs of a type are compared bit for bit.

    python tools/rank_time.py [--rows 262144] [--classes 10] [--k-search 10] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge   # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.2f} [{v.min():.2f} .. {v.max():.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--dim", type=int, default=352)
    ap.add_argument("--k-search", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    capi = ge.load_package().capi

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    n, C_, dim, ks = args.rows, args.classes, args.dim, args.k_search
    off = np.asarray([n * c // C_ for c in range(C_ + 1)], np.uint32)
    g = torch.Generator(device=dev); g.manual_seed(7)
    cls = torch.bucketize(torch.arange(n, device=dev), torch.as_tensor(off[1:].astype(np.int64), device=dev), right=True)
    proto = torch.rand((C_, dim), generator=g, device=dev) ** 3 * (torch.rand((C_, dim), generator=g, device=dev) < 0.5)
    desc = torch.rand((n, dim), generator=g, device=dev) ** 3 * (torch.rand((n, dim), generator=g, device=dev) < 0.6)
    desc = 0.5 * proto[cls] + 0.5 * desc
    desc = (desc / desc.norm(dim=1, keepdim=True).clamp_min(1e-12)).contiguous()
    print(f"{n} rows of {dim} floats in {C_} classes, KSearch {ks}")

    ctx.timers_enable(True)
    names = ("rank_scores", "knn", "knn_large_k", "rank_score_kernels", "rank_select")
    for rank_type in capi.RANK_TYPES:
        ms = {k: [] for k in names}; wall = []; first = None
        for rep in range(1 + args.reps):
            ctx.sync(); ctx.timers_reset()
            t0 = time.perf_counter()
            score = capi.rank_scores(ctx, rank_type, desc, off, ks, 0.25, 2)
            ctx.sync()
            t1 = time.perf_counter()
            keep, n_keep = capi.rank_select(ctx, score, off, 0.75, 0.0)
            ctx.sync()
            if first is None:
                first = score.clone()
            assert torch.equal(first.view(torch.int32), score.view(torch.int32)), "scores differ between two runs"
            if rep >= 1:
                wall.append((t1 - t0) * 1e3)
                for k in names:
                    ms[k].append(ctx.timer(k)[0])
        search = np.asarray(ms["knn"]) + np.asarray(ms["knn_large_k"])
        print(f"{rank_type}: rank_scores {spread(ms['rank_scores'])} ms (host wall {spread(wall)}), searches inside {spread(search)}, "
              f"rest {spread(np.asarray(ms['rank_scores']) - search)} of which the score kernels {spread(ms['rank_score_kernels'])}; rank_select {spread(ms['rank_select'])} ms; kept {int(n_keep.sum())} of {n}")

    # the bare searches, on codebooks built outside the timed region
    def codebook(rows):
        m = rows.shape[0]
        return capi.Codebook(ctx, rows.cpu().numpy(), np.arange(m + 1, dtype=np.uint32), np.zeros((m, 3), np.float32), np.zeros(m, np.uint32),
                             np.zeros(m, np.uint32), 1, np.ones(1, np.float32))
    cb_all = codebook(desc)
    cbs = [codebook(desc[int(off[c]):int(off[c + 1])]) for c in range(C_)]
    bare = {"all in all, K = KSearch + 1": lambda: capi.knn_large_k(ctx, cb_all, capi.METRIC_CHI2, desc, ks + 1),
            f"all in each of {C_} classes, K = KSearch": lambda: [capi.knn_large_k(ctx, cb, capi.METRIC_CHI2, desc, ks) for cb in cbs]}
    for label, call in bare.items():
        t = []
        for rep in range(1 + args.reps):
            ctx.sync(); ctx.timers_reset()
            call()
            ctx.sync()
            if rep >= 1:
                t.append(ctx.timer("knn")[0] + ctx.timer("knn_large_k")[0])
        print(f"bare kNN, {label}: {spread(t)} ms")
    ctx.timers_enable(False)
    for cb in [cb_all] + cbs:
        cb.close()


if __name__ == "__main__":
    main()

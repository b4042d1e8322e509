"""Timing of ismhip_knn_large_k on the MI355X: the fast path (certified threshold on the matrix cores) and the exact
scan alone (ISMHIP_KNN_LARGE_K_FAST=1 vs ISMHIP_KNN_LARGE_K_EXACT=1, a fresh ctx each), with the parts (seed, sweep, eval, exact) and the query counters.
usage: python tools/large_k_time.py [--data shot|manifold --words 102400 --nq 65536 --dim 352 --ks 32,64,256 --chi-words 8192 --chi-nq 4096 --chi-dim 1344]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--words", type=int, default=102400)
ap.add_argument("--nq", type=int, default=65536)
ap.add_argument("--dim", type=int, default=352)
ap.add_argument("--ks", default="32,64,256")
ap.add_argument("--chi-words", type=int, default=8192)
ap.add_argument("--chi-nq", type=int, default=4096)
ap.add_argument("--chi-dim", type=int, default=1344)
ap.add_argument("--skip-exact", action="store_true")
ap.add_argument("--data", default="shot", choices=["shot", "manifold"],
                help="shot: SHOT-352 descriptors of the bench generator (training split -> words, test split -> queries); manifold: synthetic rows")
ap.add_argument("--train-objects", type=int, default=100)
args = ap.parse_args()
import torch
pkg = ge.load_package()
capi = pkg.capi
dev = torch.device("cuda:0")


def manifold(rng, n, dim, intrinsic=8, unit=True):
    """rows on a low-dimensional non-negative manifold (distances spread with rank as descriptor distances do)"""
    A = np.random.default_rng(0).random((intrinsic, dim)).astype(np.float32)
    x = rng.random((n, intrinsic)).astype(np.float32) @ A + 1e-3 * rng.random((n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True) if unit else x.sum(axis=1, keepdims=True)
    return x.astype(np.float32)


def run(words, q, metric, k, exact):
    os.environ["ISMHIP_KNN_LARGE_K_EXACT" if exact else "ISMHIP_KNN_LARGE_K_FAST"] = "1"
    ctx = capi.Ctx(0)
    os.environ.pop("ISMHIP_KNN_LARGE_K_EXACT", None); os.environ.pop("ISMHIP_KNN_LARGE_K_FAST", None)
    n = len(words)
    cb = capi.Codebook(ctx, words, np.arange(n + 1, dtype=np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32),
                       np.zeros(n, np.uint32), 1, np.ones(1, np.float32))
    qd = torch.as_tensor(q).to(dev)
    capi.knn_large_k(ctx, cb, metric, qd[:2048], k)                  # warm-up (code objects, scratch)
    ctx.timers_enable(True); ctx.timers_reset()
    t0 = time.time()
    idx, dist = capi.knn_large_k(ctx, cb, metric, qd, k)
    wall = (time.time() - t0) * 1e3
    parts = {p: ctx.timer("knn_large_k" + p)[0] for p in ("", "_seed", "_sweep", "_eval", "_exact")}
    cnt = {c: int(ctx.timer(f"knn_large_k_{c}_queries")[0]) for c in ("certified", "retry", "exact")}
    print(f"metric={metric} words={n} nq={len(q)} dim={q.shape[1]} k={k} {'EXACT' if exact else 'fast '}: total {parts['']:.1f} ms (wall {wall:.0f}) "
          f"seed {parts['_seed']:.1f} sweep {parts['_sweep']:.1f} eval {parts['_eval']:.1f} exact {parts['_exact']:.1f} | {cnt}", flush=True)
    return idx.cpu().numpy(), dist.cpu().numpy()


def shot_descriptors(split, n_obj):
    """SHOT-352 of the bench's synthetic objects (headline config: 16384 points, 1024 keypoints, Radius 0.4, LRF 0.3), on the GPU"""
    ds = pkg.synthetic.Dataset(10, n_obj, split=split, n_points=16384, n_keypoints=1024)
    rec = pkg.pipeline.Recognizer(capi.Ctx(0), pkg.pipeline.IsmConfig())
    out = []
    for s in range(0, n_obj, 16):
        f = rec.compute_features(pkg.pipeline.DeviceBatch(ds.batch(range(s, min(n_obj, s + 16))), dev))
        out.append(f["desc"].cpu().numpy())
    return np.ascontiguousarray(np.concatenate(out))


rng = np.random.default_rng(1)
if args.data == "shot":
    W = shot_descriptors(0, args.train_objects)[:args.words]
    Q = shot_descriptors(1, (args.nq + 1023) // 1024 + 2)[:args.nq]
else:
    W = manifold(rng, args.words, args.dim)
    Q = manifold(rng, args.nq, args.dim)
for k in [int(x) for x in args.ks.split(",")]:
    a = run(W, Q, 0, k, False)
    if not args.skip_exact:
        b = run(W, Q, 0, k, True)
        print("  identical:", np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), flush=True)
if args.chi_nq:
    Wc = manifold(rng, args.chi_words, args.chi_dim, unit=False)
    Qc = manifold(rng, args.chi_nq, args.chi_dim, unit=False)
    a = run(Wc, Qc, 1, 32, False)
    if not args.skip_exact:
        b = run(Wc, Qc, 1, 32, True)
        print("  identical:", np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), flush=True)

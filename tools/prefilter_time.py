"""Timing of the point-cloud pre-filters on the MI355X: the "filter_sor", "filter_ror" and "filter_compact" timers on
the batch of bench config 1 (908 objects x 16384 surface points) with 3 % uniform outliers in the cube +-1.2 added to every object,
next to the "grid" and "lrf" timers of the same batch (1024 keypoints per object, ReferenceFrameRadius 0.3): the existing kernels
that do the same kind of sweep over the same search surface.
usage: python tools/prefilter_time.py [--objects 908 --points 16384 --mean-k 20 --stddev-mul 2.0 --radius 0.05 --min-neighbors 10 --cell 0.12 --reps 3]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=908)
ap.add_argument("--points", type=int, default=16384)
ap.add_argument("--outliers", type=float, default=0.03)
ap.add_argument("--mean-k", type=int, default=20)
ap.add_argument("--stddev-mul", type=float, default=2.0)
ap.add_argument("--radius", type=float, default=0.05)
ap.add_argument("--min-neighbors", type=int, default=10)
ap.add_argument("--cell", type=float, default=0.12, help="cell_size of the search surface (bench config 1: 0.4 * ReferenceFrameRadius 0.3)")
ap.add_argument("--lrf-radius", type=float, default=0.3)
ap.add_argument("--keypoints", type=int, default=1024)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
import torch
pkg = ge.load_package()
capi, syn = pkg.capi, pkg.synthetic
dev = torch.device("cuda:0")

t0 = time.time()
rng = np.random.default_rng(7)
n_out = int(args.outliers * args.points)
xyz, nrm, kp, po, ko = [], [], [], [0], [0]
for i in range(args.objects):
    p, n = syn.make_object(i % 10, 1, i, n_points=args.points)
    out = rng.uniform(-1.2, 1.2, size=(n_out, 3)).astype(np.float32)
    xyz.append(p); xyz.append(out); nrm.append(n); nrm.append(np.zeros_like(out)); nrm[-1][:, 2] = 1.0
    kp.append(p[:args.keypoints])                                  # surface points as keypoints: the yardstick needs their number, not their choice
    po.append(po[-1] + len(p) + n_out); ko.append(ko[-1] + len(kp[-1]))
xyz, nrm, kp = np.concatenate(xyz), np.concatenate(nrm), np.concatenate(kp)
po, ko = np.asarray(po, np.uint32), np.asarray(ko, np.uint32)
print(f"batch: {args.objects} objects, {len(xyz)} points ({n_out} outliers each), {len(kp)} keypoints, generated in {time.time() - t0:.1f} s", flush=True)
T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
pts = [T(xyz[:, i]) for i in range(3)] + [T(nrm[:, i]) for i in range(3)]
kps = [T(kp[:, i]) for i in range(3)]
ctx = capi.Ctx(0)


def once():
    cloud = capi.Cloud(ctx, po, *pts, args.cell)
    capi.shot_lrf(ctx, cloud, ko, *kps, args.lrf_radius)
    keep, _, thr = capi.filter_statistical(ctx, cloud, args.mean_k, args.stddev_mul, want_mean_dist=False)
    keep_r, _ = capi.filter_radius(ctx, cloud, args.radius, args.min_neighbors)
    new_off = capi.compact_points(ctx, po, keep, *pts)[0]
    ctx.sync()
    cloud.close()
    return keep, keep_r, new_off


once()                                                             # warm-up: code objects, scratch, the cloud pool
ctx.timers_enable(True)
for rep in range(args.reps):
    ctx.timers_reset()
    keep, keep_r, new_off = once()
    t = {n: ctx.timer(n)[0] for n in ("grid", "lrf", "filter_sor", "filter_ror", "filter_compact")}
    print(f"rep {rep}: grid {t['grid']:.2f} ms  lrf {t['lrf']:.2f} ms | filter_sor {t['filter_sor']:.2f} ms  filter_ror {t['filter_ror']:.2f} ms  "
          f"filter_compact {t['filter_compact']:.2f} ms | sor/lrf {t['filter_sor'] / t['lrf']:.2f}  ror/lrf {t['filter_ror'] / t['lrf']:.2f}", flush=True)
k = keep.cpu().numpy().astype(bool)
is_out = np.zeros(len(k), bool)
for o in range(args.objects):
    is_out[po[o] + args.points:po[o + 1]] = True
print(f"SOR (MeanK {args.mean_k}, StddevMul {args.stddev_mul}): removed {(~k[is_out]).sum()} of {is_out.sum()} outliers and {(~k[~is_out]).sum()} of "
      f"{(~is_out).sum()} surface points; {int(new_off[-1])} points left. ROR (r {args.radius}, > {args.min_neighbors}): kept {int(keep_r.sum())}")

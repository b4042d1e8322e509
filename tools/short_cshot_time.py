"""SHORT_CSHOT beside SHORT_SHOT and CSHOT-1344 on one bench-sized coloured batch (16 384 points, 1024 keypoints per object) -- the
measurement of DESIGN.md's SHORT_CSHOT subsection, a sibling of short_shot_time.py. Per kernel: the library timer ("short_cshot" at the
default 512 bins and at 1216 bins, "short_shot" at 32 bins, "cshot1344") of single launches on the same cloud, keypoints, frames and
radius, after 3 warm-ups, as median [min .. max] over --reps launches, with the bytes-per-keypoint model M_k * 32 + 52 + 4 D
(SHORT_SHOT: M_k * 16 + 48 + 4 D; CSHOT: M_k * 28 + 52 + 4 * 1344 as shot.hip states it) and its share of the 8 TB/s HBM peak. The share
of neighbours that take the FP64 sequence is counted on the host for a sample of keypoints with the kernel's own rule (a raw value of
either grid within eps = 2e-6 (bins + 1) of an integer n >= 1 or of n + 0.5), on float64 raw values.
End to end: the detection step of pipeline.py (features -> kNN K = 1 -> votes -> maxima) with CSHOT-1344 and with SHORT_CSHOT-512 on the
workload of bench config 3 (coloured partial views, Radius 0.05, LeafSize 0.02, chi-square, 10 000-word random codebook), with the
library timers of one step.

    python tools/short_cshot_time.py [--objects 256] [--reps 10] [--no-e2e]
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

HBM_PEAK = 8e12


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return f"{np.median(v):.3f} [{v[0]:.3f} .. {v[-1]:.3f}]"


def fp64_share(host, lrf, radius, grids, n_kp=512):
    """share of the neighbours of the first n_kp keypoints of object 0 whose raw value on one of `grids` is within the kernel's eps of a decision"""
    p = host["xyz"][host["pt_off"][0]:host["pt_off"][1]].astype(np.float64)
    kp = host["kp"][host["kp_off"][0]:host["kp_off"][0] + n_kp].astype(np.float64)
    near = total = 0
    for k in range(len(kp)):
        f = lrf[host["kp_off"][0] + k].astype(np.float64).reshape(3, 3)
        if not np.isfinite(f).all():
            continue
        v = p - kp[k]
        d2 = (v * v).sum(1)
        v = v[(d2 < radius * radius) & (d2 > 1e-15)]
        loc = v @ f.T
        r = np.sqrt((loc * loc).sum(1))
        theta = np.degrees(np.arccos(np.clip(loc[:, 2] / r, -1, 1)))
        phi = np.degrees(np.arctan2(loc[:, 1], loc[:, 0]))
        hit = np.zeros(len(r), bool)
        for rb, eb, ab in grids:
            for raw, bins in ((rb * r / radius, rb), (eb * theta / 180, eb), (ab * (phi + 180) / 360, ab)):
                eps = 2e-6 * (bins + 1)
                fl = np.floor(raw)
                d = raw - fl
                hit |= ((fl >= 1) & (d < eps)) | ((fl >= 0) & (1 - d < eps)) | (np.abs(d - 0.5) < eps)
        near += int(hit.sum()); total += len(r)
    return near / max(total, 1), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, pipeline, synthetic = pkg.capi, pkg.pipeline, pkg.synthetic
    C = args.classes
    test = synthetic.Dataset(C, args.objects, split=1, n_points=16384, n_keypoints=1024, with_color=True)
    jobs = [(test, list(range(args.objects)))]
    c3 = bench.CONFIGS[3] if hasattr(bench, "CONFIGS") else None
    if not args.no_e2e:
        kw3 = dict(n_points=8192, leaf=0.02, scale=0.15, with_color=True, partial_view=True)
        train3, test3 = synthetic.Dataset(51, 51, split=0, **kw3), synthetic.Dataset(51, 153, split=1, **kw3)
        order3 = sorted(range(51), key=lambda i: (train3.label(i), i))
        jobs += [(test3, list(range(153)))] + [(train3, order3[s:s + 32]) for s in range(0, 51, 32)]
    pool = multiprocessing.get_context("fork").Pool(max(1, min(16, len(os.sched_getaffinity(0)))))
    host = bench.generate_batches(synthetic, jobs, pool)
    pool.close(); pool.join()

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    b = pipeline.DeviceBatch(host[0], dev)
    base = pipeline.IsmConfig(n_classes=C)
    cell = min(base.radius, base.lrf_radius) * 0.4
    cloud = capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, cell, rgba=b.rgba)
    kp = (b.kp_off, b.kx, b.ky, b.kz)
    lrf = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
    _, cnt = capi.shot352(ctx, cloud, *kp, lrf, base.radius, want_counts=True)
    mk = float(cnt.float().mean())
    nkp = int(b.kp_off[-1])
    S, L = ((2, 2, 8), (2, 2, 8), 15), ((8, 4, 8), (2, 4, 8), 15)
    sc = lambda g: (lambda: capi.short_cshot(ctx, cloud, *kp, b.kp_rgba, lrf, base.radius, bins=g[0], color_bins=g[1], hist_size=g[2]))
    kernels = [("cshot1344", 1344, 28, 52, lambda: capi.cshot1344(ctx, cloud, *kp, b.kp_rgba, lrf, base.radius)),
               ("short_shot", 32, 16, 48, lambda: capi.short_shot(ctx, cloud, *kp, lrf, base.radius, bins=(2, 2, 8))),
               ("short_cshot", 512, 32, 52, sc(S)),
               ("short_cshot", 1216, 32, 52, sc(L))]
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints, radius {base.radius}, mean neighbours M_k {mk:.0f}")
    ctx.timers_enable(True)
    for name, dim, per_nb, fixed, call in kernels:
        for _ in range(3):
            call()
        ctx.sync()
        ms = []
        for _ in range(args.reps):
            ctx.timers_reset()
            call()
            ctx.sync()
            ms.append(ctx.timer(name)[0])
        per_kp = mk * per_nb + fixed + 4 * dim
        model = nkp * per_kp
        rate = model / (np.median(ms) * 1e-3)
        print(f"{name} D={dim}: {spread(ms)} ms per launch; model {per_kp:.0f} B per keypoint, {model / 1e9:.2f} GB -> {rate / 1e9:.0f} GB/s at the median, "
              f"{100 * rate / HBM_PEAK:.1f} % of the 8 TB/s peak")
    ctx.timers_enable(False)
    lrf_h = lrf.cpu().numpy()
    for label, grids in (("(2,2,8) shape = colour grid", [(2, 2, 8)]), ("(8,4,8) shape + (2,4,8) colour grid", [(8, 4, 8), (2, 4, 8)])):
        share, total = fp64_share(host[0], lrf_h, base.radius, grids)
        print(f"neighbours re-taken in FP64, {label}: {100 * share:.4f} % of {total}")
    cloud.close()
    if args.no_e2e:
        return
    b3 = pipeline.DeviceBatch(host[1], dev)
    tb = [pipeline.DeviceBatch(h, dev) for h in host[2:]]
    common = dict(k=1, n_classes=51, max_maxima=16, radius=0.05, lrf_radius=0.05, distance="ChiSquared", bandwidth=0.045, use_random_codebook=True,
                  random_codebook_size=10000)
    for kw in (dict(feature="CSHOT"), dict(feature="SHORT_CSHOT")):
        rec = pipeline.Recognizer(capi.Ctx(0), pipeline.IsmConfig(**common, **kw))
        cb = rec.train(tb)
        for _ in range(2):
            out = rec.detect(b3)
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(3, args.reps // 2)):
            t0 = time.perf_counter()
            out = rec.detect(b3)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        acc = float((out["class_score"].argmax(1).cpu().numpy() == host[1]["labels"]).mean())
        rec.ctx.timers_enable(True); rec.ctx.timers_reset()          # where one step's device time goes
        rec.detect(b3)
        rec.ctx.sync()
        parts = {n: rec.ctx.timer(n)[0] for n in ("grid", "lrf", "cshot1344", "short_cshot", "knn", "cast_votes", "maxima")}
        rec.ctx.timers_enable(False)
        print("  device ms: " + ", ".join(f"{n} {v:.2f}" for n, v in parts.items() if v > 0))
        print(f"detect step, feature {kw['feature']} (dim {rec.cfg.dim}, {cb['words'].shape[0]} words, {int(b3.kp_off[-1])} keypoints): {spread(ms)} ms per 153 objects; "
              f"top-1 on the synthetic split {acc:.3f}")


if __name__ == "__main__":
    main()

"""Region (global) descriptors on the device -- the measurement of DESIGN.md 4.13.
Workload: --objects skewed blobs of --points points each (tests/global_scenes.blob), one whole-object region per object. On the same
cloud in the same process, device events (the library timers), --warmup runs, then --reps repetitions of
  ismhip_global_short_shot   timer "global_short_shot" (2 x 2 x 8 bins)
  ismhip_global_shot352      timer "global_shot352"
  ismhip_global_vfh          timer "global_vfh" (viewpoint (0, 0, 0), size component off)
  ismhip_global_gasd         timer "global_gasd" (view direction (0, 0, 1)), once without colour (512 floats) and once with (984 floats,
                             seeded random colours on the same cloud); --plane adds the same two on planar patches of the same size, the
                             same-address case of its histogram (every point in one z layer of cells)
  the per-keypoint route     timers "lrf" + "shot352": ismhip_shot_lrf + ismhip_shot352 with ONE keypoint per object at its centroid and
                             the batch's LARGEST radius -- the only way the per-keypoint entries reach the same neighbourhood (they take
                             one radius per call); its rows equal the region rows only for the object that has that radius
reported as median [min .. max] milliseconds, with the bytes one region streams by the model of csrc/global.hip (16 B per point and
sweep, 5 sweeps, 6 + normals for SHOT-352; VFH: 2 sweeps of a whole object, each with the 16 B normal beside the 16 B position; GASD: 3
sweeps of a whole object, + 4 B per point for its colour) and the share of the HBM peak (--peak-gbs) those bytes would be at the measured time. The
outputs of the repetitions are compared bit for bit.

    python tools/global_time.py [--objects 256] [--points 16384] [--reps 20] [--warmup 3] [--plane]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge   # noqa: E402
import global_scenes as gs     # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plane", action="store_true", help="also time ismhip_global_gasd on planar patches (its same-address case)")
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM peak of the device in GB/s (MI355X: 8 TB/s)")
    args = ap.parse_args()
    capi = ge.load_package().capi

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    rng = np.random.default_rng(3)
    n_obj, n = args.objects, args.points
    objs = [gs.blob(rng, n, shift=rng.uniform(-1, 1, 3)) for _ in range(n_obj)]
    p = np.concatenate([o[0] for o in objs]); nr = np.concatenate([o[1] for o in objs])
    off = (np.arange(n_obj + 1) * n).astype(np.uint32)
    t = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (p, nr) for i in range(3)]
    rgba = torch.as_tensor(rng.integers(0, 1 << 24, size=len(p)).astype(np.int32)).to(dev)
    cloud = capi.Cloud(ctx, off, *t, 0.1, rgba=rgba)
    regions = np.arange(n_obj, dtype=np.int32)
    print(f"{n_obj} objects of {n} points, one whole-object region each")

    ctx.timers_enable(True)
    results = {}

    def timed(label, names, call):
        ms, first = [], None
        for rep in range(args.warmup + args.reps):
            ctx.sync(); ctx.timers_reset()
            out = call()
            ctx.sync()
            if first is None:
                first = [o.clone() for o in out]
            for a, b in zip(first, out):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: outputs differ between two runs"
            if rep >= args.warmup:
                ms.append(sum(ctx.timer(k)[0] for k in names))
        results[label] = float(np.median(ms))
        print(f"{label}: {spread(ms)} ms")
        return first

    g = timed("global_short_shot", ("global_short_shot",),
              lambda: list(capi.global_short_shot(ctx, cloud, dev, regions, bins=(2, 2, 8)).values()))
    timed("global_shot352", ("global_shot352",), lambda: list(capi.global_shot352(ctx, cloud, dev, regions).values()))
    timed("global_vfh", ("global_vfh",), lambda: list(capi.global_vfh(ctx, cloud, dev, regions).values()))
    timed("global_gasd (shape, 512 floats)", ("global_gasd",), lambda: list(capi.global_gasd(ctx, cloud, dev, regions, with_color=False).values()))
    timed("global_gasd (colour, 984 floats)", ("global_gasd",), lambda: list(capi.global_gasd(ctx, cloud, dev, regions).values()))
    if args.plane:
        xy = rng.uniform(-0.3, 0.3, size=(n_obj * n, 2)) * [1.0, 0.6]
        pp = np.stack([xy[:, 0], xy[:, 1], 1.5 + 0.75 * xy[:, 0]], 1).astype(np.float32) + np.repeat(rng.uniform(-1, 1, (n_obj, 3)), n, 0).astype(np.float32)
        tp = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (pp, nr) for i in range(3)]
        plane = capi.Cloud(ctx, off, *tp, 0.1, rgba=rgba)
        timed("global_gasd on planes (shape)", ("global_gasd",), lambda: list(capi.global_gasd(ctx, plane, dev, regions, with_color=False).values()))
        timed("global_gasd on planes (colour)", ("global_gasd",), lambda: list(capi.global_gasd(ctx, plane, dev, regions).values()))
        plane.close()
    cen = capi.cloud_centroids(ctx, cloud, dev)
    rmax = float(capi.cloud_radii(ctx, cloud, cen).max())
    kp_off = np.arange(n_obj + 1, dtype=np.uint32)
    k = [cen[:, i].contiguous() for i in range(3)]

    def per_keypoint():
        lrf = capi.shot_lrf(ctx, cloud, kp_off, *k, rmax)
        return [lrf, capi.shot352(ctx, cloud, kp_off, *k, lrf, rmax)]
    timed(f"per-keypoint route (one keypoint per object, radius {rmax:.3f})", ("lrf", "shot352"), per_keypoint)
    ctx.timers_enable(False)

    # VFH on a whole object: radius + normal sums, histogram; each sweep reads position and normal
    # GASD on a whole object: radius + covariance, max_coord + sign counts, histogram (+ 4 B per point for the colour)
    for label, sweeps, extra in (("global_short_shot", 5, 0), ("global_shot352", 6, 16), ("global_vfh", 2, 32),
                                 ("global_gasd (shape, 512 floats)", 3, 0), ("global_gasd (colour, 984 floats)", 3, 4)):
        b = n * (16 * sweeps + extra)
        gbs = b * n_obj / (results[label] * 1e-3) / 1e9
        print(f"{label}: {b} bytes streamed per region by the model ({sweeps} sweeps), {gbs:.1f} GB/s = {100 * gbs / args.peak_gbs:.2f} % of the HBM peak; "
              f"compulsory (one sweep) {16 * n * n_obj / (results[label] * 1e-3) / 1e9:.1f} GB/s")
    print(f"global_gasd / global_vfh: {results['global_gasd (shape, 512 floats)'] / results['global_vfh']:.2f} without colour, "
          f"{results['global_gasd (colour, 984 floats)'] / results['global_vfh']:.2f} with")
    assert g is not None
    cloud.close()


if __name__ == "__main__":
    main()

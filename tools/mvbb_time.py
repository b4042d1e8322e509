"""Minimum-volume bounding boxes on the device -- the measurement of DESIGN.md 4.24.
Workload: --objects skewed blobs of --points points each (tests/global_scenes.blob), one whole-object region per object. On the same
cloud in the same process, device events (the library timers), --warmup runs, then --reps repetitions of
  ismhip_region_mvbb   timer "region_mvbb"
  ismhip_global_gasd   timer "global_gasd" (shape only): a region descriptor on the same regions, for scale
reported as median [min .. max] milliseconds of --reps repetitions (the circles: a quarter as many, at least 3; every line states its
count); the outputs of the repetitions are compared bit for bit.
What bounds the kernel is asked of the kernel itself, by two more runs of ismhip_region_mvbb:
  the same blobs cut to half their points    the pair searches of steps A and B do n^2 / 2 FP64 distance evaluations each and shrink to a
                                             quarter; everything else (sweeps, the hull of the few survivors) to a half or less
  points on tilted circles, --points each    the pre-filter's worst case: every point survives every round whose axis looks at the
                                             circle, is rank-sorted (n^2 comparisons) and goes through the one-thread monotone chain
with the FP64 operations of the two pair searches (8 per pair: 3 subtractions, 3 products, 2 sums) against the measured time.

    python tools/mvbb_time.py [--objects 256] [--points 16384] [--reps 20] [--warmup 3] [--out profiles/mvbb_time.txt]
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
import mvbb_scenes as ms       # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    capi = ge.load_package().capi
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    rng = np.random.default_rng(3)
    n_obj, n = args.objects, args.points
    blobs = [gs.blob(rng, n, shift=rng.uniform(-1, 1, 3))[0] for _ in range(n_obj)]
    ang = np.arange(n) * (2.0 * np.pi / n)
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], axis=1)
    circles = [(ring @ ms.rotation(900 + k).T * 0.8 + rng.uniform(-1, 1, 3)).astype(np.float32) for k in range(n_obj)]
    regions = np.arange(n_obj, dtype=np.int32)

    def make(objs):
        p = np.concatenate(objs)
        off = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.uint32)
        t = [torch.as_tensor(np.ascontiguousarray(p[:, i])).to(dev) for i in range(3)]
        z = [torch.zeros(len(p), dtype=torch.float32, device=dev) for _ in range(3)]
        return capi.Cloud(ctx, off, *t, *z, 0.1), t, z

    ctx.timers_enable(True)
    results = {}

    def timed(label, name, call, reps):
        ms_, first = [], None
        for rep in range(args.warmup + reps):
            ctx.sync(); ctx.timers_reset()
            out = call()
            ctx.sync()
            if first is None:
                first = [o.clone() for o in out]
            for a, b in zip(first, out):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: outputs differ between two runs"
            if rep >= args.warmup:
                ms_.append(ctx.timer(name)[0])
        results[label] = float(np.median(ms_))
        say(f"{label}: {spread(ms_)} ms (median [min .. max] of {reps})")
        return first

    say(f"{n_obj} objects, one whole-object region each; device events, {args.warmup} warm-up runs before every line's repetitions")
    cloud, *keep = make(blobs)
    out = timed(f"region_mvbb, blobs of {n} points", "region_mvbb", lambda: list(capi.region_mvbb(ctx, cloud, dev, regions).values()), args.reps)
    trace = out[-1].cpu().numpy()
    say(f"  hull sizes over the rounds: median {int(np.median(trace[:, 9::4]))}, largest {int(trace[:, 9::4].max())}; rounds taken per region: "
        f"median {int(np.median(trace[:, 8::4].sum(1)))}; most survivors of the pre-filter in a round: median {int(np.median(trace[:, 7]))}, "
        f"largest {int(trace[:, 7].max())}")
    timed(f"global_gasd (shape), blobs of {n} points", "global_gasd", lambda: list(capi.global_gasd(ctx, cloud, dev, regions, with_color=False).values()),
          args.reps)
    cloud.close()
    half, *keep = make([b[: n // 2] for b in blobs])
    timed(f"region_mvbb, the same blobs cut to {n // 2} points", "region_mvbb", lambda: list(capi.region_mvbb(ctx, half, dev, regions).values()), args.reps)
    half.close()
    rings, *keep = make(circles)
    out = timed(f"region_mvbb, tilted circles of {n} points", "region_mvbb", lambda: list(capi.region_mvbb(ctx, rings, dev, regions).values()),
                max(3, args.reps // 4))
    tr = out[-1].cpu().numpy()
    say(f"  largest hull over the rounds: {int(tr[:, 9::4].max())}; most survivors of the pre-filter in a round: {int(tr[:, 7].max())}")
    rings.close()
    ctx.timers_enable(False)

    full, cut, ring_ms = (results[k] for k in list(results)[0:1] + list(results)[2:4])
    flops = 2 * 8 * (n * (n - 1) / 2) * n_obj
    say(f"pair searches: {flops / 1e9:.1f} G FP64 operations per call = {flops / (full * 1e-3) / 1e12:.2f} T/s at the measured time")
    say(f"full / half = {full / cut:.2f} (4: the n^2 pair searches alone; 2: linear work alone)")
    say(f"circles / blobs = {ring_ms / full:.2f} (the rank sort and the one-thread chain of {n} survivors, over the same pair searches)")
    say(f"region_mvbb / global_gasd = {full / results[list(results)[1]]:.1f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

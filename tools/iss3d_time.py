"""ISS3D keypoints on the device -- the measurement of DESIGN.md 4.14.
Workload: --objects bumpy ellipsoids of --points points each (tests/iss3d_scenes.bumpy_ellipsoid, about one unit across; the reference's
default radii 0.1 / 0.05 then hold a few hundred and about a hundred neighbours at 16384 points). On the same cloud in the same process,
device events (the library timers), --warmup runs, then --reps repetitions of
  ismhip_iss3d_keypoints        timers "iss3d_saliency" and "iss3d_nms", and the wall time of the whole call (it synchronises; the
                                difference is the ordered compaction and the offsets' round trip)
  ismhip_estimate_normals_pca   timer "normals_pca" at the salient radius: the sibling sweep with nearly the same accumulators, the yardstick
for both query-to-lane mappings of the saliency sweep (one thread per query, the default, and ISMHIP_ISS3D_MAP=wave: one wave per
query), each on a context of its own. Reported as median [min .. max] milliseconds. The outputs of all repetitions and of the two
mappings are compared bit for bit.

    python tools/iss3d_time.py [--objects 256] [--points 16384] [--reps 20] [--warmup 3] [--salient-radius 0.1] [--non-max-radius 0.05]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge   # noqa: E402
import iss3d_scenes as scenes  # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--salient-radius", type=float, default=0.1)
    ap.add_argument("--non-max-radius", type=float, default=0.05)
    ap.add_argument("--maps", default="thread,wave", help="mappings of the saliency sweep to time")
    args = ap.parse_args()
    capi = ge.load_package().capi

    import torch
    dev = torch.device("cuda:0")
    n_obj, n = args.objects, args.points
    p = np.concatenate([scenes.bumpy_ellipsoid(n, 100 + o) for o in range(n_obj)])
    off = (np.arange(n_obj + 1) * n).astype(np.uint32)
    t = [torch.as_tensor(np.ascontiguousarray(p[:, i])).to(dev) for i in range(3)] + [torch.zeros(len(p), dtype=torch.float32, device=dev) for _ in range(3)]
    rs, rn = args.salient_radius, args.non_max_radius
    print(f"{n_obj} objects of {n} points, SalientRadius {rs}, NonMaxRadius {rn}, Gamma 0.975 / 0.975, MinNeighbors 5")

    answers = {}
    for mapping in args.maps.split(","):
        os.environ["ISMHIP_ISS3D_MAP"] = mapping
        ctx = capi.Ctx(0)                                     # the switch is read when the context is created
        cloud = capi.Cloud(ctx, off, *t, 0.4 * rn)
        ctx.timers_enable(True)

        def timed(label, names, call):
            ms, wall, first = {k: [] for k in names}, [], None
            for rep in range(args.warmup + args.reps):
                ctx.sync(); ctx.timers_reset()
                t0 = time.perf_counter()
                out = call()
                ctx.sync()
                dt = (time.perf_counter() - t0) * 1e3
                if first is None:
                    first = [o.clone() for o in out]
                for a, b in zip(first, out):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: outputs differ between two runs"
                if rep >= args.warmup:
                    wall.append(dt)
                    for k in names:
                        ms[k].append(ctx.timer(k)[0])
            for k in names:
                print(f"[{mapping}] {label} timer {k}: {spread(ms[k])} ms")
            print(f"[{mapping}] {label} whole call (wall): {spread(wall)} ms")
            return first

        def keypoints():
            ko, kx, ky, kz, _kc, src = capi.iss3d_keypoints(ctx, cloud, rs, rn)
            return [torch.as_tensor(ko.astype(np.int32)), kx, ky, kz, src]
        kp = timed("iss3d_keypoints", ("iss3d_saliency", "iss3d_nms"), keypoints)
        sal, _eig, cnt = capi.iss3d_saliency(ctx, cloud, rs, want_eig=False)
        ctx.sync()
        print(f"[{mapping}] keypoints {int(kp[0][-1])} ({int(kp[0][-1]) / n_obj:.1f} per object), salient points {int((sal > 0).sum())}, "
              f"neighbours per query mean {float(cnt.float().mean()):.1f} max {int(cnt.max())}")
        answers[mapping] = kp + [sal.view(torch.int32)]
        nrm = [torch.empty_like(t[0]) for _ in range(3)]
        timed(f"estimate_normals_pca (radius {rs})", ("normals_pca",), lambda: list(capi.estimate_normals_pca(ctx, cloud, rs, 0, *nrm)))
        ctx.timers_enable(False)
        cloud.close()
        ctx.close()
    keys = list(answers)
    for other in keys[1:]:
        for a, b in zip(answers[keys[0]], answers[other]):
            assert torch.equal(a.view(torch.int32).cpu(), b.view(torch.int32).cpu()), f"mappings {keys[0]} and {other} differ"
    if len(keys) > 1:
        print("the mappings agree bit for bit")


if __name__ == "__main__":
    main()

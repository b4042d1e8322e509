"""ismhip_global_cvfh on the device -- the measurement of DESIGN.md 4.25.
Workload: --objects synthetic objects (synthetic.make_object, the classes in turn) of --points points each, one whole-object region per
object, at the parameters of config/modelnet10_shot_cvfh.ism. On the same cloud in the same process, device events (the library
timers), --warmup runs, then --reps repetitions, median [min .. max] milliseconds of
  ismhip_global_cvfh             timer "global_cvfh", and inside it
      "cvfh_normals"             region kernel, workspace init and the dense re-estimation of the clustering normals
      "cvfh_label"               the dense link sweep with its unions, and the flatten pass
      "cvfh_stats"               kept clusters in order
      "cvfh_rows"                one workgroup per (region, row slot); reported in total and per ROW actually produced
  ismhip_global_vfh              timer "global_vfh": the yardstick of the row phase (same two sweeps per row), and the figure that must
                                 not move against the parent commit (this tool runs there too: it skips what the library lacks)
  ismhip_estimate_normals_pca    timer "normals_pca" at CvfhNormalRadius: the yardstick of the normal pass
The outputs of the repetitions are compared bit for bit.

    python tools/cvfh_time.py [--objects 256] [--points 16384] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=8)
    args = ap.parse_args()
    pkg = ge.load_package()
    capi = pkg.capi
    par = dict(CvfhClusterTolerance=0.06, CvfhNormalRadius=0.08, CvfhMinPoints=200)
    cfg = os.path.join(ROOT, "config", "modelnet10_shot_cvfh.ism")
    if os.path.exists(cfg):
        par = json.load(open(cfg))["ObjectConfig"]["Children"]["GlobalFeatures"]["Parameters"]

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    n_obj, n = args.objects, args.points
    objs = [pkg.synthetic.make_object(o % 10, 0, o, n)[:2] for o in range(n_obj)]
    # the viewpoint (0, 0, 0) lies inside an object centred there: move every object two units down the z axis, as a sensor sees it
    p = np.concatenate([o[0] + np.float32([0, 0, 2]) for o in objs]).astype(np.float32); nr = np.concatenate([o[1] for o in objs])
    off = (np.arange(n_obj + 1) * n).astype(np.uint32)
    t = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (p, nr) for i in range(3)]
    cloud = capi.Cloud(ctx, off, *t, 0.1)
    regions = np.arange(n_obj, dtype=np.int32)
    print(f"{n_obj} objects of {n} points, one whole-object region each; {par}")

    ctx.timers_enable(True)

    def timed(label, names, call):
        ms, first = {k: [] for k in names}, None
        for rep in range(args.warmup + args.reps):
            ctx.sync(); ctx.timers_reset()
            out = call()
            ctx.sync()
            if first is None:
                first = [o.clone() for o in out]
            for a, b in zip(first, out):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: outputs differ between two runs"
            if rep >= args.warmup:
                for k in names:
                    ms[k].append(ctx.timer(k)[0])
        for k in names:
            print(f"{label} [{k}]: {spread(ms[k])} ms")
        return first, {k: float(np.median(v)) for k, v in ms.items()}

    _, vfh = timed("global_vfh", ("global_vfh",), lambda: list(capi.global_vfh(ctx, cloud, dev, regions).values()))
    if hasattr(capi, "global_cvfh"):
        names = ("global_cvfh", "cvfh_normals", "cvfh_label", "cvfh_stats", "cvfh_rows")
        keys = []

        def cvfh():
            out = capi.global_cvfh(ctx, cloud, dev, regions, cluster_tolerance=par["CvfhClusterTolerance"], normal_radius=par["CvfhNormalRadius"],
                                   min_points=par["CvfhMinPoints"], max_rows=args.max_rows)
            keys[:] = list(out.keys())
            return list(out.values())
        first, med = timed("global_cvfh", names, cvfh)
        ncl = first[keys.index("n_clusters")].cpu().numpy()
        rows = int(np.minimum(ncl, args.max_rows).sum())
        print(f"clusters per object: min {ncl.min()}, median {int(np.median(ncl))}, max {ncl.max()}; {rows} rows in {n_obj * args.max_rows} slots")
        print(f"cvfh_rows per row produced: {med['cvfh_rows'] / max(rows, 1) * 1e3:.3f} us; global_vfh per region: {vfh['global_vfh'] / n_obj * 1e3:.3f} us")
        nrm = [torch.empty(len(p), dtype=torch.float32, device=dev) for _ in range(3)]
        timed(f"estimate_normals_pca (radius {par['CvfhNormalRadius']})", ("normals_pca",),
              lambda: list(capi.estimate_normals_pca(ctx, cloud, par["CvfhNormalRadius"], 0, *nrm) or nrm))
    ctx.timers_enable(False)
    cloud.close()


if __name__ == "__main__":
    main()

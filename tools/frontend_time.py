"""Timing of the front end on the MI355X: the "grid", "lrf" and "shot352" timers of ismhip_cloud_create, ismhip_shot_lrf and
ismhip_shot352 on the batch of bench config 1 (908 objects x 16384 points, 1024 keypoints each in random order, cell 0.12, radii 0.3),
once per setting of the A/B switches of the grid build and of the keypoint order. Every setting gets a context of its own (the switches are
read when a context is created); the settings alternate over the repetitions. Prints one JSON line.
--lrf-type SHOTNA times ismhip_shotna_lrf (the z sign voted by the normals) under the same "lrf" timer key.
usage: python tools/frontend_time.py [--objects 908 --points 16384 --keypoints 1024 --cell 0.12 --radius 0.3 --reps 5 --lrf-type SHOT]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=908)
ap.add_argument("--points", type=int, default=16384)
ap.add_argument("--keypoints", type=int, default=1024)
ap.add_argument("--cell", type=float, default=0.12)
ap.add_argument("--radius", type=float, default=0.3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--lrf-type", choices=["SHOT", "SHOTNA"], default="SHOT")
args = ap.parse_args()
import torch
pkg = ge.load_package()
capi, syn = pkg.capi, pkg.synthetic
dev = torch.device("cuda:0")

rng = np.random.default_rng(7)
xyz, nrm, kp, po, ko = [], [], [], [0], [0]
for i in range(args.objects):
    p, n = syn.make_object(i % 10, 1, i, n_points=args.points)
    xyz.append(p); nrm.append(n)
    kp.append(p[rng.permutation(len(p))[:args.keypoints]])
    po.append(po[-1] + len(p)); ko.append(ko[-1] + len(kp[-1]))
xyz, nrm, kp = np.concatenate(xyz), np.concatenate(nrm), np.concatenate(kp)
po, ko = np.asarray(po, np.uint32), np.asarray(ko, np.uint32)
T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
pts = [T(xyz[:, i]) for i in range(3)] + [T(nrm[:, i]) for i in range(3)]
kps = [T(kp[:, i]) for i in range(3)]

SETTINGS = {"default": {}, "grid_fused_0": {"ISMHIP_GRID_FUSED": "0"}, "kp_order_0": {"ISMHIP_KP_ORDER": "0"}}
SWITCHES = sorted({k for env in SETTINGS.values() for k in env})
ctxs = {}
for name, env in SETTINGS.items():
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    ctxs[name] = capi.Ctx(0)
for k in SWITCHES:
    os.environ.pop(k, None)


def once(ctx):
    cloud = capi.Cloud(ctx, po, *pts, args.cell)
    lrf = capi.LRF_TYPES[args.lrf_type](ctx, cloud, ko, *kps, args.radius)
    desc = capi.shot352(ctx, cloud, ko, *kps, lrf, args.radius)
    ctx.sync()
    cloud.close()
    return lrf, desc


ref = None
for name, ctx in ctxs.items():                                      # warm-up: code objects, scratch, the cloud pool; and the outputs agree
    lrf, desc = once(ctx)
    got = (lrf.cpu().numpy().tobytes(), desc.cpu().numpy().tobytes())
    ref = ref or got
    assert got == ref, f"{name}: outputs differ from the default setting"
    ctx.timers_enable(True)
runs = {name: [] for name in ctxs}
for rep in range(args.reps):
    for name, ctx in ctxs.items():
        ctx.timers_reset()
        once(ctx)
        runs[name].append({t: round(ctx.timer(t)[0], 4) for t in ("grid", "lrf", "shot352")})
print(json.dumps({"objects": args.objects, "points": int(po[-1]), "keypoints": int(ko[-1]), "cell": args.cell, "radius": args.radius, "lrf_type": args.lrf_type,
                  "ms": runs, "outputs_identical": True}))

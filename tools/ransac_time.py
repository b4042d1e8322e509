"""The `maxima` timer with and without the RANSAC vote filter (Voting.RansacVoteFiltering) on the votes of bench.py config 1 / config 2
shapes: N_OBJ (default 128) rotated test objects, so that the poses are not the identity; two warm-up detections per side, five timed,
alternating. Prints one JSON line per config and writes profiles-style JSON to the path given as argv[1]."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
capi, pipeline, syn = pkg.capi, pkg.pipeline, pkg.synthetic
import multiprocessing


def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q); w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

N_OBJ = int(os.environ.get("N_OBJ", "128"))

def gen_rot(job):
    test, i, nkp, seed = job
    o = test.get(i)
    R = _rot(np.random.default_rng([seed, i])).astype(np.float32)
    xyz = np.ascontiguousarray((o["xyz"] @ R.T).astype(np.float32)); nrm = np.ascontiguousarray((o["normals"] @ R.T).astype(np.float32))
    return dict(xyz=xyz, normals=nrm, kp=syn.keypoints_fixed(xyz, nkp), label=o["label"])

def gen_train(job):
    train, ids = job
    return train.batch(ids)

def batch_of(objs):
    pt_off = np.concatenate([[0], np.cumsum([len(o["xyz"]) for o in objs])]).astype(np.uint32)
    kp_off = np.concatenate([[0], np.cumsum([len(o["kp"]) for o in objs])]).astype(np.uint32)
    return dict(pt_off=pt_off, kp_off=kp_off, xyz=np.concatenate([o["xyz"] for o in objs]), normals=np.concatenate([o["normals"] for o in objs]),
                kp=np.concatenate([o["kp"] for o in objs]), labels=np.array([o["label"] for o in objs], np.int32))

CONFIGS = {1: dict(classes=10, keypoints=1024, tpc=10, model=dict(feature="SHOT")),
           2: dict(classes=40, keypoints=2048, tpc=1, model=dict(feature="SHOT", use_random_codebook=True, random_codebook_size=10000))}
host = {}
pool = multiprocessing.get_context("fork").Pool(14)
for cid, cd in CONFIGS.items():
    C = cd["classes"]; n_train = cd["tpc"] * C
    train = syn.Dataset(C, n_train, split=0, n_points=16384, n_keypoints=cd["keypoints"])
    test = syn.Dataset(C, N_OBJ, split=1, n_points=16384, n_keypoints=cd["keypoints"])
    order = sorted(range(n_train), key=lambda i: (train.label(i), i))
    tb = pool.map(gen_train, [(train, order[s:s + 8]) for s in range(0, n_train, 8)])
    objs = pool.map(gen_rot, [(test, i, cd["keypoints"], 77) for i in range(N_OBJ)])
    host[cid] = (tb, batch_of(objs))
pool.close(); pool.join()
print("host data ready", flush=True)
import torch
dev = torch.device("cuda:0")
res = {}
for cid, cd in CONFIGS.items():
    tb, nb = host[cid]
    ctx_off, ctx_on = capi.Ctx(0), capi.Ctx(0)
    cfg_off = pipeline.IsmConfig(k=1, n_classes=cd["classes"], max_maxima=16, **cd["model"])
    cfg_on = pipeline.IsmConfig(k=1, n_classes=cd["classes"], max_maxima=16, ransac_vote_filtering=True, **cd["model"])
    rec_off = pipeline.Recognizer(ctx_off, cfg_off); cb = rec_off.train([pipeline.DeviceBatch(b, dev) for b in tb])
    rec_on = pipeline.Recognizer(ctx_on, cfg_on); rec_on.load_codebook(cb)
    b = pipeline.DeviceBatch(nb, dev)
    for _ in range(2):
        o0 = rec_off.detect(b); o1 = rec_on.detect(b); torch.cuda.synchronize()
    for c in (ctx_off, ctx_on):
        c.timers_enable(True); c.timers_reset()
    steps = 5
    for _ in range(steps):
        o0 = rec_off.detect(b); torch.cuda.synchronize()
        o1 = rec_on.detect(b); torch.cuda.synchronize()
    t_off, t_on = ctx_off.timer("maxima"), ctx_on.timer("maxima")
    ctr = {k: ctx_on.timer(k)[0] / steps for k in ("ransac_clusters", "ransac_clusters_kept", "ransac_hypotheses_needed", "ransac_hypotheses_evaluated")}
    n0, n1 = o0["n"].cpu().numpy(), o1["n"].cpu().numpy()
    lab = nb["labels"]
    acc0 = float((o0["cls"][:, 0].cpu().numpy() == lab).mean()); acc1 = float((o1["cls"][:, 0].cpu().numpy()[n1 > 0] == lab[n1 > 0]).mean()) if (n1 > 0).any() else 0.0
    res[cid] = dict(objects=N_OBJ, votes_slots=int(o1["_keep"][3]["pos"].shape[0]), maxima_ms_off=t_off[0] / t_off[1], maxima_ms_on=t_on[0] / t_on[1],
                    vote_keypoints_ms=ctx_on.timer("vote_keypoints")[0] / max(1, ctx_on.timer("vote_keypoints")[1]), per_detect=ctr,
                    evaluated_over_needed=ctr["ransac_hypotheses_evaluated"] / max(1.0, ctr["ransac_hypotheses_needed"]),
                    maxima_off=int(n0.sum()), maxima_on=int(n1.sum()), objects_with_maxima_on=int((n1 > 0).sum()), top1_off=acc0, top1_on_where_any=acc1)
    print("config", cid, json.dumps(res[cid]), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)

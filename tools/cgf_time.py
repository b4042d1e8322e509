"""CGF stage by stage on the bench-sized batch (256 objects x 16 384 points x 1024 keypoints, radius 0.4) -- the measurement of DESIGN.md
4.20. Device events (the library timers) around single calls, median [min .. max] of --reps calls after --warmup warm-ups:
  "lrf" + "keypoint_normals_pca"  CGF's own frames (SHOT at 0.75 R) and the PCA normals of the keypoints (0.1 R)
  "cgf_raw"                       (k_cgf_raw) one wave per keypoint, 2244 counters per wave, all keypoints in one call
  "mlp_forward"                   (k_mlp_forward) the embedding 2244 -> 512 -> 512 -> 512 -> 512 -> 40 with seeded weights over the raw rows in
                                  chunks of --chunk keypoints (the sum over the chunks of one pass)
  "shot352"                       (k_shot<false>) on the same cloud, keypoints and radius: the sibling on the same balls
and, by torch events in the same run, a torch float32 `linear` chain (addmm + relu) on the same rows and weights: the yardstick of the
embedding. With the gather model of the raw kernel, sum_k M_k * 16 + K (12 + 36 + 12 + 4 * 2244) bytes (M_k = candidates of the ball: the
16-byte position record; the centre, the frame, the normal, the row), its share of the 8 TB/s HBM peak, and the embedding's share of the
155 TFLOP/s that the FP32 matrix cores reach (2 * sum in * out FLOP per row).

    python tools/cgf_time.py [--objects 256] [--reps 20] [--warmup 3] [--chunk 32768]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge   # noqa: E402
import bench                   # noqa: E402  (generate_batches: objects made by forked workers before the GPU is touched)

HBM_PEAK = 8e12
FP32_MATRIX_PEAK = 155e12
WIDTHS = [2244, 512, 512, 512, 512, 40]


def spread(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f} .. {v.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=32768)
    args = ap.parse_args()
    pkg = ge.load_package()
    capi, pipeline, synthetic = pkg.capi, pkg.pipeline, pkg.synthetic
    test = synthetic.Dataset(args.classes, args.objects, split=1, n_points=16384, n_keypoints=1024)
    pool = multiprocessing.get_context("fork").Pool(max(1, min(16, len(os.sched_getaffinity(0)))))
    host = bench.generate_batches(synthetic, [(test, list(range(args.objects)))], pool)
    pool.close(); pool.join()

    import torch
    dev = torch.device("cuda:0")
    ctx = capi.Ctx(0)
    b = pipeline.DeviceBatch(host[0], dev)
    base = pipeline.IsmConfig(n_classes=args.classes)
    radius = base.radius
    R, rmin, rl = capi.cgf_radii(radius)
    cloud = capi.Cloud(ctx, b.pt_off, b.x, b.y, b.z, b.nx, b.ny, b.nz, min(radius, base.lrf_radius) * 0.4)
    kp = (b.kp_off, b.kx, b.ky, b.kz)
    rng = np.random.default_rng(1)
    layers = [((rng.normal(size=(i, o)) / np.sqrt(i)).astype(np.float32), (0.1 * rng.normal(size=o)).astype(np.float32), l + 2 < len(WIDTHS))
              for l, (i, o) in enumerate(zip(WIDTHS[:-1], WIDTHS[1:]))]
    mlp = capi.Mlp(ctx, layers)
    lrf = capi.shot_lrf(ctx, cloud, *kp, rl)
    lrf_shot = capi.shot_lrf(ctx, cloud, *kp, base.lrf_radius)
    nrm = capi.keypoint_normals_pca(ctx, cloud, *kp, 0.1 * R)
    raw, ball = capi.cgf_raw(ctx, cloud, *kp, lrf, *nrm, R, rmin, want_counts=True)
    ctx.sync()
    nkp = int(b.kp_off[-1])
    out = torch.empty((nkp, WIDTHS[-1]), dtype=torch.float32, device=dev)
    chunks = [(s, min(nkp, s + args.chunk)) for s in range(0, nkp, args.chunk)]
    mk = float(ball.float().mean())
    print(f"{args.objects} objects x 16384 points, {nkp} keypoints, radius {radius} (R {R}, rmin {rmin}, LRF {rl}): {mk:.0f} deposits per keypoint, "
          f"NaN normals {int(torch.isnan(nrm[0]).sum())}, NaN frames {int(torch.isnan(lrf[:, 0]).sum())}, zero rows {int((ball == 0).sum())}; "
          f"raw rows {raw.numel() * 4 / 1e9:.2f} GB, embedded in {len(chunks)} chunks of {args.chunk}")
    ctx.timers_enable(True)

    def timed(names, call):
        for _ in range(args.warmup):
            call()
        ctx.sync()
        ms = []
        for _ in range(args.reps):
            ctx.timers_reset()
            call()
            ctx.sync()
            ms.append(sum(ctx.timer(n)[0] for n in names))
        return ms

    def frames():
        capi.shot_lrf(ctx, cloud, *kp, rl)
        capi.keypoint_normals_pca(ctx, cloud, *kp, 0.1 * R)

    def embed():
        for s, e in chunks:
            mlp.forward(raw[s:e], out=out[s:e])

    tf = timed(["lrf", "keypoint_normals_pca"], frames)
    tn = timed(["keypoint_normals_pca"], lambda: capi.keypoint_normals_pca(ctx, cloud, *kp, 0.1 * R))
    tr = timed(["cgf_raw"], lambda: capi.cgf_raw(ctx, cloud, *kp, lrf, *nrm, R, rmin))
    tm = timed(["mlp_forward"], embed)
    ts = timed(["shot352"], lambda: capi.shot352(ctx, cloud, *kp, lrf_shot, radius))
    ctx.timers_enable(False)

    tw = [(torch.as_tensor(W).to(dev), torch.as_tensor(bb).to(dev), r) for W, bb, r in layers]

    def torch_chain():
        for s, e in chunks:
            h = raw[s:e]
            for W, bb, r in tw:
                h = torch.addmm(bb, h, W)
                if r:
                    h = torch.relu_(h)
            out[s:e] = h
    for _ in range(args.warmup):
        torch_chain()
    tt = []
    for _ in range(args.reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); torch_chain(); z.record(); torch.cuda.synchronize()
        tt.append(a.elapsed_time(z))
    ref_out = out.clone()
    embed(); ctx.sync()
    diff = float((out - ref_out).abs().max())

    cand = nkp * (mk / 0.52) * 16.0                  # candidates of the swept cells: the ball is 0.52 of its bounding cube
    model = nkp * (mk * 16 + 12 + 36 + 12 + 4 * capi.CGF_RAW_DIM)
    rate = model / (np.median(tr) * 1e-3)
    flop_row = 2.0 * sum(i * o for i, o in zip(WIDTHS[:-1], WIDTHS[1:]))
    tflops = flop_row * nkp / (np.median(tm) * 1e-3) / 1e12
    print(f"frames + keypoint normals (lrf at {rl} + keypoint_normals_pca at {0.1 * R:.4f}): {spread(tf)} ms per call; of it the normals {spread(tn)}")
    print(f"cgf_raw (k_cgf_raw), {capi.CGF_RAW_DIM} bins:                 {spread(tr)} ms per call; model {model / 1e9:.2f} GB -> {rate / 1e9:.0f} GB/s, "
          f"{100 * rate / HBM_PEAK:.1f} % of the 8 TB/s peak (of the model, {4 * capi.CGF_RAW_DIM * nkp / 1e9:.2f} GB are the rows written; "
          f"candidates at ball / cube = 0.52: {cand / 1e9:.2f} GB)")
    print(f"mlp_forward (k_mlp_forward), {len(chunks)} chunks:           {spread(tm)} ms per pass; {flop_row / 1e6:.2f} MFLOP per row, {flop_row * nkp / 1e12:.2f} TFLOP per "
          f"pass -> {tflops:.1f} TFLOP/s, {100 * tflops * 1e12 / FP32_MATRIX_PEAK:.1f} % of the 155 TFLOP/s FP32 matrix peak")
    print(f"torch float32 addmm + relu chain, same rows and weights: {spread(tt)} ms per pass; mlp_forward / torch = {np.median(tm) / np.median(tt):.2f}; "
          f"largest difference between the two outputs {diff:.3g}")
    print(f"shot352 (k_shot<false>), same inputs:                    {spread(ts)} ms per call; cgf_raw / shot352 = {np.median(tr) / np.median(ts):.2f}")
    cloud.close(); mlp.close()


if __name__ == "__main__":
    main()

"""CPU model of the score-insertion ("hit") path of k_knn_l2_ring16's epilogue (DESIGN.md §4.1 "Hit path", §5) on oracle SHOT-352
descriptors of the bench's own generator, on the pattern of tools/stage1_proof_model.py. numpy + the oracle; no GPU.

  python tools/ring_hit_model.py [train_objects=100] [queries=300]

Stage 1 as the bench runs it: class-major codebook, 128 rotated coordinates, 2 splits x 8 lane slots (wave row, row group), T = 2
candidates per slot (a slot's own threshold is its third best score), thresholds shared by a query's eight slots once per tile, start
value = the best score in every 32nd tile relaxed by twice the mean second moment the truncation leaves out. A "hit" is a score that
passes the threshold as it stands at the start of its tile. Printed: hits per query (both splits together), hits per wave and tile (a wave serves 64
queries x 128 rows), the share of wave-tiles that take the hit branch, and the share of queries whose proof fails (margin 2e-3 on the
distance, as in the proof model) for
  today      today's rule
  rho_b      k = 1 only: every inserted row b with score s_b also lowers the threshold to (sqrt(s_b + (rho_q + rho_b)^2) + margin)^2 -- b's
             full distance is at most s_b + (rho_q + rho_b)^2, rho = the norm of what the rotation truncates -- per-row rho_b
  rho_max    the same with the codebook-wide maximum of rho_b
  rho_b/16   per-row rho_b and a start value from every 16th tile"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
ora = ge.load_oracle()
n_train = int(sys.argv[1]) if len(sys.argv) > 1 else 100
n_q = int(sys.argv[2]) if len(sys.argv) > 2 else 300
M, N_SPLITS, T, MARGIN = 128, 2, 2, 2e-3


def descriptors(ds, ids):
    out = []
    for i in ids:
        o = ds.get(i)
        x, y, z = (o["xyz"][:, j].copy() for j in range(3))
        nx, ny, nz = (o["normals"][:, j].copy() for j in range(3))
        kx, ky, kz = (o["kp"][:, j].copy() for j in range(3))
        po, ko = [0, len(x)], [0, len(kx)]
        lrf = ora.shot_lrf(po, x, y, z, ko, kx, ky, kz, 0.3)
        d = ora.shot352(po, x, y, z, nx, ny, nz, ko, kx, ky, kz, lrf, 0.4)
        d = d[0] if isinstance(d, tuple) else d
        out.append(d[~np.isnan(d).any(1)])
    return np.concatenate(out)


t0 = time.time()
W = descriptors(pkg.synthetic.Dataset(10, n_train, split=0, n_points=16384, n_keypoints=1024), range(n_train)).astype(np.float64)
Q = descriptors(pkg.synthetic.Dataset(10, 4, split=1, n_points=16384, n_keypoints=1024), range(1)).astype(np.float64)[:n_q]
obj = np.arange(len(W)) // 1024
W = W[np.argsort((obj % 10) * 100000 + obj, kind="stable")]                # class-major, as the bench trains
W = W[:len(W) // 512 * 512]
n_words, n_tiles = len(W), len(W) // 256
print(f"{n_words} words, {len(Q)} queries ({time.time() - t0:.0f} s of oracle)", flush=True)
w, V = np.linalg.eigh(W.T @ W)
V = V[:, ::-1]
Wr, Qr = W @ V, Q @ V


def sq(A, B):
    return (A * A).sum(1)[:, None] + (B * B).sum(1)[None] - 2 * A @ B.T


D_full, D_part = sq(Q, W), np.maximum(sq(Qr[:, :M], Wr[:, :M]), 0.0)
rho_w, rho_q = np.sqrt((Wr[:, M:] ** 2).sum(1)), np.sqrt((Qr[:, M:] ** 2).sum(1))
resid2 = float((rho_w ** 2).mean())
print(f"second moment in the leading {M} coordinates {1 - (Wr[:, M:] ** 2).sum() / (Wr ** 2).sum():.4f}; rho_b mean {rho_w.mean():.3f} max {rho_w.max():.3f}, "
      f"rho_q mean {rho_q.mean():.3f}")
rows = np.arange(256)
slot_of_row = (rows // 128) * 4 + (rows % 16) // 4                          # lane slot (wave row, row group) of a tile's row
tiles_per_split = n_tiles // N_SPLITS


def sweep(qi, rule, rho_rows, pre_step):
    """one query: (hits per split-sweep, [tile, wave row] hit flags, proof failed)"""
    dp, df = D_part[qi], D_full[qi]
    start = dp.reshape(n_tiles, 256)[::pre_step].min() + 2.0 * resid2
    hits, flags, kept_best, fail = [], np.zeros((n_tiles, 2), bool), np.inf, False
    for s in range(N_SPLITS):
        thr, lists, n_hit = start, [[] for _ in range(8)], 0
        for t in range(s * tiles_per_split, (s + 1) * tiles_per_split):
            d = dp[t * 256:(t + 1) * 256]
            h = np.nonzero(d < thr)[0]
            if len(h) == 0:
                continue
            n_hit += len(h)
            flags[t, 0] |= bool((h < 128).any()); flags[t, 1] |= bool((h >= 128).any())
            for r in h:
                lists[slot_of_row[r]].append((d[r], t * 256 + r))
                if rule:
                    thr = min(thr, (np.sqrt(d[r] + (rho_q[qi] + rho_rows[t * 256 + r]) ** 2) + MARGIN) ** 2)
            for l in lists:
                l.sort()
                del l[T + 1:]
                if len(l) == T + 1:
                    thr = min(thr, l[T][0])
        hits.append(n_hit)
        for l in lists:
            for _, r in l[:T]:
                kept_best = min(kept_best, df[r])
        fail |= max(np.sqrt(thr) - MARGIN, 0.0) ** 2 < kept_best          # every slot of the split reports the shared threshold
    return hits, flags, fail


for name, rule, rho_rows, pre_step in (("today", False, None, 32), ("rho_b", True, rho_w, 32), ("rho_max", True, np.full(n_words, rho_w.max()), 32),
                                       ("rho_b/16", True, rho_w, 16)):
    t0 = time.time()
    per_q, fails, flag_all = [], 0, []
    for qi in range(len(Q)):
        h, f, fail = sweep(qi, rule, rho_rows, pre_step)
        per_q.append(np.sum(h)); fails += fail; flag_all.append(f)
    per_q = np.asarray(per_q)
    groups = [np.any(flag_all[a:a + 64], axis=0) for a in range(0, len(Q) - 63, 64)]        # 64 queries = the columns of one wave
    taken = float(np.mean(groups)) if groups else float("nan")
    print(f"{name:9s} hits per query (both splits): mean {per_q.mean():.1f} median {np.median(per_q):.0f} p90 {np.percentile(per_q, 90):.0f}; "
          f"per wave and tile {64 * per_q.mean() / (n_tiles * 2):.2f}; wave-tiles with a hit {100 * taken:.0f} %; "
          f"proof failures {100.0 * fails / len(Q):.1f} %  ({time.time() - t0:.0f} s)", flush=True)

"""Stage 2 of the two-stage squared-L2 search on per-split failure lists: a query whose stage-1 proof failed is
searched again only on the rows of the stage-1 splits in which it failed; the answer is the merge of stage 1's result with the
result of every list the query stands in, and one exact scan serves the call. None of that may change an answer: indices and
distances are those of the exact-f32 route (ISMHIP_KNN_MODE=f32) bit for bit for every query, for k = 1 and 2, and the arrays of
ISMHIP_KNN_STAGE2_SPLITS=0 (every stage-2 query sweeps the whole codebook) byte for byte.

8192 queries x 8192 words x 352 dimensions, stage 1 on 128 rotated coordinates. The spectrum is steep by construction: the first
128 coordinates carry standard deviations from 0.2 down to 0.02, the other 224 carry 0.0006, so the rotation keeps (very nearly) the
first 128 coordinates and a vector that differs from a query only in the LAST 224 looks like the query itself to stage 1.

A proof failure is forced the way tests/test_gpu_knn_ring_hits.py forces hits: three rows (T + 1 for stage 1's T = 2) of ONE lane
slot, v + eps t_j with t_j a unit vector in the trailing coordinates, for the queries around the base v. Their full distance is
eps^2 = 0.04, their stage-1 score that of a row at distance ~0: the slot drops one of them, its bound cannot clear the query's best
full distance, and the split that holds the slot is unproven -- that split only: every other row is a natural row at distance
~1.4. Rows 16 m + 4 fq + j of a 128-row block share a lane slot in every tile shape of the ring kernel.

Base kinds (HALF = 4096 rows = one stage-1 split when the codebook is cut in two):
  c0, c1     cluster in half 0 / half 1 only                      -> in one list; the nearest row is the cluster's first
  c01        clusters in both halves                              -> in both lists
  far0, far1 cluster in half 0 (1), and ONE row u at 0.8 eps in the other half: the true neighbour lies in the half that is not
             searched again, stage 1's answer must survive the merge; k = 2 has one answer row in each half
  late       the slot's three rows are r1, r2 (trailing eps) and r3 = v + 0.1 (leading) + 0.1 (trailing): r3 is the true neighbour
             (distance^2 0.02 < 0.04) but has the worst stage-1 score of the three, so only stage 2 (T = 4) can find it
  tie        cluster in half 1, and two bit-identical rows u at 0.8 eps, one in each half: the lower row wins, k = 2 returns both
  six        six rows of one lane slot: stage 2's four candidates overflow too, and the slot goes to the exact scan
plus, in the larger data set, one query scaled by 400: its largest rotated coordinate is at least |q| / sqrt(128) = 40, beyond the
fixed f16 scale of the rotated images (2 |c|max = 2.5 at 2^13 .. 2^14, so 20 at most): no seed, unproven in every split. (The smaller
data set goes without: its stage 2 runs on the original f16 image, whose scale follows the batch.)

A third data set holds c01 bases only: every query built to fail fails in BOTH halves, the lists are made, would save nothing and
DECLINE, and the unsplit stage 2 follows them in the same call (test_lists_decline_and_the_unsplit_stage2_follows)."""
import numpy as np
import pytest

N_WORDS, NQ, DIM, M1, HALF = 8192, 8192, 352, 128, 4096
EPS = 0.2
KINDS = [("c0", 40), ("c1", 40), ("c01", 16), ("far0", 2), ("far1", 2), ("late", 2), ("tie", 2), ("six", 2)]
Q_BIG = NQ - 1


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def bare_cb(pkg, ctx, words):
    n = len(words)
    return pkg.capi.Codebook(ctx, words, np.arange(n + 1, dtype=np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32),
                             np.zeros(n, np.uint32), 1, np.ones(1, np.float32))


def natural(rng, n):
    scale = np.r_[np.geomspace(1.0, 0.1, M1), np.full(DIM - M1, 0.003)] / 5.0
    return (rng.standard_normal((n, DIM)) * scale).astype(np.float32)


def trailing(rng, length):
    """a vector of that length in the trailing coordinates only"""
    t = np.zeros(DIM)
    t[M1:] = rng.standard_normal(DIM - M1)
    return (length * t / np.linalg.norm(t)).astype(np.float32)


def slot_row(b, half, i):
    """i-th row (i < 28) of the lane slot base b owns in that half: tile b % 16 of the half, slot (wr, fq) = (b // 64, b // 16 % 4)"""
    return (16 * half + b % 16) * 256 + 128 * (b // 64) + 16 * (i // 4) + 4 * (b // 16 % 4) + i % 4


def single_row(b, half, j=0):
    """a row of the same slot, beyond the cluster rows"""
    return slot_row(b, half, 28 + j)


def make(per_base, big, kinds=KINDS):
    """words, queries, {kind: [(base, its queries, expected rows for k = 2)]}, number of queries built to fail (big: the scaled one too)"""
    rng = np.random.default_rng(2024)
    words = natural(rng, N_WORDS)
    q = np.zeros((NQ, DIM), np.float32)
    info, b, nfail, used = {}, 0, 0, set()
    for kind, count in kinds:
        for _ in range(count):
            v = natural(rng, 1)[0]
            def cluster(half, n, first=1.0):
                rows = [slot_row(b, half, i) for i in range(n)]
                used.update(rows)
                for i, r in enumerate(rows):
                    words[r] = v + trailing(rng, EPS * (first + 0.05 * i))
                return rows
            if kind in ("c0", "c1"):
                exp = cluster(int(kind[1]), 3)[:2]
            elif kind == "c01":
                exp = cluster(0, 3)[:2]; cluster(1, 3, first=1.5)
            elif kind in ("far0", "far1"):
                h = int(kind[3])
                rows = cluster(h, 3)
                u = single_row(b, 1 - h); words[u] = v + trailing(rng, 0.8 * EPS)
                exp = [u, rows[0]]
            elif kind == "late":
                rows = cluster(0, 2)
                r3 = slot_row(b, 0, 2)
                used.add(r3)
                lead = np.zeros(DIM, np.float32); lead[b % 8] = 0.1
                words[r3] = v + lead + trailing(rng, 0.1)
                exp = [r3, rows[0]]
            elif kind == "tie":
                cluster(1, 3)
                u = v + trailing(rng, 0.8 * EPS)
                words[single_row(b, 0)] = u; words[single_row(b, 1)] = u
                exp = [single_row(b, 0), single_row(b, 1)]
            elif kind == "six":
                exp = cluster(0, 6)[:2]
            used.update(single_row(b, h) for h in (0, 1))
            qs = np.arange(nfail, nfail + per_base)
            q[qs] = v
            info.setdefault(kind, []).append((b, qs, exp))
            nfail += per_base; b += 1
    assert nfail < Q_BIG and b <= 128
    free = np.setdiff1d(np.arange(N_WORDS), sorted(used))
    q[nfail:] = words[rng.choice(free, NQ - nfail, replace=False)]         # ordinary queries: an untouched codeword each, proven by stage 1
    q = (q + 1e-5 * rng.standard_normal(q.shape)).astype(np.float32)
    if big:
        q[Q_BIG] *= 400.0
    return words, q, info, nfail + int(big)


@pytest.fixture(scope="module")
def datasets():
    """46 queries per base: 4876 built to fail, stage 2 takes the ring; 8 per base: 848, the merged-splits kernel; both: 106 bases of
    kind c01 only, 4876 queries that fail in both halves, no scaled query"""
    return {"many": make(46, True), "few": make(8, False), "both": make(46, False, [("c01", 106)])}


def test_forced_rows_share_a_lane_slot_and_a_half():
    """(no GPU) the rows of a base lie in one lane slot of the 256-row and of the 128-row tile, in the half they are meant for"""
    for b in (0, 17, 63, 64, 105):
        for half in (0, 1):
            rows = [slot_row(b, half, i) for i in range(32)]
            assert len(set(rows)) == 32 and {r // HALF for r in rows} == {half}
            assert len({(r % 256 // 128, r % 16 // 4) for r in rows}) == 1 and len({r // 256 for r in rows}) == 1
    owners = {(slot_row(b, 0, 0) // 256, slot_row(b, 0, 0) % 256 // 128, slot_row(b, 0, 0) % 16 // 4) for b in range(128)}
    assert len(owners) == 128                                              # no two bases share a slot


_cache = {}


def search(pkg, dev, monkeypatch, name, words, q, env):
    """k = 1 and 2 on a fresh context (the switches are read when one is created); cached: the f32 reference of a data set is made once"""
    key = (name, tuple(sorted(env.items())))
    if key in _cache:
        return _cache[key]
    for var in ("ISMHIP_KNN_MODE", "ISMHIP_KNN_STAGE2_SPLITS", "ISMHIP_KNN_STAGE2_T4", "ISMHIP_KNN_SPLITS", "ISMHIP_KNN_PCA_M2"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("ISMHIP_KNN_PCA_M", str(M1))
    for var, v in env.items():
        monkeypatch.setenv(var, v)
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    if env.get("ISMHIP_KNN_MODE") != "f32":
        assert cb.stage1_dims == M1 and cb.stage1_energy < 1.0, (cb.stage1_dims, cb.stage1_energy)
        assert "ISMHIP_KNN_PCA_M2" not in env or cb.stage2_dims == int(env["ISMHIP_KNN_PCA_M2"])
    ctx.timers_enable(True)
    out = {}
    for k in (1, 2):
        idx, dist = pkg.capi.knn(ctx, cb, 0, T(q, dev), k)
        out[k] = dict(idx=idx.cpu().numpy(), dist=dist.cpu().numpy(), n2=int(ctx.timer("knn_stage2_queries")[0]),
                      entries=int(ctx.timer("knn_stage2_list_entries")[0]), items=int(ctx.timer("knn_flagged_items")[0]))
    out["ranged"] = int(ctx.timer("knn_stage2_ranged")[0])
    out["scans"] = int(ctx.timer("knn_fallback")[1])
    cb.close(); ctx.close()
    _cache[key] = out
    return out


CONFIGS = {
    # two stage-1 splits of 16 tiles; 4096 .. 32 767 list entries: the 128-row ring of stage 2
    "half-tile": ("many", {"ISMHIP_KNN_SPLITS": "2", "ISMHIP_KNN_PCA_M2": "192"}),
    # ... the 256-row ring
    "tile256": ("many", {"ISMHIP_KNN_SPLITS": "2", "ISMHIP_KNN_PCA_M2": "192", "ISMHIP_KNN_STAGE2_T4": "1"}),
    # fewer than 4096 entries: the merged-splits kernel
    "merged": ("few", {"ISMHIP_KNN_SPLITS": "2"}),
    # the planner's own cut of this launch: four stage-1 splits of 8 tiles, four lists
    "four-splits": ("many", {"ISMHIP_KNN_PCA_M2": "192"}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_split_lists_match_exact_route_and_unsplit_stage2(pkg, gpu, datasets, monkeypatch, cfg):
    _, dev = gpu
    name, env = CONFIGS[cfg]
    words, q, info, nfail = datasets[name]
    got = search(pkg, dev, monkeypatch, name, words, q, dict(env, ISMHIP_KNN_STAGE2_SPLITS="1"))
    off = search(pkg, dev, monkeypatch, name, words, q, dict(env, ISMHIP_KNN_STAGE2_SPLITS="0"))
    exact = search(pkg, dev, monkeypatch, name, words, q, {"ISMHIP_KNN_MODE": "f32"})
    n_lists = 2 if "ISMHIP_KNN_SPLITS" in env else 4
    both = sum(len(qs) for kind in ("c01",) for _, qs, _ in info[kind])
    for k in (1, 2):
        g, o, e = got[k], off[k], exact[k]
        print(f"{cfg} k={k}: stage-2 queries {g['n2']} (unsplit {o['n2']}), list entries {g['entries']}, exact-scan items {g['items']} (unsplit {o['items']})")
        assert np.array_equal(g["idx"], e["idx"]), f"rows differ from the f32 route in {int((g['idx'] != e['idx']).any(1).sum())} queries"
        assert np.array_equal(g["dist"].view(np.uint32), e["dist"].view(np.uint32))
        assert np.array_equal(g["idx"], o["idx"]) and np.array_equal(g["dist"].view(np.uint32), o["dist"].view(np.uint32))
        # what was built, found: first (and second) row of every base kind
        for kind, bases in info.items():
            for b, qs, exp in bases:
                assert (g["idx"][qs] == np.asarray(exp[:k])).all(), (kind, b, g["idx"][qs[0]], exp)
        b, qs, exp = info["tie"][0]
        if k == 2:
            assert (g["dist"][qs, 0].view(np.uint32) == g["dist"][qs, 1].view(np.uint32)).all()      # equal distance: the lower row first
        # the count of stage-2 queries keeps its meaning: distinct failing queries, however many lists they stand in
        assert g["n2"] == o["n2"] and nfail <= g["n2"] <= NQ, (g["n2"], o["n2"], nfail)
        assert o["entries"] == 0
        # a query stands once in the list of every split it failed in: the queries built to fail in both halves twice, the scaled one
        # in every list, nobody more often than there are lists
        big = (n_lists - 1) if name == "many" else 0
        assert g["n2"] + both + big <= g["entries"] <= n_lists * g["n2"], (g["entries"], g["n2"])
        if name == "many":
            assert g["entries"] >= 4096                                       # the ring path of stage 2 cannot have been skipped
            assert g["items"] >= 1                                            # the six-row slot overflowed stage 2's lists: exact scan
        else:
            assert g["entries"] + 256 * n_lists < 4096                        # padded to whole query tiles, still the merged-splits kernel
    assert got["ranged"] == 2 and off["ranged"] == 0, (got["ranged"], off["ranged"])
    assert got["scans"] == 2, got["scans"]                                    # ONE exact-scan launch per call


@pytest.mark.gpu
def test_lists_decline_and_the_unsplit_stage2_follows(pkg, gpu, datasets, monkeypatch):
    """Queries that failed in every split: the failure lists are built (entries > 0) but cover the whole sweep, so the saving rule
    declines them (ranged == 0) and the call goes on with the unsplit gather and stage 2. With two equal splits the rule declines when
    the padded entries x half the rows exceed 7/8 of n2 x all rows: entries * 4 >= 7 * n2 is the precondition (padding only adds)."""
    _, dev = gpu
    env = {"ISMHIP_KNN_SPLITS": "2", "ISMHIP_KNN_PCA_M2": "192"}
    words, q, info, nfail = datasets["both"]
    got = search(pkg, dev, monkeypatch, "both", words, q, dict(env, ISMHIP_KNN_STAGE2_SPLITS="1"))
    off = search(pkg, dev, monkeypatch, "both", words, q, dict(env, ISMHIP_KNN_STAGE2_SPLITS="0"))
    exact = search(pkg, dev, monkeypatch, "both", words, q, {"ISMHIP_KNN_MODE": "f32"})
    for k in (1, 2):
        g, o, e = got[k], off[k], exact[k]
        print(f"both k={k}: stage-2 queries {g['n2']} (unsplit {o['n2']}), list entries {g['entries']}, exact-scan items {g['items']} (unsplit {o['items']})")
        assert g["entries"] * 4 >= 7 * g["n2"], (g["entries"], g["n2"])       # the data set's precondition: the lists must decline
        assert g["entries"] > 0 and o["entries"] == 0                         # ... after they were built
        assert nfail <= g["n2"] == o["n2"], (g["n2"], o["n2"], nfail)
        assert np.array_equal(g["idx"], e["idx"]), f"rows differ from the f32 route in {int((g['idx'] != e['idx']).any(1).sum())} queries"
        assert np.array_equal(g["dist"].view(np.uint32), e["dist"].view(np.uint32))
        assert np.array_equal(g["idx"], o["idx"]) and np.array_equal(g["dist"].view(np.uint32), o["dist"].view(np.uint32))
        for b, qs, exp in info["c01"]:
            assert (g["idx"][qs] == np.asarray(exp[:k])).all(), (b, g["idx"][qs[0]], exp)
    assert got["ranged"] == 0 and off["ranged"] == 0, (got["ranged"], off["ranged"])

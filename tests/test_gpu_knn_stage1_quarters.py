"""Squared-L2 search with the codebook cut into FOUR splits (ISMHIP_KNN_SPLITS=4) and the ring kernel's block -> (query tile, split)
map with the split as the fast or the slow index (ISMHIP_KNN_SPLIT_MAJOR=0 | 1). Neither may change an answer: rows and distances
are the oracle's exact `knn`, element for element, whatever the cut and the map.

Dimension 352, steep spectrum (the data of tests/test_gpu_knn_stage2_splits.py), rotated image forced to 128 coordinates.

Two sizes:
  small  1 024 / 1 280 words x 300 / 40 queries, K = 1 and 4. Launches below 4 096 queries or words take the single-stage search on
         the 128-row tile kernel (knn.hip, ismhip_knn): the split count is forced the same way, a proof that fails sends the query
         to the exact scan (`knn_flagged_queries`) and `knn_stage2_queries` stays 0. 1 280 words are ten tiles: splits of 3, 3, 3, 1;
         eight splits asked for clamp to what the candidate slots hold.
  ring   4 352 words (17 tiles of 256: quarters of 5, 5, 5, 2) x 4 396 queries (17 full query tiles and a ragged one), K = 1 and 2:
         the two-stage search, stage 1 on k_knn_l2_ring16 with four splits, stage 2 on one failure list per quarter.

Failures are planted without reference to any lane-slot map: a block of 64 consecutive rows of ONE quarter holds 64 bit-identical
copies of a vector v, and the planted queries are v plus noise of 1e-5. A split has at most 8 lane slots of at most T = 4 candidates,
so at most 32 of the 64 copies fit its lists: some slot drops a copy, its bound equals the best distance and cannot clear it
(pigeonhole; test_planted_rows_overflow_their_quarter_only checks the counts in float64). The other quarters hold natural rows at
distance^2 ~ 1 from v against ~ 4e-8 for the copies: they are proven. Ties go to the lowest row, as in the oracle.
Kinds: `one` = a block in quarter 2; `all` = one vector with a block in every quarter (the lists then save nothing and the unsplit
stage 2 runs); `mixed` = four vectors: blocks in quarter 0, in quarter 2, in quarters 1 and 3, in every quarter.
5 queries per vector in the small launches; 256 in the ring launches, where a failure list is padded to whole groups of 256 queries
and fewer entries would make every list decline.
What is asserted about counts. K = 1: the nearest row of an ordinary query is its own codeword at distance^2 ~ 4e-8, every other row
lies at ~ 1: its proofs hold in every split, so exactly the planted queries fail, each in exactly the quarters it was planted in.
K > 1: an ordinary query's K-th and (K+1)-th rows are natural rows whose distances may differ by less than the f16 error bound, so
more queries may fail: at least the planted ones."""
import numpy as np
import pytest

DIM, M1, BLOCK = 352, 128, 64
KINDS = {"none": [], "one": [(2,)], "all": [(0, 1, 2, 3)], "mixed": [(0,), (2,), (1, 3), (0, 1, 2, 3)]}


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


def quarters(n_words, tile):
    """row ranges of the four splits: whole tiles, dealt as knn_plan deals them (ceil(tiles / 4) each, the last one short)"""
    n_t = (n_words + tile - 1) // tile
    tps = (n_t + 3) // 4
    return [(s * tps * tile, min(n_words, (s + 1) * tps * tile)) for s in range(4) if s * tps * tile < n_words]


_data = {}


def make(n_words, nq, tile, kind, per=5):
    """words, queries, [(planted queries, quarters, expected rows ascending)], number of planted queries"""
    key = (n_words, nq, tile, kind, per)
    if key in _data:
        return _data[key]
    rng = np.random.default_rng(77)
    words = natural(rng, n_words)
    qr = quarters(n_words, tile)
    assert len(qr) == 4
    q = np.zeros((nq, DIM), np.float32)
    used = np.zeros(n_words, bool)
    info, n_planted, nxt = [], 0, [lo for lo, _ in qr]
    for where in KINDS[kind]:
        v = natural(rng, 1)[0]
        rows = []
        for s in where:
            assert nxt[s] + BLOCK <= qr[s][1], "quarter too short for another block"
            words[nxt[s]:nxt[s] + BLOCK] = v
            used[nxt[s]:nxt[s] + BLOCK] = True
            rows += list(range(nxt[s], nxt[s] + BLOCK))
            nxt[s] += BLOCK
        qs = np.arange(n_planted, n_planted + per)
        q[qs] = v
        info.append((qs, where, sorted(rows)))
        n_planted += per
    free = np.nonzero(~used)[0]
    pick = rng.choice(free, nq - n_planted, replace=len(free) < nq - n_planted)
    q[n_planted:] = words[pick]                                              # ordinary queries: an untouched codeword each
    q = (q + 1e-5 * rng.standard_normal(q.shape)).astype(np.float32)
    _data[key] = (words, q, info, n_planted)
    return _data[key]


@pytest.mark.parametrize("n_words,nq,tile,kind", [(1024, 300, 128, "mixed"), (1280, 300, 128, "mixed"), (4352, 4396, 256, "mixed"),
                                                  (1024, 40, 128, "mixed"), (1024, 300, 128, "all"), (4352, 4396, 256, "one")])
def test_planted_rows_overflow_their_quarter_only(n_words, nq, tile, kind):
    """(no GPU) float64: a planted query has, in each quarter it is planted in, more rows at or below its 4th best distance than the 32
    candidates that 8 slots x 4 hold, and none within 1000x that distance in any other quarter; ordinary queries have one near row"""
    words, q, info, n_planted = make(n_words, nq, tile, kind, 256 if tile == 256 else 5)
    w64 = words.astype(np.float64)
    qr = quarters(n_words, tile)
    def dist2(i):
        return ((w64 - q[i].astype(np.float64)) ** 2).sum(1)
    for qs, where, rows in info:
        for i in qs[::51]:
            d = dist2(i)
            dk = np.sort(d)[3]
            for s, (lo, hi) in enumerate(qr):
                near = int((d[lo:hi] <= dk).sum())
                if s in where:
                    assert near > 32, (i, s, near)
                else:
                    assert int((d[lo:hi] <= 1000.0 * dk).sum()) == 0, (i, s)
    for i in range(n_planted, nq, 37):
        d = np.sort(dist2(i))
        assert d[0] < 1e-6 and d[1] > 0.1, (i, d[:2])


def search(pkg, dev, monkeypatch, words, q, ks, env):
    for var in ("ISMHIP_KNN_MODE", "ISMHIP_KNN_STAGE2_SPLITS", "ISMHIP_KNN_STAGE2_T4", "ISMHIP_KNN_SPLITS", "ISMHIP_KNN_PCA_M2", "ISMHIP_KNN_SPLIT_MAJOR"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("ISMHIP_KNN_PCA_M", str(M1))
    for var, v in env.items():
        monkeypatch.setenv(var, v)
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    ctx.timers_enable(True)
    out = {}
    for k in ks:
        idx, dist = pkg.capi.knn(ctx, cb, 0, T(q, dev), k)
        out[k] = dict(idx=idx.cpu().numpy().reshape(len(q), k), dist=dist.cpu().numpy().reshape(len(q), k),
                      n2=int(ctx.timer("knn_stage2_queries")[0]), entries=int(ctx.timer("knn_stage2_list_entries")[0]),
                      flagged=int(ctx.timer("knn_flagged_queries")[0]), ranged=int(ctx.timer("knn_stage2_ranged")[0]) - sum(o["ranged"] for o in out.values()))
    out["stage1_dims"] = cb.stage1_dims
    cb.close(); ctx.close()
    return out


_oracle = {}


def exact(ora, key, words, q, k):
    if (key, k) not in _oracle:
        idx, dist = ora.knn(0, words, q, k)
        _oracle[(key, k)] = (np.asarray(idx).reshape(len(q), k), np.asarray(dist).reshape(len(q), k))
    return _oracle[(key, k)]


def check_answers(got, want, info, k):
    wi, wd = want
    assert np.array_equal(got["idx"], wi), f"rows differ from the oracle in {int((got['idx'] != wi).any(1).sum())} queries"
    assert np.array_equal(got["dist"].view(np.uint32), wd.view(np.uint32))
    for qs, where, rows in info:                                             # ties: the k lowest copies
        assert (got["idx"][qs] == np.asarray(rows[:k])).all(), (where, got["idx"][qs[0]], rows[:k])


@pytest.mark.gpu
@pytest.mark.parametrize("n_words,nq,splits,kind", [
    pytest.param(1024, 300, "4", "none", id="1024w-none"),
    pytest.param(1024, 300, "4", "one", id="1024w-one-quarter"),
    pytest.param(1024, 300, "4", "all", id="1024w-all-quarters"),
    pytest.param(1280, 300, "4", "mixed", id="1280w-uneven"),
    pytest.param(1280, 300, "8", "mixed", id="1280w-clamped"),
    pytest.param(1024, 40, "4", "mixed", id="40-queries"),
])
def test_four_splits_small_launch(pkg, gpu, ora, monkeypatch, n_words, nq, splits, kind):
    """the single-stage search below 4 096 queries: K = 1 and 4, oracle-equal; the planted queries, and nobody else, reach the exact scan"""
    _, dev = gpu
    words, q, info, n_planted = make(n_words, nq, 128, kind)
    got = search(pkg, dev, monkeypatch, words, q, (1, 4), {"ISMHIP_KNN_SPLITS": splits})
    for k in (1, 4):
        g = got[k]
        print(f"{n_words} words x {nq} queries, splits {splits}, {kind}, k={k}: stage-2 queries {g['n2']}, exact-scan queries {g['flagged']} (planted {n_planted})")
        check_answers(g, exact(ora, (n_words, nq, 128, kind), words, q, k), info, k)
        assert g["n2"] == 0
        assert g["flagged"] == n_planted if k == 1 else n_planted <= g["flagged"] <= nq, (g["flagged"], n_planted)


@pytest.mark.gpu
@pytest.mark.parametrize("major", ["0", "1"])
@pytest.mark.parametrize("kind", ["none", "one", "all", "mixed"])
def test_four_stage1_splits_ring(pkg, gpu, ora, monkeypatch, kind, major):
    """the two-stage search: four stage-1 quarters of 5, 5, 5 and 2 tiles, K = 1 and 2, both block maps. Stage 2 gets exactly the planted
    queries, each once per quarter it was planted in; a query planted in every quarter makes the lists decline"""
    _, dev = gpu
    n_words, nq = 4352, 4396
    words, q, info, n_planted = make(n_words, nq, 256, kind, 256)
    got = search(pkg, dev, monkeypatch, words, q, (1, 2), {"ISMHIP_KNN_SPLITS": "4", "ISMHIP_KNN_SPLIT_MAJOR": major})
    assert got["stage1_dims"] == M1
    n_entries = sum(len(qs) * len(where) for qs, where, _ in info)
    for k in (1, 2):
        g = got[k]
        print(f"ring, {kind}, split-major {major}, k={k}: stage-2 queries {g['n2']} (planted {n_planted}), list entries {g['entries']} (planted {n_entries}), exact-scan queries {g['flagged']}")
        check_answers(g, exact(ora, (n_words, nq, 256, kind), words, q, k), info, k)
        if k == 1:
            assert g["n2"] == n_planted and g["entries"] == n_entries, (g["n2"], n_planted, g["entries"], n_entries)
            # lists that cover less than 7/8 of the unsplit sweep are taken (run_knn_stage2_lists): every kind but `all`
            assert g["ranged"] == (0 if kind in ("none", "all") else 1), g["ranged"]
        else:
            assert n_planted <= g["n2"] <= nq and g["entries"] >= n_entries, (g["n2"], n_planted, g["entries"], n_entries)
        assert g["flagged"] <= max(g["n2"], g["entries"])                    # the scan counts a query once per list it stands in


@pytest.mark.gpu
def test_four_stage1_splits_with_prepass(pkg, gpu, ora, monkeypatch):
    """>= 128 codeword tiles, 96 rotated coordinates: the sampling pre-pass starts the four-split stage 1 (its LDS comes from its own
    layout, not the main kernel's). Oracle-equal on a sample of the queries. Stage-2 queries on this input, measured on the parent
    commit with the same four splits: 8 (K = 1) and 49 (K = 2); with three splits 17 and 88, with two 29 and 177. Where a workgroup
    joins its split's codeword stream depends on timing, so which rows a slot drops, and with it the count, may move from run to run:
    the bound is twice the parent's count. A pre-pass reading thresholds from beyond its LDS fails proofs by the thousand."""
    _, dev = gpu
    rng = np.random.default_rng(99)
    n_words, nq = 32768 + 100, 4096 + 200
    basis = rng.random((40, DIM)).astype(np.float32)                         # a low-rank part + small isotropic noise, unit length
    def draw(n):
        x = rng.random((n, 40)).astype(np.float32) ** 3 @ basis + 0.005 * rng.random((n, DIM)).astype(np.float32)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    words, q = draw(n_words), draw(nq)
    q[:8] = words[:8]
    q[9] *= 40.0
    sel = np.r_[0:16, 16:nq:8]
    for var in ("ISMHIP_KNN_MODE", "ISMHIP_KNN_PCA_M2", "ISMHIP_KNN_SPLIT_MAJOR", "ISMHIP_KNN_PREPASS"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("ISMHIP_KNN_PCA_M", "96"); monkeypatch.setenv("ISMHIP_KNN_SPLITS", "4")
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    assert cb.stage1_dims == 96
    ctx.timers_enable(True)
    for k in (1, 2):
        idx, dist = pkg.capi.knn(ctx, cb, 0, T(q, dev), k)
        n2 = int(ctx.timer("knn_stage2_queries")[0])
        print(f"pre-pass, four splits, k={k}: stage-2 queries {n2}")
        wi, wd = ora.knn(0, words, q[sel], k)
        assert np.array_equal(idx.cpu().numpy()[sel].reshape(len(sel), k), np.asarray(wi).reshape(len(sel), k))
        assert np.array_equal(dist.cpu().numpy()[sel].reshape(len(sel), k), np.asarray(wd).reshape(len(sel), k))
        assert 1 <= n2 <= 2 * {1: 8, 2: 49}[k], n2
    cb.close(); ctx.close()

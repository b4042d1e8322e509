"""The score-insertion path of k_knn_l2_ring16's epilogue: the walk of a flagged column starts from the group
maxima the scan leaves, a wave swaps and publishes the thresholds only of a column it has just inserted into, and the partner wave
row's thresholds are read at the top of the next epilogue. None of that may change an answer: on codebooks that make the path as
busy as it gets, indices and distances are those of the exact-f32 route (ISMHIP_KNN_MODE=f32) bit for bit for every query, and the
oracle's on every 16th. 4 096 (+ 37) queries x 32 768 words x 352 dimensions with a steep spectrum, stage 1 on 128 rotated
coordinates: the smallest launch that takes the 256 x 256 tile with the resident query panel AND the sampling pre-pass (128 tiles).

Rows of a tile, as the kernel sees them: row = 128 wr + 16 mt + 4 fq + j; the lane slot (wr, fq) of a query column keeps ONE
candidate list per codebook split, fed by its 32 rows (mt = 0..7, j = 0..3) of every tile of the split. With 16 query tiles the
planner cuts the 128 codeword tiles into 4 splits of 32."""
import numpy as np
import pytest

N_WORDS, NQ, DIM, M1 = 32768, 4096, 352, 128
N_TILES, TILES_PER_SPLIT = N_WORDS // 256, 32
EXTRA = 37                                   # the second batch ends in a partial query tile
# the special rows of the "special" codebook, one tile each (splits 1, 2, 3)
TILE_ONE_SLOT, TILE_SPREAD, TILE_GROUP = 40, 70, 100
Q_ONE_SLOT, Q_SPREAD, Q_GROUP, Q_BIG, Q_TINY = 20, 21, 22, 23, 24


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def bare_cb(pkg, ctx, words):
    n = len(words)
    return pkg.capi.Codebook(ctx, words, np.arange(n + 1, dtype=np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32),
                             np.zeros(n, np.uint32), 1, np.ones(1, np.float32))


def steep_draw(rng, basis, n, noise=0.65):
    """descriptor-like vectors: a low-rank part + isotropic noise, non-negative, unit length (the pattern of the rotated stage-1
    tests; at this noise 128 coordinates hold 99.92 % of the second moment, so the image IS truncated -- with the 0.005 of the
    pre-pass inputs there the kept share rounds to 1 and the planner leaves the pre-pass out -- and a good part of the stage-1 proofs
    fails, so stage 2 and its seeds run on these answers too)"""
    x = rng.random((n, basis.shape[0])).astype(np.float32) ** 3 @ basis + noise * rng.random((n, basis.shape[1])).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def slot_rows(tile, wr, fq):
    """the 32 rows of lane slot (wr, fq) in a tile, ascending"""
    return np.asarray([tile * 256 + 128 * wr + 16 * mt + 4 * fq + j for mt in range(8) for j in range(4)])


def one_slot_rows():
    """40 rows of ONE lane slot: a tile holds only 32 rows of a slot, so all 32 of slot (1, 2) in one tile and the slot's first 8 in
    the next tile of the same split -- one candidate list meets 40 equal scores"""
    return np.r_[slot_rows(TILE_ONE_SLOT, 1, 2), slot_rows(TILE_ONE_SLOT + 1, 1, 2)[:8]]


def spread_rows():
    """40 rows spread over all eight lane slots of one tile, five each"""
    return np.sort(np.concatenate([slot_rows(TILE_SPREAD, wr, fq)[:5] for wr in range(2) for fq in range(4)]))


def group_rows():
    """the four rows of ONE 4-row group (mt = 3, fq = 1), in both wave rows of the same tile"""
    return np.asarray([TILE_GROUP * 256 + 128 * wr + 16 * 3 + 4 * 1 + j for wr in range(2) for j in range(4)])


def make_ordered():
    """Case 1: every tile of a sweep holds a better row than all tiles before it, for (nearly) every query. The queries sit in a small
    ball around one centre c; the words are ranked by their distance to c, worst first, and dealt out to the four splits in turn, each
    split in rank order. A workgroup sweeps ONE split, so every one of its tiles brings a new best row; the pre-pass samples the first
    (worst) tile of every split, so its start thresholds do not shield any tile."""
    rng = np.random.default_rng(7)
    basis = rng.random((40, DIM)).astype(np.float32)
    words = steep_draw(rng, basis, N_WORDS)
    c = steep_draw(rng, basis, 1)[0]
    d = ((words.astype(np.float64) - c) ** 2).sum(1)
    rank = np.argsort(-d, kind="stable")                                   # worst first
    r = np.arange(N_WORDS)
    pos = (r % 4) * (N_WORDS // 4) + r // 4
    out = np.empty_like(words)
    out[pos] = words[rank]
    q = c[None, :] + 1e-2 * rng.standard_normal((NQ, DIM)).astype(np.float32) / np.sqrt(DIM).astype(np.float32)
    q = np.abs(q); q[0] = c
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return out, q


def make_special():
    """Cases 2-4 in one codebook: the equal rows, the full 4-row groups, the overflowing and the tiny query"""
    rng = np.random.default_rng(11)
    basis = rng.random((40, DIM)).astype(np.float32)
    words = steep_draw(rng, basis, N_WORDS)
    q = steep_draw(rng, basis, NQ + EXTRA)
    v = steep_draw(rng, basis, 3)
    words[one_slot_rows()] = v[0]
    words[spread_rows()] = v[1]
    q[Q_ONE_SLOT] = v[0]                                                    # 40 rows at distance zero: the lowest one wins
    q[Q_SPREAD] = v[1] + (1e-4 * rng.random(DIM)).astype(np.float32)        # 40 rows at one non-zero distance
    for i, row in enumerate(group_rows()):                                  # eight near rows at eight different distances
        words[row] = v[2] + ((i + 1) * 2e-3 * rng.random(DIM)).astype(np.float32)
        words[row] /= np.linalg.norm(words[row])
    q[Q_GROUP] = v[2]
    q[Q_BIG] *= 40.0                                                        # beyond the fixed query scale of the rotated image
    q[Q_TINY] *= 1e-6
    return words, q


def check_inputs(ora, name, words, q, tied):
    """CPU check of the inputs: the exact search alone answers every query without a tie for the first two places, except the
    intended ones (tied: {query: its equal rows, ascending}); returns the share of (query, tile) pairs of the sweeps in which the
    tile brings a new best row"""
    wn = (words.astype(np.float64) ** 2).sum(1).astype(np.float32)        # (float32 is enough to FIND the close pairs: they go to the oracle)
    new_best, pairs, close = 0, 0, []
    for a in range(0, len(q), 1024):
        qq = q[a:a + 1024]
        D = wn[None, :] - 2.0 * (qq / np.maximum(np.linalg.norm(qq, axis=1, keepdims=True), 1e-30)) @ words.T     # order of |q/|q|| - w|^2
        part = np.partition(D, 1, axis=1)[:, :2]
        close += [a + i for i in np.nonzero(part[:, 1] - part[:, 0] < 1e-4)[0]]
        tmin = D.reshape(len(qq), 4, TILES_PER_SPLIT, 256).min(3)
        run = np.minimum.accumulate(tmin, axis=2)
        new_best += int((tmin[:, :, 1:] < run[:, :, :-1]).sum()); pairs += tmin[:, :, 1:].size
    close = sorted(set(close) | set(tied))
    idx, dist = ora.knn(0, words, q[close], 2)
    for i, qi in enumerate(close):
        if qi in tied:
            assert list(idx[i]) == list(tied[qi][:2]) and dist[i, 0] == dist[i, 1], (name, qi, idx[i], dist[i])
        else:
            assert dist[i, 0] != dist[i, 1], (name, qi, idx[i], dist[i])
    return new_best / pairs


@pytest.fixture(scope="module")
def cases(ora):
    """both codebooks with their queries, checked on the CPU, and the oracle's answers on the special queries + every 16th: made once"""
    out = {}
    for name, (words, q) in (("ordered", make_ordered()), ("special", make_special())):
        tied = {Q_ONE_SLOT: one_slot_rows(), Q_SPREAD: spread_rows()} if name == "special" else {}
        share = check_inputs(ora, name, words, q, tied)
        print(f"{name}: a tile of a sweep brings a new best row in {share:.3f} of the (query, tile) pairs")
        if name == "ordered":
            assert share > 0.95, share                                      # the construction holds for the batch, not only for its centre
        sel = np.r_[0:32, 32:len(q):16]
        out[name] = (words, q, sel, {k: ora.knn(0, words, q[sel], k) for k in (1, 2)})
    return out


def test_inputs_are_answered_without_unintended_ties(cases):
    """(no GPU) the fixture's CPU checks, and the special rows are where the docstring says: 40 rows in one lane slot, 40 over all
    eight, a whole 4-row group in both wave rows"""
    words, q, _, ref = cases["special"]
    slot = lambda r: ((r % 256) // 128, (r % 16) // 4)
    assert len(one_slot_rows()) == 40 and {slot(r) for r in one_slot_rows()} == {(1, 2)}
    assert {r // 256 // TILES_PER_SPLIT for r in one_slot_rows()} == {TILE_ONE_SLOT // TILES_PER_SPLIT}
    assert len(spread_rows()) == 40 and all(sum(slot(r) == s for r in spread_rows()) == 5 for s in [(a, b) for a in range(2) for b in range(4)])
    g = group_rows()
    assert len(g) == 8 and {r % 128 // 4 for r in g} == {13} and {r // 256 for r in g} == {TILE_GROUP}
    assert ref[1][0][Q_ONE_SLOT, 0] == one_slot_rows()[0] and ref[1][0][Q_SPREAD, 0] == spread_rows()[0]
    assert ref[2][0][Q_GROUP].tolist() == [g[0], g[1]]


def search(pkg, dev, monkeypatch, words, q, mode, ks, runs=1):
    """{k: (idx, dist, [stage-2 queries of every run])} on a fresh context (the switches are read when one is created)"""
    monkeypatch.setenv("ISMHIP_KNN_MODE", mode)
    monkeypatch.setenv("ISMHIP_KNN_PCA_M", str(M1))
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    if mode == "f16":
        assert cb.stage1_dims == M1 and cb.stage1_energy < 1.0, (cb.stage1_dims, cb.stage1_energy)
    ctx.timers_enable(True)
    out = {}
    for k in ks:
        n2 = []
        for _ in range(runs):
            idx, dist = pkg.capi.knn(ctx, cb, 0, T(q, dev), k)
            gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
            n2.append(int(ctx.timer("knn_stage2_queries")[0]))
        out[k] = (gi, gd, n2)
    if mode == "f16":
        assert int(ctx.timer("knn_pca_launches")[0]) >= runs * len(ks)      # every search ran stage 1 on the rotated image (stage 2 may add one)
    cb.close(); ctx.close()
    return out


def compare(name, got, exact, sel, ref):
    for k, (gi, gd, n2) in got.items():
        ei, ed, _ = exact[k]
        print(f"{name} k={k}: stage-2 queries per run {n2}")
        assert np.array_equal(gi, ei), f"{name} k={k}: rows differ from the f32 route in {int((gi != ei).any(1).sum())} queries"
        assert np.array_equal(gd.view(np.uint32), ed.view(np.uint32))
        assert np.array_equal(gi[sel], ref[k][0]) and np.array_equal(gd[sel].view(np.uint32), ref[k][1].view(np.uint32))
        assert len(set(n2)) == 1, n2                                        # the bounds do not depend on how the waves ran


@pytest.mark.gpu
def test_every_tile_of_a_sweep_hits(pkg, gpu, cases, monkeypatch):
    """Case 1: rows ordered so that every tile of a workgroup's sweep brings a better row than all before it: the insertion path runs
    in every tile for every query column, and every insertion raises a threshold that the partner wave row has to pick up."""
    _, dev = gpu
    words, q, sel, ref = cases["ordered"]
    got = search(pkg, dev, monkeypatch, words, q, "f16", (1,), runs=2)
    exact = search(pkg, dev, monkeypatch, words, q, "f32", (1,))
    compare("ordered", got, exact, sel, ref)
    assert got[1][0][0, 0] == N_WORDS - 1                                  # the centre's nearest row is the last one dealt


@pytest.mark.gpu
def test_equal_rows_full_groups_and_scale_extremes(pkg, gpu, cases, monkeypatch):
    """Cases 2-4, k = 1 and 2, 4 096 + 37 queries (a partial last query tile). 40 equal rows in one lane slot and 40 over all eight
    slots of a tile overflow the candidate lists: ties go to the lowest row. All four rows of a 4-row group above the threshold at
    once, in both wave rows of one tile: every one of them is walked. A query 40x beyond the fixed scale of the rotated image and a
    1e-6-scaled one get the exact answers like everybody else."""
    _, dev = gpu
    words, q, sel, ref = cases["special"]
    got = search(pkg, dev, monkeypatch, words, q, "f16", (1, 2), runs=2)
    exact = search(pkg, dev, monkeypatch, words, q, "f32", (1, 2))
    compare("special", got, exact, sel, ref)
    g = group_rows()
    assert got[1][0][Q_ONE_SLOT, 0] == one_slot_rows()[0] and got[1][0][Q_SPREAD, 0] == spread_rows()[0]
    assert got[2][0][Q_ONE_SLOT].tolist() == one_slot_rows()[:2].tolist() and got[2][0][Q_SPREAD].tolist() == spread_rows()[:2].tolist()
    assert got[2][0][Q_GROUP].tolist() == [g[0], g[1]]
    assert all(n >= 1 for n in got[1][2])                                   # at least the overflowing query went to stage 2

"""Stage 2 of the two-stage squared-L2 search started from stage 1's answer (k_knn_seed_thr): every lane slot of a
stage-2 query begins at the threshold its stage-1 k-th exact distance allows instead of -inf. Seeds may only save work: answers stay
the oracle's bit for bit (FLANN exact search, ties to the lowest row), on both stage-2 images and both ring tiles, for queries whose
seed is zero, cannot be formed (overflowing image row, NaN) or is undercut by more equal rows than a slot keeps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WORDS, NQ, DIM = 8192 + 100, 9000, 352
NOISE = 0.65         # isotropic part of the rows: with 64 of 352 rotated coordinates in stage 1, more than half of the proofs fail
CLUSTER = 2048 + 8   # first row of six bit-identical rows inside ONE lane slot of its tile (both tile shapes, stage 1 and stage 2)
Q_EXACT, Q_DUP, Q_BIG, Q_TINY, Q_NAN, Q_CLUSTER = slice(0, 8), 8, 9, 10, 11, slice(12, 16)


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def bare_cb(pkg, ctx, words):
    n = len(words)
    return pkg.capi.Codebook(ctx, words, np.arange(n + 1, dtype=np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32),
                             np.zeros(n, np.uint32), 1, np.ones(1, np.float32))


def steep_spectrum_data(rng, n_words, nq, dim, rank=40, noise=0.02):
    """descriptor-like vectors: a low-rank part + isotropic noise, non-negative, unit length"""
    basis = rng.random((rank, dim)).astype(np.float32)
    def draw(n):
        x = rng.random((n, rank)).astype(np.float32) ** 3 @ basis + noise * rng.random((n, dim)).astype(np.float32)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return draw(n_words), draw(nq)


@pytest.fixture(scope="module")
def data(ora):
    """codebook, queries, the checked rows (the special queries and every 4th) and the oracle's answers for k = 1, 2: made once"""
    rng = np.random.default_rng(99)
    words, q = steep_spectrum_data(rng, N_WORDS, NQ, DIM, noise=NOISE)
    words[4000:4003] = words[17]                                          # duplicates: ties to the lowest row
    rows = np.asarray([CLUSTER + 16 * (i // 4) + (i % 4) for i in range(6)])
    words[rows] = words[CLUSTER]                                          # more equal rows in one lane slot than any candidate list keeps
    q[Q_EXACT] = words[:8]                                                # a query equal to a codeword: seed distance 0
    q[Q_DUP] = words[17]
    q[Q_BIG] *= 40.0                                                      # beyond the fixed query scale of the rotated images: no seed
    q[Q_TINY] *= 1e-6
    q[Q_NAN, 5] = np.nan
    q[Q_CLUSTER] = words[CLUSTER] + (1e-4 * rng.random((4, DIM))).astype(np.float32)
    sel = np.r_[0:11, 12:16, 16:NQ:4]                                     # (a NaN query has no defined order: compared between the two starts only)
    ref = {k: ora.knn(0, words, q[sel], k) for k in (1, 2)}
    return words, q, sel, ref


def search(pkg, dev, monkeypatch, words, q, env):
    """k = 1 and k = 2 on a fresh context (the switches are read when one is created): [(idx, dist, stage-2 queries, scan items)] and the
    number of candidate launches that started from seeds"""
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    assert cb.stage1_dims == 64 and cb.stage2_dims == int(env["ISMHIP_KNN_PCA_M2"])
    ctx.timers_enable(True)
    out = []
    for k in (1, 2):
        idx, dist = pkg.capi.knn(ctx, cb, 0, T(q, dev), k)
        gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
        out.append((gi, gd, int(ctx.timer("knn_stage2_queries")[0]), int(ctx.timer("knn_flagged_items")[0])))
    seed_launches = int(ctx.timer("knn_seed_launches")[0])
    cb.close(); ctx.close()
    return out, seed_launches


@pytest.mark.parametrize("t4", ["0", "1"], ids=["half-tile", "tile256"])
@pytest.mark.parametrize("m2", ["192", "0"], ids=["rotated192", "f16-original"])
def test_seeded_stage2_matches_oracle_and_cold_start(pkg, gpu, ora, data, monkeypatch, m2, t4):
    """Stage 1 on 64 rotated coordinates leaves 4096 .. nq queries to stage 2, which therefore runs the ring kernel: on the second
    rotated image (lower-bound proof) or the original f16 image (thr_tau_of model), on the 128 x 256 tile or (ISMHIP_KNN_STAGE2_T4=1)
    the 256 x 256 one. Answers: the oracle's for k = 1, 2, and the arrays of the cold start (ISMHIP_KNN_STAGE2_SEED=0) byte for byte,
    the NaN query included. The six equal rows in one slot overflow every candidate list, so the exact scan must have run; seeds
    that hold never add exact-scan items (the bounds a search reports do not depend on how its waves ran, so the two counts can be
    compared as they are). Seeding must have run: one seeded candidate launch per search, none from the cold start."""
    _, dev = gpu
    words, q, sel, ref = data
    env = {"ISMHIP_KNN_PCA_M": "64", "ISMHIP_KNN_PCA_M2": m2, "ISMHIP_KNN_STAGE2_T4": t4}
    seeded, n_seeded = search(pkg, dev, monkeypatch, words, q, dict(env, ISMHIP_KNN_STAGE2_SEED="1"))
    cold, n_cold = search(pkg, dev, monkeypatch, words, q, dict(env, ISMHIP_KNN_STAGE2_SEED="0"))
    assert (n_seeded, n_cold) == (2, 0), (n_seeded, n_cold)              # one stage-2 chunk per search took k_knn_seed_thr's thresholds
    for k, (gi, gd, n2, items), (ci, cd, cn2, citems) in zip((1, 2), seeded, cold):
        print(f"m2={m2} t4={t4} k={k}: stage-2 queries {n2}, exact-scan items seeded {items} cold {citems}")
        assert 4096 <= n2 < NQ and 4096 <= cn2 < NQ, (n2, cn2)            # the ring path of stage 2 cannot have been skipped
        widx, wdist = ref[k]
        assert np.array_equal(gi[sel], widx), f"rows differ in {int((gi[sel] != widx).any(1).sum())} queries"
        assert np.array_equal(gd[sel].view(np.uint32), wdist.view(np.uint32))
        assert np.array_equal(gi, ci) and np.array_equal(gd, cd, equal_nan=True)
        assert gi[Q_DUP, 0] == 17 and (gi[Q_CLUSTER, 0] == CLUSTER).all()   # ties: the lowest row
        assert items >= 1                                                 # the overflowing slot went to the exact scan
        assert items <= citems, (items, citems)

"""Threshold activation (ActivationStrategyThreshold, activation_strategy_threshold.cpp:27-44) on the device: the radius search
ismhip_knn_threshold, vote casting over its lists (ismhip_cast_votes_csr) and training over them (ismhip_train_activate_lists),
against the CPU oracle: ora.knn(metric, words, q, k=n_words) lists every exact functor value; the activation set is d < threshold,
re-sorted by row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def T(a, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def bare_cb(pkg, ctx, words):
    n = len(words)
    return pkg.capi.Codebook(ctx, words, np.arange(n + 1, dtype=np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32),
                             np.zeros(n, np.uint32), 1, np.ones(1, np.float32))


def descriptors(rng, n, dim, rank=24, noise=0.3, unit=True):
    """descriptor-like rows: a shared low-rank part plus noise; non-negative. unit: L2-normalised (SHOT), else summing to 1 (histograms)"""
    basis = rng.random((rank, dim)).astype(np.float32)
    x = (rng.random((n, rank)).astype(np.float32) ** 3) @ basis + noise * rng.random((n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True) if unit else x.sum(axis=1, keepdims=True)
    return x.astype(np.float32)


def oracle_lists(ora, metric, words, q, thr):
    """per query: (rows ascending, exact functor values) with value < thr"""
    idx, dist = ora.knn(metric, words, q, len(words))
    out = []
    for i in range(len(q)):
        m = dist[i] < np.float32(thr)
        r, d = idx[i][m], dist[i][m]
        o = np.argsort(r, kind="stable")
        out.append((r[o].astype(np.int32), d[o]))
    return out


def check_lists(off, idx, dist, want, rows=None):
    rows = range(len(want)) if rows is None else rows
    idx = idx.cpu().numpy() if idx is not None else np.zeros(0, np.int32)
    dist = dist.cpu().numpy() if dist is not None else np.zeros(0, np.float32)
    for j, i in enumerate(rows):
        a, b = off[i], off[i + 1]
        assert np.array_equal(idx[a:b], want[j][0]), f"query {i}: rows differ"
        assert np.array_equal(dist[a:b].view(np.uint32), want[j][1].view(np.uint32)), f"query {i}: distances not bit-equal"


def thresholds_for(ora, metric, words, q, means):
    """thresholds whose mean list length over q is about each of `means`"""
    _, dist = ora.knn(metric, words, q, len(words))
    return [float(np.quantile(dist, min(m / len(words), 1.0))) for m in means]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("shape", [(700, 352, 100), (130, 33, 300), (3000, 1344, 60), (40, 16, 9)])
def test_threshold_small_matches_oracle(pkg, gpu, ora, metric, shape):
    """launches below the matrix-core gates: the exact VALU scan, every list complete, ordered and bit-equal"""
    ctx, dev = gpu
    n_words, dim, nq = shape
    rng = np.random.default_rng(n_words + dim + metric)
    words = descriptors(rng, n_words, dim, unit=metric == 0)
    q = descriptors(rng, nq, dim, unit=metric == 0)
    q[:3] = words[:3]
    cb = bare_cb(pkg, ctx, words)
    before = ctx.timer("knn_threshold_mfma_launches")[0]
    for thr in thresholds_for(ora, metric, words, q, [0.05, 8, 64]):
        off, idx, dist = pkg.capi.knn_threshold(ctx, cb, metric, T(q, dev), thr)
        check_lists(off, idx, dist, oracle_lists(ora, metric, words, q, thr))
    assert ctx.timer("knn_threshold_mfma_launches")[0] == before
    cb.close()


@pytest.mark.parametrize("metric,dim", [(0, 352), (1, 1344)])
def test_threshold_mfma_matches_oracle(pkg, gpu, ora, metric, dim):
    """4096 queries x 8192 words: the EMIT sweep on the matrix cores + evaluation + compaction. A sample of 192 queries is compared with
    the oracle (the whole list of each). Squared L2 at the two shorter list lengths: the evaluation stage must have answered most
    queries (few went to the exact scan). Chi-square: the Hellinger lower bound lists far more rows than the per-query cap for nearly
    every query on this data, and the exact scan answers them"""
    ctx, dev = gpu
    n_words, nq = 8192, 4096
    rng = np.random.default_rng(dim)
    words = descriptors(rng, n_words, dim, unit=metric == 0)
    q = descriptors(rng, nq, dim, unit=metric == 0)
    cb = bare_cb(pkg, ctx, words)
    sample = np.sort(rng.choice(nq, 192, replace=False))
    for j, thr in enumerate(thresholds_for(ora, metric, words, q[sample], [0.05, 8, 64])):
        before = ctx.timer("knn_threshold_mfma_launches")[0]
        off, idx, dist = pkg.capi.knn_threshold(ctx, cb, metric, T(q, dev), thr)
        assert ctx.timer("knn_threshold_mfma_launches")[0] > before, "the matrix-core path did not run"
        if j < 2 and metric == 0:
            assert ctx.timer("knn_threshold_overflow_queries")[0] < nq // 8, "the candidate lists did not answer the queries"
        check_lists(off, idx, dist, oracle_lists(ora, metric, words, q[sample], thr), rows=sample)
        assert np.all(np.diff(off) >= 0) and off[0] == 0
    cb.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_threshold_edges(pkg, gpu, ora, metric):
    ctx, dev = gpu
    rng = np.random.default_rng(11 + metric)
    n_words, dim, nq = 2048, 64 * 6, 512
    # dyadic data: every functor value is exact in float, so rows AT the threshold exist and must be excluded (strict <)
    words = (rng.integers(0, 4, (n_words, dim)) / 4.0).astype(np.float32)
    q = (rng.integers(0, 4, (nq, dim)) / 4.0).astype(np.float32)
    q[:2] = words[:2]
    words[100:100 + 700] = words[5]                  # 700 duplicate rows: one query lists more rows than the per-query emit cap
    q[7] = words[5]
    cb = bare_cb(pkg, ctx, words)
    _, dist = ora.knn(metric, words, q, n_words)
    thr = float(np.sort(dist[:, 20])[nq // 2])                          # a value some query has: rows AT the threshold
    assert np.any(dist == np.float32(thr)), "no row at the threshold: the strictness check is empty"
    want = oracle_lists(ora, metric, words, q, thr)
    off, idx, dist_g = pkg.capi.knn_threshold(ctx, cb, metric, T(q, dev), thr)
    check_lists(off, idx, dist_g, want)
    assert off[8] - off[7] >= 701
    # a too-small capacity: the count and the offsets, the lists untouched; then the re-call
    total = int(off[-1])
    off2, i2, d2 = pkg.capi.knn_threshold(ctx, cb, metric, T(q, dev), thr, capacity=total - 1)
    assert i2 is None and d2 is None and np.array_equal(off2, off)
    off3, i3, d3 = pkg.capi.knn_threshold(ctx, cb, metric, T(q, dev), thr, capacity=total)
    check_lists(off3, i3, d3, want)
    off0, _, _ = pkg.capi.knn_threshold(ctx, cb, metric, T(q, dev), thr, capacity=0)
    assert np.array_equal(off0, off)
    # threshold <= 0: empty lists
    for t in (0.0, -1.0):
        offz, _, _ = pkg.capi.knn_threshold(ctx, cb, metric, T(q, dev), t)
        assert np.all(offz == 0)
    # a huge threshold lists every row of every query
    offh, ih, dh = pkg.capi.knn_threshold(ctx, cb, metric, T(q[:40], dev), 1e30)
    assert np.array_equal(np.diff(offh), np.full(40, n_words))
    check_lists(offh, ih, dh, oracle_lists(ora, metric, words, q[:40], 1e30))
    cb.close()
    # fewer words than one tile
    small = words[:37].copy()
    cbs = bare_cb(pkg, ctx, small)
    t2 = float(np.sort(ora.knn(metric, small, q, 37)[1][:, 5])[nq // 2])
    offs, i_s, d_s = pkg.capi.knn_threshold(ctx, cbs, metric, T(q, dev), t2)
    check_lists(offs, i_s, d_s, oracle_lists(ora, metric, small, q, t2))
    cbs.close()


@pytest.mark.parametrize("flags", [0, 1 | 2, 4, 1 | 2 | 4 | 8])
def test_cast_votes_csr_matches_oracle(pkg, gpu, ora, flags):
    ctx, dev = gpu
    rng = np.random.default_rng(3 + flags)
    n_words, dim, nq, n_classes = 1500, 352, 300, 4
    words = descriptors(rng, n_words, dim)
    q = descriptors(rng, nq, dim)
    vpw = rng.integers(0, 4, n_words)
    off_v = np.concatenate([[0], np.cumsum(vpw)]).astype(np.uint32)
    nv = int(off_v[-1])
    host = dict(words=words, vote_offsets=off_v, vote_xyz=rng.normal(size=(nv, 3)).astype(np.float32),
                vote_class=rng.integers(0, n_classes, nv).astype(np.uint32), vote_instance=rng.integers(0, 9, nv).astype(np.uint32),
                class_sigma=rng.uniform(0.2, 2.0, n_classes).astype(np.float32), word_weight=rng.uniform(0.5, 1.5, n_words).astype(np.float32),
                vote_weight=rng.uniform(0.5, 1.5, nv).astype(np.float32), vote_class_weight=rng.uniform(0.1, 1, nv).astype(np.float32))
    cb = pkg.capi.Codebook(ctx, words, off_v, host["vote_xyz"], host["vote_class"], host["vote_instance"], n_classes, host["class_sigma"],
                           word_weight=host["word_weight"], vote_weight=host["vote_weight"], vote_class_weight=host["vote_class_weight"])
    lrf = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(np.float32).reshape(9) for _ in range(nq)])
    kp = rng.normal(size=(nq, 3)).astype(np.float32)
    thr = thresholds_for(ora, 0, words, q, [6])[0]
    off, idx, dist = pkg.capi.knn_threshold(ctx, cb, 0, T(q, dev), thr)
    got = pkg.capi.cast_votes_csr(ctx, cb, flags, T(lrf, dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev), off, idx, dist)
    # the oracle over the lists padded to a dense [nq, Lmax] with -1
    lens = np.diff(off)
    L = max(int(lens.max()), 1)
    pidx = np.full((nq, L), -1, np.int32); pdist = np.zeros((nq, L), np.float32)
    ih, dh = idx.cpu().numpy(), dist.cpu().numpy()
    for f in range(nq):
        pidx[f, :lens[f]] = ih[off[f]:off[f + 1]]; pdist[f, :lens[f]] = dh[off[f]:off[f + 1]]
    want = ora.cast_votes(host, flags, lrf, kp[:, 0], kp[:, 1], kp[:, 2], pidx, pdist)
    maxv = cb.max_votes
    a = np.arange(int(off[-1]))
    fa = np.searchsorted(off, a, side="right") - 1
    ja = a - off[fa]
    slots = ((fa * L + ja)[:, None] * maxv + np.arange(maxv)[None, :]).reshape(-1)
    for key in ("cls", "inst", "codeword"):
        assert np.array_equal(got[key].cpu().numpy(), want[key][slots]), key
    assert np.abs(got["weight"].cpu().numpy() - want["weight"][slots]).max() <= 1e-4
    live = want["cls"][slots] >= 0
    assert np.abs(got["pos"].cpu().numpy()[live] - want["pos"][slots][live]).max() <= 1e-4
    cb.close()


def _train_inputs(rng, n, dim, n_classes):
    cls = np.sort(rng.integers(0, n_classes, n)).astype(np.uint32)
    model = np.zeros(n, np.uint32)
    for c in range(n_classes):                                       # 2-3 models per class, contiguous
        m = np.nonzero(cls == c)[0]
        model[m] = c * 10 + (np.arange(len(m)) * 3 // max(len(m), 1))
    desc = descriptors(rng, n, dim)
    lrf = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(np.float32).reshape(9) for _ in range(n)])
    kp = rng.normal(size=(n, 3)).astype(np.float32)
    center = np.stack([np.full(3, 0.1 * m, np.float32) for m in model])
    return desc, lrf, kp, cls, model, center


def test_train_lists_regular_equals_knn_training(pkg, gpu, ora):
    """k-lists from ismhip_knn through ismhip_train_activate_lists == ora.activate(k, clean_up=False)"""
    ctx, dev = gpu
    rng = np.random.default_rng(21)
    n, dim, k = 240, 352, 3
    desc, lrf, kp, cls, model, center = _train_inputs(rng, n, dim, 3)
    cb = bare_cb(pkg, ctx, desc)
    idx, _ = pkg.capi.knn(ctx, cb, 0, T(desc, dev), k)
    off = (np.arange(n + 1) * k).astype(np.int64)
    got = pkg.capi.train_activate_lists(ctx, 0, T(desc, dev), T(lrf, dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev), cls, model, center,
                                        off, idx.reshape(-1).contiguous(), n_classes=3)
    want = ora.activate(0, desc, lrf, kp, cls, model, center, k=k, clean_up=False, n_classes=3)
    for key in ("word_src", "vote_offsets", "vote_feature"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("vote_xyz", "vote_weight", "vote_class_weight", "class_sigma"):
        assert np.allclose(got[key], want[key], rtol=1e-4, atol=1e-5, equal_nan=True), key
    cb.close()


def restate_training(metric, desc, lrf, kp, cls, model, center, off, idx, n_classes, ora):
    """numpy restatement of Codebook::activate (codebook.cpp:64-368) for a CSR of activations, codewords = the features (Clustering
    "None"), with the distributions' computeWeights (codeword_distribution.cpp:169-243)"""
    n = len(desc)
    feat_of = np.repeat(np.arange(n), np.diff(off))
    members = [[] for _ in range(n)]                                  # activations of every codeword in activation order
    for a, w in enumerate(idx):
        members[w].append(a)
    word_src = np.array([w for w in range(n) if members[w]], np.uint32)
    vote_feature = np.array([feat_of[a] for w in word_src for a in members[w]], np.uint32)
    vote_offsets = np.concatenate([[0], np.cumsum([len(members[w]) for w in word_src])]).astype(np.uint32)
    vote_xyz = np.stack([ora.rotate_into(lrf[f], center[f] - kp[f]) for f in vote_feature])
    # sigma^2: whole lists of the first features while the sample holds fewer than sqrt(#features) words; whole models
    sigma = np.empty(n_classes, np.float32)
    for c in range(n_classes):
        fs = np.nonzero(cls == c)[0]
        if len(fs) == 0:
            sigma[c] = np.nan
            continue
        me = int(np.sqrt(len(fs)))
        sw = []
        for f in fs:
            if len(sw) >= me:
                break
            sw.extend(idx[off[f]:off[f + 1]])
        sf = []
        t = 0
        while t < len(fs) and len(sf) < me:
            e = t
            while e < len(fs) and model[fs[e]] == model[fs[t]]:
                e += 1
            sf.extend(fs[t:e]); t = e
        d = np.array([ora.distance(metric, desc[f], desc[w]) for f in sf for w in sw], np.float64)
        sigma[c] = np.float32(np.sum((d - d.mean()) ** 2) / (len(d) - 1)) if len(d) > 1 else np.nan
    # weights: median over the word's activating features of exp(-|centre_j - centre_i|^2 / 0.25)
    vote_weight = np.empty(len(vote_feature), np.float32)
    for e in range(len(word_src)):
        v0, v1 = vote_offsets[e], vote_offsets[e + 1]
        for vi in range(v0, v1):
            ws = []
            for vj in range(v0, v1):
                fj = vote_feature[vj]
                cj = kp[fj] + ora.rotate_back(lrf[fj], vote_xyz[vi])
                d = np.linalg.norm(cj.astype(np.float64) - center[vote_feature[vi]])
                ws.append(np.exp(-d * d / 0.25))
            vote_weight[vi] = np.median(ws)
    # statistical class weights term1 * term2 * term3 (codebook.cpp:226-368; term3 keyed by class, the last word holding it wins)
    vcls = cls[vote_feature]
    num_features = np.bincount(vcls, minlength=n_classes)
    words_per_class = np.zeros(n_classes); term3 = np.zeros(n_classes)
    for e in range(len(word_src)):
        vc = vcls[vote_offsets[e]:vote_offsets[e + 1]]
        cs = np.unique(vc)
        words_per_class[cs] += 1
        s = sum(np.sum(vc == c) / num_features[c] for c in cs)
        for c in cs:
            term3[c] = (np.sum(vc == c) / num_features[c]) / s
    vote_class_weight = np.empty(len(vote_feature), np.float32)
    for e in range(len(word_src)):
        v0, v1 = vote_offsets[e], vote_offsets[e + 1]
        for vi in range(v0, v1):
            c = vcls[vi]
            vote_class_weight[vi] = (1.0 / words_per_class[c]) * (1.0 / (v1 - v0)) * term3[c]
    return dict(word_src=word_src, vote_offsets=vote_offsets, vote_feature=vote_feature, vote_xyz=vote_xyz, vote_weight=vote_weight,
                vote_class_weight=vote_class_weight, class_sigma=sigma)


@pytest.mark.parametrize("metric", [0, 1])
def test_train_lists_variable_matches_restatement(pkg, gpu, ora, metric):
    ctx, dev = gpu
    rng = np.random.default_rng(31 + metric)
    n, dim, n_classes = 280, 352, 3
    desc, lrf, kp, cls, model, center = _train_inputs(rng, n, dim, n_classes)
    cb = bare_cb(pkg, ctx, desc)
    thr = thresholds_for(ora, metric, desc, desc, [5])[0]
    off, idx, _ = pkg.capi.knn_threshold(ctx, cb, metric, T(desc, dev), thr)
    assert len(np.unique(np.diff(off))) > 2, "list lengths should vary"
    got = pkg.capi.train_activate_lists(ctx, metric, T(desc, dev), T(lrf, dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev), cls, model,
                                        center, off, idx, n_classes=n_classes)
    want = restate_training(metric, desc, lrf, kp, cls, model, center, off, idx.cpu().numpy(), n_classes, ora)
    for key in ("word_src", "vote_offsets", "vote_feature"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("vote_xyz", "vote_weight", "vote_class_weight", "class_sigma"):
        assert np.allclose(got[key], want[key], rtol=1e-4, atol=1e-5, equal_nan=True), key
    cb.close()

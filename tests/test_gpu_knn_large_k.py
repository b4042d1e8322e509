"""KNN activation for any K up to 1024 (ismhip_knn_large_k) against the CPU oracle: the contract of ismhip_knn --
exact FLANN functor values, ascending (distance, row), -1 / NaN padding, an all-NaN query gets the first k rows -- checked bit for bit,
on the exact scan and on the certified matrix-core path; training (ismhip_train_activate) with k > 16 against ora.activate."""
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


def manifold(rng, n, dim, intrinsic=8, unit=True, basis_seed=0):
    """rows on a low-dimensional non-negative manifold: distances spread with rank the way descriptor distances do
    (d_K / d_4 ~ (K/4)^(2/intrinsic)), unlike iid high-dimensional rows whose distances all crowd together"""
    A = np.random.default_rng(basis_seed).random((intrinsic, dim)).astype(np.float32)
    x = rng.random((n, intrinsic)).astype(np.float32) @ A + 1e-3 * rng.random((n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True) if unit else x.sum(axis=1, keepdims=True)
    return x.astype(np.float32)


def fast_ctx(pkg, monkeypatch, **env):
    """a ctx with the certified matrix-core path on for chi-square too (the knobs are read when a context is created)"""
    monkeypatch.setenv("ISMHIP_KNN_LARGE_K_FAST", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = pkg.capi.Ctx(0)
    for k in ["ISMHIP_KNN_LARGE_K_FAST", *env]:
        monkeypatch.delenv(k)
    return ctx


def check(ora, metric, words, q, k, idx, dist):
    wi, wd = ora.knn(metric, words, q, k)
    gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(gi, wi), f"rows differ in {int((gi != wi).any(1).sum())} of {len(q)} queries"
    assert np.array_equal(np.isnan(gd), np.isnan(wd)), "NaN pattern differs"
    m = ~np.isnan(wd)
    assert np.array_equal(gd[m].view(np.uint32), wd[m].view(np.uint32)), "distances not bit-equal"


def counters(ctx):
    return {n: int(ctx.timer(f"knn_large_k_{n}_queries")[0]) for n in ("certified", "retry", "exact")}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("shape", [(300, 33, 200), (3000, 96, 600)])
@pytest.mark.parametrize("k", [17, 32, 100, 256, 1024])
def test_large_k_exact_scan_matches_oracle(pkg, gpu, ora, metric, shape, k):
    ctx, dev = gpu
    n, dim, nq = shape
    rng = np.random.default_rng(7 + n + k + metric)
    words = descriptors(rng, n, dim, unit=metric == 0)
    q = descriptors(rng, nq, dim, unit=metric == 0)
    cb = bare_cb(pkg, ctx, words)
    idx, dist = pkg.capi.knn_large_k(ctx, cb, metric, T(q, dev), k)
    check(ora, metric, words, q, k, idx, dist)
    if n < k:
        assert (idx.cpu().numpy()[:, n:] == -1).all()


def test_large_k_edge_cases(pkg, gpu, ora):
    ctx, dev = gpu
    rng = np.random.default_rng(3)
    # 40 identical rows among others: K = 32 takes the 32 lowest of them
    words = descriptors(rng, 500, 64)
    words[100:140] = words[7]
    q = np.repeat(words[7:8], 3, axis=0).copy()
    q[2] += 1e-3
    cb = bare_cb(pkg, ctx, words)
    idx, dist = pkg.capi.knn_large_k(ctx, cb, 0, T(q, dev), 32)
    check(ora, 0, words, q, 32, idx, dist)
    assert idx.cpu().numpy()[0].tolist() == [7] + list(range(100, 131))
    # n_words < K and n_words == K, and an all-NaN query (the first k rows, NaN distances)
    for n in (40, 64):
        w = descriptors(rng, n, 48)
        qq = descriptors(rng, 5, 48)
        qq[3] = np.nan
        cbn = bare_cb(pkg, ctx, w)
        for metric in (0, 1):
            idx, dist = pkg.capi.knn_large_k(ctx, cbn, metric, T(qq, dev), 64)
            check(ora, metric, w, qq, 64, idx, dist)
            gi = idx.cpu().numpy()
            assert gi[3, :n].tolist() == list(range(n))
            if metric == 0:                                       # (chi-square skips terms whose sum is not > 0: a NaN query scores 0)
                assert np.isnan(dist.cpu().numpy()[3, :n]).all()


def test_large_k_small_k_and_cap(pkg, gpu):
    ctx, dev = gpu
    rng = np.random.default_rng(5)
    words = descriptors(rng, 2000, 352)
    q = T(descriptors(rng, 300, 352), dev)
    cb = bare_cb(pkg, ctx, words)
    for k in (1, 4, 16):
        a = pkg.capi.knn(ctx, cb, 0, q, k)
        b = pkg.capi.knn_large_k(ctx, cb, 0, q, k)
        assert all(np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32)) for x, y in zip(a, b))
    with pytest.raises(RuntimeError, match="k > 1024"):
        pkg.capi.knn_large_k(ctx, cb, 0, q, 1025)
    lib = pkg.capi.lib()
    import ctypes as C
    i = T(np.zeros(1, np.int32), dev); d = T(np.zeros(1, np.float32), dev)
    assert lib.ismhip_knn_large_k(ctx._h, cb._h, 0, 1, C.c_void_p(q.data_ptr()), 1025, C.c_void_p(i.data_ptr()), C.c_void_p(d.data_ptr())) == -4
    assert lib.ismhip_knn_large_k(ctx._h, cb._h, 0, 1, C.c_void_p(q.data_ptr()), 0, C.c_void_p(i.data_ptr()), C.c_void_p(d.data_ptr())) == -1


@pytest.mark.parametrize("k", [17, 64, 256])
def test_large_k_gated_l2(pkg, gpu, ora, k, monkeypatch):
    _, dev = gpu
    rng = np.random.default_rng(11 + k)
    words = manifold(rng, 16384, 352)
    q = manifold(rng, 2048, 352)
    qd = T(q, dev)
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    idx, dist = pkg.capi.knn_large_k(ctx, cb, 0, qd, k)
    check(ora, 0, words, q, k, idx, dist)
    c = counters(ctx)
    assert c["certified"] > 0, c                                  # the matrix-core path ran (by default) and certified queries
    assert c["certified"] + c["exact"] == len(q)
    base = (idx.cpu().numpy(), dist.cpu().numpy().view(np.uint32))
    runs = ((fast_ctx(pkg, monkeypatch, ISMHIP_KNN_LARGE_K_EXACT="1"), "exact"),
            (fast_ctx(pkg, monkeypatch, ISMHIP_KNN_LARGE_K_SEED_SCALE="1e-3"), "small seed"),
            (fast_ctx(pkg, monkeypatch, ISMHIP_KNN_LARGE_K_SEED_SCALE="1e3"), "large seed"))
    for c2, what in runs:
        cb2 = bare_cb(pkg, c2, words)
        i2, d2 = pkg.capi.knn_large_k(c2, cb2, 0, qd, k)
        assert np.array_equal(i2.cpu().numpy(), base[0]) and np.array_equal(d2.cpu().numpy().view(np.uint32), base[1]), what
        cc = counters(c2)
        if what == "exact":
            assert cc == {"certified": 0, "retry": 0, "exact": len(q)}, (what, cc)
        elif what == "small seed":                                 # every list falls short: all retried, what the retry misses is scanned
            assert cc["retry"] > 0 and cc["certified"] + cc["exact"] == len(q), cc
        else:                                                      # every list overflows: all scanned
            assert cc["exact"] > c["exact"], cc


def test_large_k_gated_chi2(pkg, gpu, ora, monkeypatch):
    _, dev = gpu
    rng = np.random.default_rng(19)
    # (a 4-dimensional manifold: the Hellinger lists hold about 4x the rows of chi-square <= t there and fit the cap)
    words = manifold(rng, 8192, 352, intrinsic=4, unit=False)
    q = manifold(rng, 1024, 352, intrinsic=4, unit=False)
    ctx = fast_ctx(pkg, monkeypatch)
    cb = bare_cb(pkg, ctx, words)
    for k in (32, 100):
        idx, dist = pkg.capi.knn_large_k(ctx, cb, 1, T(q, dev), k)
        check(ora, 1, words, q, k, idx, dist)
        c = counters(ctx)
        assert c["certified"] + c["exact"] == len(q), c
        if k == 32:
            assert c["certified"] > 0, c                          # certified through the shadow codebook's row permutation
    # without ISMHIP_KNN_LARGE_K_FAST chi-square takes the exact scan
    c0 = pkg.capi.Ctx(0)
    i0, d0 = pkg.capi.knn_large_k(c0, bare_cb(pkg, c0, words), 1, T(q, dev), 32)
    check(ora, 1, words, q, 32, i0, d0)
    assert counters(c0) == {"certified": 0, "retry": 0, "exact": len(q)}
    # a negative element in the batch: no Hellinger images, every query takes the exact scan
    q2 = q.copy()
    q2[5, 3] = -0.25
    idx, dist = pkg.capi.knn_large_k(ctx, cb, 1, T(q2, dev), 32)
    check(ora, 1, words, q2, 32, idx, dist)
    assert counters(ctx) == {"certified": 0, "retry": 0, "exact": len(q2)}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k", [24, 64])
@pytest.mark.parametrize("with_centres", [False, True])
def test_train_activate_large_k_matches_oracle(pkg, gpu, ora, metric, k, with_centres):
    ctx, dev = gpu
    rng = np.random.default_rng(60 + 10 * metric + k)
    n, D = 1500, 48
    proto = rng.random((60, D)).astype(np.float32)
    feats = (proto[rng.integers(0, 60, n)] + 0.05 * rng.random((n, D))).astype(np.float32)
    feats[1000:1030] = feats[5:35]
    cls = np.sort(rng.integers(0, 4, n)).astype(np.uint32)
    model = np.zeros(n, np.uint32)
    for c in range(4):
        ids = np.nonzero(cls == c)[0]
        model[ids] = c * 10 + (np.arange(len(ids)) * 3 // max(1, len(ids)))
    A = rng.normal(size=(n, 3, 3)); Q, _ = np.linalg.qr(A); Q[np.linalg.det(Q) < 0, 2] *= -1
    lrf = Q.reshape(n, 9).astype(np.float32); kp = rng.normal(size=(n, 3)).astype(np.float32)
    centre = rng.normal(size=(40, 3)).astype(np.float32)[model]
    cw = (proto[rng.integers(0, 60, 300)] + 0.05 * rng.random((300, D))).astype(np.float32) if with_centres else None
    got = pkg.capi.train_activate(ctx, metric, T(feats, dev), T(lrf, dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev), cls, model, centre,
                                  k=k, clean_up=False, n_classes=4, codewords=None if cw is None else T(cw, dev))
    want = ora.activate(metric, feats, lrf, kp, cls, model, centre, k=k, clean_up=False, n_classes=4, codewords=cw)
    for key in ("word_src", "vote_offsets", "vote_feature"):
        assert np.array_equal(got[key], want[key]), key
    np.testing.assert_allclose(got["vote_xyz"], want["vote_xyz"], atol=2e-6)
    np.testing.assert_allclose(got["vote_weight"], want["vote_weight"], atol=2e-6)
    np.testing.assert_allclose(got["vote_class_weight"], want["vote_class_weight"], rtol=1e-6, atol=1e-12)
    assert np.array_equal(got["class_sigma"], want["class_sigma"])

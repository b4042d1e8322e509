"""The codeword search for rows of 1345 to 2048 floats (-m gpu): ismhip_knn, _ratio and _rule on codebooks of 1345, 1960 and 2048 columns
bit-equal to the oracle (the FLANN functor in its own summation order, ties to the lowest row), ismhip_train_activate and ismhip_kmeans
at 1960, and the refusals that stay: 2049 columns everywhere, ismhip_knn_large_k above K = 16 and ismhip_knn_threshold above 1344.

Shapes (words, dim, queries): (300, 1960, 70) the USC row; (130, 1345, 65) the first length past the old cap, not a multiple of four
(dim_pad 1376: the last 16-byte chunk row of a lane group is half empty); (40, 2048, 9) the cap itself with fewer words than one row
range; (4200, 1960, 300) above the sizes at which shorter rows go to the matrix cores (1024 words, 256 queries)."""
import functools

import numpy as np
import pytest

from test_gpu_parity import T

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(300, 1960, 70), (130, 1345, 65), (40, 2048, 9), (4200, 1960, 300)]


@functools.lru_cache(maxsize=None)
def data(shape, kind):
    """(words, queries). "hist": non-negative sparse histogram-like rows (queries are perturbed words and fresh rows); "wild": signed
    rows with magnitudes spread over 10^6, exact duplicates among the words and queries that ARE words (distance 0, ties)."""
    nw, dim, nq = shape
    rng = np.random.default_rng(nw * 7 + dim + (0 if kind == "hist" else 1))
    if kind == "hist":
        w = rng.gamma(0.3, 1.0, size=(nw, dim)) * (rng.random((nw, dim)) < 0.3)
        q = np.concatenate([w[rng.integers(0, nw, nq // 2)] * rng.uniform(0.9, 1.1, size=(nq // 2, dim)),
                            rng.gamma(0.3, 1.0, size=(nq - nq // 2, dim)) * (rng.random((nq - nq // 2, dim)) < 0.3)])
    else:
        scale = 10.0 ** rng.uniform(-3, 3, size=(nw, 1))
        w = rng.normal(size=(nw, dim)) * scale
        w[nw // 2:nw // 2 + 8] = w[3:11]                                  # duplicates: the lower row wins
        w[-1] = w[0]
        q = np.concatenate([w[rng.integers(0, nw, nq // 2)], rng.normal(size=(nq - nq // 2, dim)) * 10.0 ** rng.uniform(-3, 3, size=(nq - nq // 2, 1))])
    return w.astype(F), q.astype(F)


def codebook(pkg, gpu, words, n_classes=5, seed=3):
    ctx, _ = gpu
    n = len(words)
    wcls = np.random.default_rng(seed).integers(0, n_classes, n).astype(np.uint32)
    cb = pkg.capi.Codebook(ctx, words, np.arange(n + 1, dtype=np.uint32), np.zeros((n, 3), F), wcls, np.zeros(n, np.uint32), n_classes, np.ones(n_classes, F))
    return cb, wcls


@pytest.fixture(scope="module")
def books(pkg, gpu):
    """one device codebook per (shape, kind), shared by the search tests"""
    made = {}

    def get(shape, kind):
        if (shape, kind) not in made:
            made[(shape, kind)] = codebook(pkg, gpu, data(shape, kind)[0])
        return made[(shape, kind)]
    yield get
    for cb, _ in made.values():
        cb.close()


@functools.lru_cache(maxsize=None)
def oracle_knn(shape, kind, metric):
    """k = 16 once per case: the first k columns are the answer for every smaller k (the oracle sorts by (distance, row))"""
    import __graft_entry__ as ge
    w, q = data(shape, kind)
    return ge.load_oracle().knn(metric, w, q, min(16, len(w)))


@pytest.mark.parametrize("k", [1, 2, 3, 16])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", ["hist", "wild"])
@pytest.mark.parametrize("shape", SHAPES)
def test_knn_is_bit_equal_to_the_oracle(pkg, gpu, ora, books, shape, kind, metric, k):
    ctx, dev = gpu
    w, q = data(shape, kind)
    cb, _ = books(shape, kind)
    idx, dist = pkg.capi.knn(ctx, cb, metric, T(q, dev), k)
    ctx.sync()
    widx, wdist = oracle_knn(shape, kind, metric)
    if shape == SHAPES[0] and k == 16:
        one = ora.knn(metric, w, q[:5], 3)                                   # the prefix property, checked where it is used
        assert np.array_equal(one[0], widx[:5, :3]) and np.array_equal(one[1].view(np.uint32), wdist[:5, :3].view(np.uint32))
    assert np.array_equal(idx.cpu().numpy(), widx[:, :k])
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), wdist[:, :k].view(np.uint32))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", ["hist", "wild"])
@pytest.mark.parametrize("shape", SHAPES)
def test_ratio_and_rule_against_the_oracle(pkg, gpu, ora, books, shape, kind, metric):
    ctx, dev = gpu
    w, q = data(shape, kind)
    cb, wcls = books(shape, kind)
    for thr in (0.8, 0.95):
        i, d = pkg.capi.knn_ratio(ctx, cb, metric, T(q, dev), thr)
        wi, wd = ora.knn_ratio(metric, w, q, thr)
        assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy().view(np.uint32), wd.view(np.uint32))
        i, d = pkg.capi.knn_rule(ctx, cb, metric, T(q, dev), thr)
        wi, wd = ora.knn_rule(metric, w, wcls, q, thr)
        assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(d.cpu().numpy().view(np.uint32), wd.view(np.uint32))


def test_refusals(pkg, gpu, books):
    ctx, dev = gpu
    capi = pkg.capi
    rng = np.random.default_rng(5)
    with pytest.raises(capi.IsmHipError, match=r"\(-4\).*longer than 2048"):
        codebook(pkg, gpu, rng.random((20, 2049)).astype(F))
    with pytest.raises(capi.IsmHipError, match=r"\(-4\).*kmeans: descriptor longer than 2048"):
        capi.kmeans(ctx, 0, T(rng.random((20, 2049)).astype(F), dev), 3)
    feats, cls, model, lrf, kp, centre = _training_set(rng, 200, 2049)
    with pytest.raises(capi.IsmHipError, match=r"\(-4\).*train_activate: descriptor longer than 2048"):
        capi.train_activate(ctx, 0, T(feats, dev), T(lrf, dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev), cls, model, centre, k=1, n_classes=3)
    w, q = data(SHAPES[0], "hist")
    cb, _ = books(SHAPES[0], "hist")
    with pytest.raises(capi.IsmHipError, match=r"\(-4\).*knn_large_k: descriptor longer than 1344"):
        capi.knn_large_k(ctx, cb, 0, T(q, dev), 17)
    with pytest.raises(capi.IsmHipError, match=r"\(-4\).*knn_threshold: descriptor longer than 1344"):
        capi.knn_threshold(ctx, cb, 0, T(q, dev), 1.0)
    with pytest.raises(capi.IsmHipError, match=r"\(-4\).*k > 16"):
        capi.knn(ctx, cb, 0, T(q, dev), 17)
    idx, _ = capi.knn_large_k(ctx, cb, 0, T(q, dev), 16)                     # K <= 16 is ismhip_knn: served; the context stays usable
    assert np.array_equal(idx.cpu().numpy(), oracle_knn(SHAPES[0], "hist", 0)[0])


def _training_set(rng, n, D, n_classes=3):
    proto = rng.gamma(0.3, 1.0, size=(12, D)) * (rng.random((12, D)) < 0.3)
    feats = (proto[rng.integers(0, 12, n)] * rng.uniform(0.8, 1.2, size=(n, D))).astype(F)
    feats[150:158] = feats[5:13]                                             # exact duplicates: both copies activate the LOWER row
    cls = np.sort(rng.integers(0, n_classes, n)).astype(np.uint32)
    model = np.zeros(n, np.uint32)
    for c in range(n_classes):
        ids = np.nonzero(cls == c)[0]
        model[ids] = c * 10 + (np.arange(len(ids)) * 3 // max(1, len(ids)))
    A = rng.normal(size=(n, 3, 3)); Q, _ = np.linalg.qr(A); Q[np.linalg.det(Q) < 0, 2] *= -1
    lrf = Q.reshape(n, 9).astype(F); kp = rng.normal(size=(n, 3)).astype(F)
    centre = rng.normal(size=(n_classes * 10 + 3, 3)).astype(F)[model]
    return feats, cls, model, lrf, kp, centre


@pytest.mark.parametrize("metric,k,clean_up", [(0, 1, True), (1, 2, False)])
def test_train_activate_at_1960(pkg, gpu, ora, metric, k, clean_up):
    """200 rows in 3 classes: the activation (wide search), the class sigma^2 (wave_functor on a 2048-float term buffer) and the vote
    tables against the oracle; the integers and sigma^2 bit for bit, the weights as test_gpu_parity.py holds them at shorter rows"""
    ctx, dev = gpu
    feats, cls, model, lrf, kp, centre = _training_set(np.random.default_rng(40 + metric), 200, 1960)
    got = pkg.capi.train_activate(ctx, metric, T(feats, dev), T(lrf, dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev), cls, model, centre,
                                  k=k, clean_up=clean_up, n_classes=3)
    want = ora.activate(metric, feats, lrf, kp, cls, model, centre, k=k, clean_up=clean_up, n_classes=3)
    for key in ("word_src", "vote_offsets", "vote_feature"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["class_sigma"].view(np.uint32), want["class_sigma"].view(np.uint32))
    np.testing.assert_allclose(got["vote_xyz"], want["vote_xyz"], atol=2e-6)
    np.testing.assert_allclose(got["vote_weight"], want["vote_weight"], atol=2e-6)
    np.testing.assert_allclose(got["vote_class_weight"], want["vote_class_weight"], rtol=1e-6, atol=1e-12)
    if clean_up:
        assert len(want["word_src"]) < 200                                   # the duplicated rows were cleaned away


@pytest.mark.parametrize("init", ["FLANN_CENTERS_RANDOM", "FLANN_CENTERS_GONZALES", "FLANN_CENTERS_KMEANSPP"])
@pytest.mark.parametrize("metric", [0, 1])
def test_kmeans_at_1960(pkg, gpu, ora, init, metric):
    ctx, dev = gpu
    feats = _training_set(np.random.default_rng(50 + metric), 200, 1960)[0]
    cen, assign, dist, it = pkg.capi.kmeans(ctx, metric, T(feats, dev), 9, max_iterations=15, centers_init=init, seed=11)
    wcen, wassign, wdist, wit = ora.kmeans(metric, feats, 9, max_iterations=15, centers_init=pkg.capi.CENTERS_INIT[init], seed=11)
    assert it == wit and tuple(cen.shape) == wcen.shape
    assert np.array_equal(cen.cpu().numpy().view(np.uint32), wcen.view(np.uint32))
    assert np.array_equal(assign.cpu().numpy(), wassign)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), wdist.view(np.uint32))

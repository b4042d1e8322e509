"""ismhip_rank_scores / ismhip_rank_select on the device against the numpy transcription of the reference (ranking_ref.py), whose
neighbour lists come from the CPU oracle's exact chi-square kNN."""
import numpy as np
import pytest

import __graft_entry__ as ge
import ranking_ref as ref
import ranking_scenes as scenes

pytestmark = pytest.mark.gpu

# (type, ScoreIncrementType): every variant whose arithmetic the reference states in float
VARIANTS = (("KNNActivation", 1), ("KNNActivation", 2), ("Incremental", 0), ("Strangeness", 0), ("NaiveBayes", 0))
_cache = {}


def _scene(i):
    if ("scene", i) not in _cache:
        sc = scenes.SCENES[i]()
        _, dist = ge.load_oracle().knn(ref.CHI2, sc["desc"], sc["desc"], sc["k_search"] + 1)
        sc["threshold"] = scenes.bayes_threshold(dist)
        _cache["scene", i] = sc
    return _cache["scene", i]


def _want(i, variant):
    """the reference scores of a scene, computed once"""
    if ("want", i, variant) not in _cache:
        sc = _scene(i)
        _cache["want", i, variant] = ref.scores(ge.load_oracle().knn, variant[0], sc["desc"], sc["off"], sc["k_search"], sc["threshold"], variant[1])
    return _cache["want", i, variant]


def _got(pkg, gpu, i, variant, fresh=False):
    """the device scores of a scene (host copy), computed once unless `fresh`"""
    import torch
    if fresh or ("got", i, variant) not in _cache:
        ctx, dev = gpu
        sc = _scene(i)
        s = pkg.capi.rank_scores(ctx, variant[0], torch.as_tensor(sc["desc"]).to(dev), sc["off"], sc["k_search"], sc["threshold"], variant[1])
        s = s.cpu().numpy()
        if fresh:
            return s
        _cache["got", i, variant] = s
    return _cache["got", i, variant]


def _same_bits(a, b):
    """bit-equal where neither is NaN, NaN in the same places (the sign and payload of a NaN are the platform's)"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "%s%d" % v)
@pytest.mark.parametrize("i", range(len(scenes.SCENES)), ids=[s.__name__ for s in scenes.SCENES])
def test_scores_equal_reference(pkg, gpu, i, variant):
    want, got = _want(i, variant), _got(pkg, gpu, i, variant)
    bad = np.nonzero(~((want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))))[0]
    assert _same_bits(got, want), (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def test_scenes_hold_their_edge_cases(pkg, gpu):
    """what the scenes are there for shows in the reference: 0/0 and x/0 in the nan scene, a self match that is not first in the wide one,
    a class smaller than K + 1 and an empty one in the mixed one, thresholds that split the neighbour lists"""
    nan_i = [s.__name__ for s in scenes.SCENES].index("nan")
    s = _want(nan_i, ("Strangeness", 0))
    assert np.isnan(s).sum() == 7 and np.isposinf(s).sum() == 1
    sc = _scene(1)
    idx, dist = ge.load_oracle().knn(ref.CHI2, sc["desc"], sc["desc"], 2)
    assert (idx[:, 0] != np.arange(len(idx))).sum() >= 7 and (dist[:, 1] == 0).sum() >= 9
    off = _scene(0)["off"]
    assert 0 in np.diff(off) and (np.diff(off)[np.diff(off) > 0] < _scene(0)["k_search"] + 1).any()
    # the hub scene: reverse lists (how often a row is named among the first K results) beyond a wave's 64 lanes and beyond the 1024
    # entries the sum kernel orders in LDS, with terms of many sizes
    sc = _scene([s.__name__ for s in scenes.SCENES].index("hub"))
    idx, dist = ge.load_oracle().knn(ref.CHI2, sc["desc"], sc["desc"], sc["k_search"] + 1)
    named = np.bincount(idx[:, :-1].ravel(), minlength=len(idx))
    assert named.max() > 1024 and ((named > 64) & (named <= 1024)).any()
    assert len(np.unique(dist[idx[:, 1] == named.argmax(), 1])) > 500
    for i in range(len(scenes.SCENES)):
        b = _want(i, ("NaiveBayes", 0))
        assert len(np.unique(b[~np.isnan(b)])) >= 3


@pytest.mark.parametrize("i", range(len(scenes.SCENES)), ids=[s.__name__ for s in scenes.SCENES])
def test_knn_activation_exp_within_float_bound(pkg, gpu, i):
    """ScoreIncrementType 3 adds exp(d). The reference does not pin which exp overload it calls, so the device's float sum is compared to
    the same sum in float64. With t terms e_1 .. e_t of a score (all positive): the device's expf is within 1 ulp, a relative 2^-23 per
    term, together 2^-23 * sum|e|; each of its t float additions rounds a partial sum that is at most sum|e| (1 + t 2^-23) by half an ulp,
    together below t * 2^-24 * sum|e| (1 + t 2^-23); the distances d are the same floats on both sides. That is (1 + t / 2) * 2^-23 *
    sum|e| and a second-order rest; (t + 2) * 2^-23 * sum|e| covers it and the reference's own final rounding to float."""
    sc = _scene(i)
    got = _got(pkg, gpu, i, ("KNNActivation", 3)).astype(np.float64)
    s, a, t = ref.knn_activation_exp_f64(ge.load_oracle().knn, sc["desc"], sc["k_search"])
    err, bound = np.abs(got - s), (t + 2) * 2.0 ** -23 * a
    print("exp sum: max err / bound %.3g" % (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (err.max(), bound[err.argmax()])
    assert (got[t == 0] == 0).all()


@pytest.mark.parametrize("i", range(len(scenes.SCENES)), ids=[s.__name__ for s in scenes.SCENES])
def test_scores_are_deterministic(pkg, gpu, i):
    for variant in VARIANTS + (("KNNActivation", 3),):
        a, b = _got(pkg, gpu, i, variant), _got(pkg, gpu, i, variant, fresh=True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), variant


def _check_select(pkg, gpu, score, off):
    import torch
    ctx, dev = gpu
    d_score = torch.as_tensor(score).to(dev)
    for factor, offset in scenes.WINDOWS:
        keep, n_keep = pkg.capi.rank_select(ctx, d_score, off, factor, offset)
        want_keep, want_n = ref.select(score, off, factor, offset)
        assert np.array_equal(n_keep, want_n), (factor, offset, n_keep, want_n)
        assert np.array_equal(keep.cpu().numpy(), want_keep), (factor, offset, np.nonzero(keep.cpu().numpy() != want_keep)[0][:8])


@pytest.mark.parametrize("i", range(len(scenes.SCENES)), ids=[s.__name__ for s in scenes.SCENES])
def test_select_on_device_scores(pkg, gpu, i):
    """the scores the device computed (ties by the thousand in KNNActivation type 1, NaN and +inf in Strangeness) through every window"""
    for variant in VARIANTS:
        _check_select(pkg, gpu, _got(pkg, gpu, i, variant), _scene(i)["off"])


@pytest.mark.parametrize("case", scenes.score_vectors(), ids=lambda c: c[0])
def test_select_on_hand_made_scores(pkg, gpu, case):
    _check_select(pkg, gpu, case[1], case[2])


def test_select_more_than_one_pass_of_the_block(pkg, gpu):
    """a class longer than the select kernel's workgroup (1024 threads), few distinct values: ranks decided by the index digits"""
    rng = np.random.default_rng(5)
    score = rng.integers(0, 4, 5000).astype(np.float32)
    score[rng.integers(0, 5000, 50)] = np.nan
    score[rng.integers(0, 5000, 50)] = -0.0
    _check_select(pkg, gpu, score, np.asarray([0, 3000, 3001, 5000], np.uint32))


def test_argument_errors_leave_outputs_unwritten(pkg, gpu):
    import torch
    capi = pkg.capi
    ctx, dev = gpu
    sc = _scene(0)
    desc = torch.as_tensor(sc["desc"]).to(dev)
    n = len(sc["desc"])
    score = torch.full((n,), 123.0, dtype=torch.float32, device=dev)
    bad_off = sc["off"].copy(); bad_off[1], bad_off[2] = bad_off[2], bad_off[1] + 200
    cases = [dict(rank_type=9, class_offsets=sc["off"]),                                       # a bad type
             dict(rank_type="KNNActivation", class_offsets=sc["off"], increment_type=4),
             dict(rank_type="Strangeness", class_offsets=np.asarray([0, n, n], np.uint32)),     # a single non-empty class
             dict(rank_type="Incremental", class_offsets=np.asarray([0, 100, 50, n], np.uint32)),
             dict(rank_type="Incremental", class_offsets=bad_off)]
    for kw in cases:
        with pytest.raises(capi.IsmHipError, match=r"\(-1\)"):
            capi.rank_scores(ctx, desc=desc, k_search=10, out=score, **kw)
        assert (score.cpu().numpy() == 123.0).all(), kw
    keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    n_keep = np.full(3, 99, np.uint32)
    with pytest.raises(capi.IsmHipError, match=r"\(-1\)"):
        capi.rank_select(ctx, score, np.asarray([0, 100, 50, n], np.uint32), 0.75, 0.0, out=(keep, n_keep))
    assert (keep.cpu().numpy() == 7).all() and (n_keep == 99).all()
    # and the same arguments in order are accepted
    capi.rank_scores(ctx, "Strangeness", desc, sc["off"], 10, out=score)
    assert not (score.cpu().numpy() == 123.0).any()

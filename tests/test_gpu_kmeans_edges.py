"""k-means (kmeans.hip) on the cases of kmeans_scenes.py (-m gpu). Each case is checked twice: bit-equal to the CPU oracle's
restatement (ora.kmeans: centres, assignment, distances, rounds), and against properties that do not depend on that restatement:
chosen centres are data rows; GONZALES rows maximise the float64 minimum distance to the earlier centres and the lowest row wins
float32 ties; the k-means++ rows are those of a Python-integer restatement of the draws; coincident data gives fewer centres than
asked; after convergence every centre is the float64 mean of its members within 2^(e-40) plus a float32 rounding and every point
sits at its float64 nearest centre wherever the gap to the runner-up exceeds the float32 error bound of the functor."""
import numpy as np
import pytest

import kmeans_scenes as ks

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def both(pkg, gpu, ora, c, max_iterations=None):
    """(device result, oracle result) as host arrays, after the bit-equality check"""
    ctx, dev = gpu
    mi = c["max_iterations"] if max_iterations is None else max_iterations
    centres, assign, dist, it = pkg.capi.kmeans(ctx, c["metric"], T(c["x"], dev), c["k"], mi, c["init"], c["seed"])
    got = (centres.cpu().numpy(), assign.cpu().numpy(), dist.cpu().numpy(), it)
    want = ora.kmeans(c["metric"], c["x"], c["k"], mi, c["init"], c["seed"])
    assert got[0].shape == want[0].shape, (got[0].shape, want[0].shape)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "centres differ from the oracle"
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)) and got[3] == want[3]
    return got


def rows_of(x, centres):
    """the data row every centre is a copy of (lowest such row)"""
    out = []
    for c in centres:
        hit = np.nonzero((x.view(np.uint32) == c.view(np.uint32)).all(1))[0]
        assert len(hit), "a centre is not a data row"
        out.append(int(hit[0]))
    return out


def dist64(metric, a, b):
    a = a.astype(f64); b = b.astype(f64)
    if metric == 1:
        s = a + b
        return np.where(s > 0, (a - b) ** 2 / np.where(s > 0, s, 1.0), 0.0).sum(-1)
    return ((a - b) ** 2).sum(-1)


def functor_bound(dim, d):
    """|float32 functor - exact| <= gamma_(dim + 4) * d: every term takes at most 4 rounded operations (subtract, square, divide, the
    add that forms x + y) and the sum at most dim additions; all terms are non-negative"""
    u = 2.0 ** -24
    n = dim + 4
    return n * u / (1 - n * u) * d


def check_gonzales(ora, c, centres):
    x = c["x"]
    rows = rows_of(x, centres)
    assert rows[0] == ks.first_centre(c["seed"], len(x))
    for s in range(1, len(rows)):
        d64 = np.min([dist64(c["metric"], x, x[r][None]) for r in rows[:s]], axis=0)
        d32 = np.min([[ora.distance(c["metric"], x[i], x[r]) for i in range(len(x))] for r in rows[:s]], axis=0).astype(f32)
        assert d64[rows[s]] >= d64.max() - 2 * functor_bound(x.shape[1], d64.max()), s
        tied = np.nonzero(d32 == d32[rows[s]])[0]
        assert rows[s] == tied[0] and d32[rows[s]] == d32.max(), (s, rows[s], tied)
    return rows


@pytest.mark.parametrize("name", list(ks.cases()))
def test_kmeans_case(pkg, gpu, ora, name):
    c = ks.cases()[name]
    x = c["x"]
    n = len(x)
    centres, assign, dist, it = both(pkg, gpu, ora, c)
    kc = len(centres)
    assert assign.min() >= 0 and assign.max() < kc
    if c["max_iterations"] == 0:
        assert it == 0
        rows = rows_of(x, centres)
        assert len(set(rows)) == kc
    if name == "gonzales-ties":
        assert check_gonzales(ora, c, centres) == [4, 0, 1, 2, 3, 5]
    if name == "no-lloyd-gonzales":
        assert len(check_gonzales(ora, c, centres)) == c["k"]
    if name == "no-lloyd-kmeanspp":
        assert rows_of(x, centres) == ks.kmeanspp_picks(lambda i, r: ora.distance(0, x[i], x[r]), x, c["k"], c["seed"])
    if name == "no-lloyd-random":
        assert rows_of(x, centres) == ks.permutation(c["seed"], n)[:c["k"]]
    if name.startswith("all-equal"):
        assert kc == 1 and np.array_equal(centres[0], x[0]) and np.all(assign == 0) and np.all(dist == 0)
    if name.startswith("two-values"):
        assert kc == 2 and sorted(map(tuple, centres.tolist())) == [(1.0, 2.0, 3.0), (4.0, 0.0, 1.0)] and np.all(dist == 0)
    if name.startswith("k1-"):
        assert kc == 1 and np.all(assign == 0) and np.abs(centres[0] - x.astype(f64).mean(0)).max() <= 2.0 ** (5 - 40) + 2.0 ** -19
    if name.startswith("k-is-n") or name.startswith("k-above-n"):
        assert kc == n and sorted(assign.tolist()) == list(range(n)) and np.all(dist == 0)
    if name == "random-run":
        p = c["perm"]
        assert all(np.array_equal(x[p[j]], x[p[0]]) for j in range(1, 71)) and not np.array_equal(x[p[71]], x[p[0]])
        c0 = both(pkg, gpu, ora, c, max_iterations=0)[0]
        assert rows_of(x, c0)[1:] == [p[71], p[72], p[73]] and np.array_equal(c0[0], x[p[0]])
    if name == "fix-empty":
        check_fix_empty(pkg, gpu, ora, c)
    if c.get("converge"):
        check_converged(c, centres, assign, it)


@pytest.mark.parametrize("n", ks.BLOCK_N)
def test_kmeanspp_draws_in_the_partial_last_block(pkg, gpu, ora, n):
    c = ks.kmeanspp_block_case(n, ora)
    centres = both(pkg, gpu, ora, c)[0]
    last = (n - 1) // 1024
    assert last in [p // 1024 for p in c["picks"][1:]]
    assert rows_of(c["x"], centres) == c["picks"] and len(c["picks"]) == c["k"]


def check_fix_empty(pkg, gpu, ora, c):
    """the oracle's own rounds show the hand-over: after round 1 the exact assignment to its centres leaves a cluster empty (also in
    float64, with a decided gap); round 2 then has that cluster's centre ON the first member of the next cluster with more than one"""
    x = c["x"]
    c1, a1, _, _ = both(pkg, gpu, ora, c, max_iterations=1)
    cnt = np.bincount(a1, minlength=len(c1))
    empty = np.nonzero(cnt == 0)[0]
    assert len(c1) == c["k"] and len(empty) == 1
    i = int(empty[0])
    d = np.stack([dist64(0, x, c1[j][None]) for j in range(len(c1))], 1)
    others = np.delete(d, i, axis=1).min(1)
    assert np.all(d[:, i] - others > 2 * functor_bound(x.shape[1], d.max())), "the emptied cluster is not decided in float64"
    j = (i + 1) % len(c1)
    while cnt[j] <= 1:
        j = (j + 1) % len(c1)
    p = int(np.nonzero(a1 == j)[0][0])
    c2 = both(pkg, gpu, ora, c, max_iterations=2)[0]
    assert np.array_equal(c2[i], x[p]), "round 2 does not show the handed-over point"


def check_converged(c, centres, assign, it):
    x = c["x"]; dim = x.shape[1]
    assert 0 < it < c["max_iterations"], "did not converge"
    e = int(np.frexp(np.abs(x).max())[1])
    for j in range(len(centres)):
        members = x[assign == j].astype(f64)
        assert len(members)
        mean = members.mean(0)
        assert np.all(np.abs(centres[j] - mean) <= 2.0 ** (e - 40) + np.spacing(np.abs(mean).astype(f32)).astype(f64)), j
    d = np.stack([dist64(c["metric"], x, centres[j][None]) for j in range(len(centres))], 1)
    srt = np.sort(d, 1)
    decided = srt[:, 1] - srt[:, 0] > functor_bound(dim, srt[:, 0]) + functor_bound(dim, srt[:, 1])
    left_out = 1 - decided.mean()
    print(f"{c['name']}: {it} rounds, {100 * left_out:.2f} % of the assignments left out as undecided")
    assert left_out < 0.01
    assert np.array_equal(assign[decided], d.argmin(1)[decided])

"""k-means inputs that sit on the decisions of kmeans.hip: the centre choosers at their block and lane boundaries, data that runs
out of distinct points, and a Lloyd round that empties a cluster. Each case is a dict of the arguments of capi.kmeans / ora.kmeans
with `pins`, one line on what it holds still. The build-defined choices are restated here from the header of kmeans.hip:
randomness = splitmix64(seed + draw counter), first centre = draw % n; k-means++ potentials floor(d / dmax0 * 2^40) summed as
integers, the draw r = floor(rng * total / 2^64) picks the first index whose running sum exceeds r; RANDOM walks a Fisher-Yates
permutation (draw i uses splitmix64(seed + (n - i)) % (i + 1)) and skips entries closer than 1e-16 to a chosen centre; means are
integer sums of the elements scaled by 2^(40 - e), e = the binary exponent of the largest |element| (amax < 2^e)."""
import functools

import numpy as np

f32 = np.float32
RANDOM, GONZALES, KMEANSPP = 0, 1, 2
MASK = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def first_centre(seed, n):
    return splitmix64(seed) % n


def permutation(seed, n):
    p = list(range(n))
    for i in range(n - 1, 0, -1):
        j = splitmix64(seed + (n - i)) % (i + 1)
        p[i], p[j] = p[j], p[i]
    return p


def kmeanspp_picks(dist, x, k, seed):
    """the k-means++ draws by Python integers; dist(i, c) = the float32 functor value. -> the chosen rows, in the order drawn"""
    n = len(x)
    chosen = [first_centre(seed, n)]
    closest = np.full(n, np.inf)
    dmax0 = None
    for step in range(1, k):
        c = chosen[-1]
        closest = np.minimum(closest, np.array([dist(i, c) for i in range(n)], np.float64))
        if step == 1:
            dmax0 = float(closest.max())
        if not dmax0 > 0:
            break
        q = [int(float(d) / dmax0 * float(1 << 40)) if d > 0 else 0 for d in closest]
        total = sum(q)
        if total == 0:
            break
        r = (splitmix64(seed + step) * total) >> 64
        run = 0
        for i in range(n):
            if q[i] and run + q[i] > r:
                chosen.append(i)
                break
            run += q[i]
    return chosen


def case(name, x, k, init, seed=0, max_iterations=100, metric=0, pins="", **extra):
    return dict(name=name, x=np.ascontiguousarray(x, f32), k=k, init=init, seed=seed, max_iterations=max_iterations, metric=metric, pins=pins, **extra)


def mirrored():
    """GONZALES ties: pairs +-v about the point every seed here starts from (row 4), on dyadic coordinates so that float32 distances
    tie exactly; the lower row of each pair must win"""
    v = np.array([[3, 0], [0, 3], [2, 2], [1, 0.5]])
    x = np.concatenate([v[:2], -v[:2], [[0, 0]], v[2:], -v[2:], [[0.25, 0.125]]]) + 8.0      # rows 0..3 at distance 9, row 4 the middle
    seed = next(s for s in range(64) if first_centre(s, len(x)) == 4)
    return case("gonzales-ties", x, 6, GONZALES, seed, max_iterations=0, pins="GONZALES: the farthest point, the lowest row among float32 ties (mirrored "
                "points), chosen rows returned untouched at max_iterations = 0")


def blocks(n):
    """k-means++ over n points whose last row is an outlier: a seed is chosen (by the restatement) whose draws land in the last,
    partial block of 1024 as well as in an earlier one"""
    rng = np.random.default_rng(n)
    x = rng.random((n, 6)).astype(f32)
    x[-1] += 10.0
    x[-2] -= 2.0
    return x


def kmeanspp_block_case(n, ora):
    x = blocks(n)
    dist = lambda i, c: ora.distance(0, x[i], x[c])
    last = (n - 1) // 1024
    for seed in range(64):
        picks = kmeanspp_picks(dist, x, 6, seed)
        blk = [p // 1024 for p in picks[1:]]
        if last in blk and (last == 0 or min(blk) < last):
            return case(f"kmeanspp-{n}", x, 6, KMEANSPP, seed, max_iterations=0, picks=picks,
                        pins=f"k_km_select at n = {n}: a draw in the partial last block of 1024 and one before it")
    raise AssertionError("no seed reaches the last block")


def random_run():
    """RANDOM: the 70 permutation entries after the first centre coincide with it, so the cursor crosses the 64-lane window"""
    n, seed = 200, 3
    rng = np.random.default_rng(41)
    x = rng.integers(0, 64, (n, 5)).astype(f32)
    x[:, 4] = np.arange(n)                                           # all rows distinct
    p = permutation(seed, n)
    x[p[1:71]] = x[p[0]]
    return case("random-run", x, 4, RANDOM, seed, perm=p, pins="RANDOM skips a run of 70 permutation entries that coincide with the first centre: "
                "more than the 64 lanes one ballot sees")


def emptied():
    """found with the CPU oracle: RANDOM centres (seed 5) whose first Lloyd round leaves cluster 1 without members, so that
    k_km_fix_empty hands it the first member of the next cluster with more than one"""
    x = np.random.default_rng(255).integers(0, 16, (14, 2)).astype(f32)
    return case("fix-empty", x, 4, RANDOM, 5, pins="a Lloyd round empties a cluster: k_km_fix_empty hands it the first point of the next populated one")


def clustered(dim, metric=0, n=300, k=7):
    rng = np.random.default_rng(100 + dim)
    centres = rng.random((k, dim))
    x = centres[rng.integers(0, k, n)] + 0.9 * rng.random((n, dim))              # overlapping blobs: several rounds
    return case(f"converge-{'chi2' if metric else 'l2'}-{dim}", x, k, KMEANSPP, 1, metric=metric, converge=True,
                pins=f"Lloyd to convergence at dim {dim}: wave_functor on rows that are only 4-byte aligned, integer means, exact assignment")


def static_cases():
    rng = np.random.default_rng(9)
    distinct = rng.integers(0, 32, (7, 3)).astype(f32); distinct[:, 2] = np.arange(7)
    two = np.tile([[1.0, 2.0, 3.0]], (9, 1)); two[[2, 5, 6]] = [4.0, 0.0, 1.0]
    out = [mirrored(), random_run(), emptied()]
    for init, nm in ((RANDOM, "random"), (GONZALES, "gonzales"), (KMEANSPP, "kmeanspp")):
        out.append(case(f"all-equal-{nm}", np.tile([[0.5, 0.25, 2.0, 1.0]], (40, 1)), 4, init, 2, pins="all points coincide: one centre, fewer than asked"))
        out.append(case(f"two-values-{nm}", two, 5, init, 1, pins="two distinct values and k = 5: two centres"))
        out.append(case(f"k1-{nm}", distinct, 1, init, 4, pins="k = 1: no chooser step runs"))
        out.append(case(f"k-is-n-{nm}", distinct, 7, init, 4, pins="k = n: every point a centre, k_km_fix_empty is not launched"))
        out.append(case(f"k-above-n-{nm}", distinct, 10, init, 4, pins="k = n + 3 is clamped to n"))
        out.append(case(f"no-lloyd-{nm}", blocks(300), 5, init, 6, max_iterations=0, pins="max_iterations = 0: the chosen rows are returned untouched"))
    out += [clustered(33), clustered(35), clustered(33, metric=1), clustered(8)]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return {c["name"]: c for c in static_cases()}


BLOCK_N = (1023, 1024, 1025, 2049)

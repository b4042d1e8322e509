"""The workgroup reductions and the ordered compaction step of common.h (block_*, BlockRank) through the C ABI (-m gpu), at the sizes
where a wave (64) or a chunk (256 / 1024) boundary can go wrong.

Cloud reductions and global regions: objects of 1 .. 1025 points whose coordinates are multiples of 2^-10 below 2^10, so every double
partial sum is exact in any order and the centroid must be THE float of the float64 mean. Every object ends in a tail of up to 65
points above the rest in z, each tail group in grid cells of its own, so the tail points are the last of the cell-sorted span and three
balls select exactly its last 1, 64 and 65 points. No entry exposes the bounding box, so it is not checked here.
Ordered compaction: the exact radius scan on integer-valued words with the hits at rows {0, 63, 64, 255, 256, n - 1}, everywhere, nowhere.
Statistical outlier removal: 257 points on an integer lattice (mean distances dyadic: exact double sums) with one NaN point.
Normals from frames: 257 points of which rows 63, 64 and 256 are isolated (invalid frames), the count that crosses a wave and a chunk.

k-means++ across the 1024-point block of k_km_block_sums / k_km_select (n = 1025, 2049, bit-equal to the oracle) is asserted by
test_gpu_kmeans_edges.py::test_kmeanspp_draws_in_the_partial_last_block and not repeated here."""
import numpy as np
import pytest

import frontend_scenes as fs
import normals_ref as nr
from test_gpu_frontend import Batch
from test_gpu_threshold import T, bare_cb

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
NAN_LAST = (65, 257)                 # these objects end in a point with a NaN coordinate
CELL = 64.0
TAILS = (1, 64, 65)
_cloud_run = {}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dyadic(rng, n, lo, hi):
    """n coordinates in [lo, hi), multiples of 2^-10"""
    return (rng.integers(int(lo * 1024), int(hi * 1024), n) / 1024.0).astype(f32)


def tail_object(rng, n):
    """n points in input order: the main part (z in [-1000, 0)), then the tail in z order: one point at z = 400 (65 finite points or
    more), up to 63 at z in [600, 700), the last at z = 1000; x, y of the tail within 32 of (100, -200). A NaN point, when the size asks
    for one, comes last and belongs to neither."""
    nf = n - (1 if n in NAN_LAST else 0)
    t = min(65, nf)
    P = np.stack([dyadic(rng, nf, -1000, 1000), dyadic(rng, nf, -1000, 1000), dyadic(rng, nf, -1000, 0)], 1)
    z_tail = np.concatenate([[400.0] if t == 65 else [], np.sort(dyadic(rng, max(min(t, 64) - 1, 0), 600, 700)), [1000.0]])
    P[nf - t:, 0] = 100 + dyadic(rng, t, -32, 32)
    P[nf - t:, 1] = -200 + dyadic(rng, t, -32, 32)
    P[nf - t:, 2] = z_tail.astype(f32)
    if nf < n:
        P = np.concatenate([P, np.array([[5.0, np.nan, 7.0]], f32)])
    return P.astype(f32)


# a ball per tail length: (centre z, radius) round (100, -200, z); decided by margins of 50 and more
TAIL_BALL = {1: (1000.0, 100.0), 64: (850.0, 300.0), 65: (700.0, 350.0)}


def cloud_case():
    rng = np.random.default_rng(2024)
    objs = [tail_object(rng, n) for n in SIZES]
    regions = [(o, None) for o in range(len(objs))]
    for o, P in enumerate(objs):
        nf = int(np.isfinite(P).all(1).sum())
        regions += [(o, k) for k in TAILS if k <= nf]
    return objs, regions


def centroid_of(P):
    """make_grid_meta's cast: the float of (float64 sum / count)"""
    return (P.astype(f64).sum(0) / f64(len(P))).astype(f32)


def radius_of(P, c):
    """k_cloud_radii's float arithmetic; a NaN row never compares greater"""
    d = (P - c).astype(f32)
    d2 = ((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32) + (d[:, 2] * d[:, 2]).astype(f32)
    d2 = d2.astype(f32)
    return np.sqrt(d2[~np.isnan(d2)]).astype(f32).max() if (~np.isnan(d2)).any() else f32(0)


def cloud_run(pkg, gpu):
    if _cloud_run:
        return _cloud_run
    ctx, dev = gpu
    objs, regions = cloud_case()
    zero = [np.zeros_like(P) for P in objs]
    b = Batch(pkg, ctx, dev, list(zip(objs, zero)), [np.zeros((0, 3), f32)] * len(objs), CELL)
    try:
        cc = pkg.capi.cloud_centroids(ctx, b.cloud, dev)
        obj = [o for o, _ in regions]
        cen = [(0, 0, 0) if k is None else (100.0, -200.0, TAIL_BALL[k][0]) for _, k in regions]
        rad = [-1.0 if k is None else TAIL_BALL[k][1] for _, k in regions]
        out = pkg.capi.global_short_shot(ctx, b.cloud, dev, obj, cen, rad, bins=(2, 2, 8))
        _cloud_run.update(objs=objs, regions=regions, centroid=cc.cpu().numpy(), radius=pkg.capi.cloud_radii(ctx, b.cloud, cc).cpu().numpy(),
                          region={k: v.cpu().numpy() for k, v in out.items()})
        ctx.sync()
    finally:
        b.close()
    return _cloud_run


def test_cloud_centroid_count_and_radius(pkg, gpu):
    r = cloud_run(pkg, gpu)
    for o, P in enumerate(r["objs"]):
        fin = P[np.isfinite(P).all(1)]
        assert len(fin) == SIZES[o] - (1 if SIZES[o] in NAN_LAST else 0)
        assert int(r["region"]["n_sel"][o]) == len(fin), o                       # whole-object region o: the finite count
        c = centroid_of(fin)
        print("object %d: n %d centroid %s radius %.9g" % (o, len(P), r["centroid"][o], r["radius"][o]))
        assert np.array_equal(bits(r["centroid"][o]), bits(c)), (o, r["centroid"][o], c)
        assert bits(r["radius"][o:o + 1])[0] == bits([radius_of(P, c)])[0], o    # over the caller's arrays, the NaN point included


def test_global_regions_over_the_tail_of_the_sorted_span(pkg, gpu):
    r = cloud_run(pkg, gpu)
    got = r["region"]
    seen = set()
    for i, (o, k) in enumerate(r["regions"]):
        P = r["objs"][o]
        fin = P[np.isfinite(P).all(1)]
        sel = fin if k is None else fin[len(fin) - k:]
        if k is not None:                                                       # the ball selects the last k finite points and nothing else
            q = np.array([100.0, -200.0, TAIL_BALL[k][0]])
            d = np.linalg.norm(fin.astype(f64) - q, axis=1)
            assert np.array_equal(np.nonzero(d < TAIL_BALL[k][1])[0], np.arange(len(fin) - k, len(fin)))
            assert np.abs(d - TAIL_BALL[k][1]).min() > 40
            if k < len(fin):                                                    # two cell edges (<= 2000 / 30.5 each) apart in z: cells of their own
                assert fin[len(fin) - k:, 2].min() - fin[:len(fin) - k, 2].max() > 2 * 2000 / 30.5
            seen.add(k)
        assert int(got["n_sel"][i]) == len(sel), (o, k)
        c = centroid_of(sel)
        assert np.array_equal(bits(got["centroid"][i]), bits(c)), (o, k, got["centroid"][i], c)
        assert bits(got["radius"][i:i + 1])[0] == bits([radius_of(sel, c)])[0], (o, k)
        if k is None:
            assert np.array_equal(bits(got["centroid"][i]), bits(r["centroid"][o]))
    assert seen == set(TAILS)


@pytest.mark.parametrize("n_words", [255, 256, 257, 513])
def test_exact_radius_scan_lists_rows_in_order(pkg, gpu, n_words):
    """query 0 = (0.25, 0.5, 0, 0): a hit row (a, b, 0, 0), a, b in {0, 1}, lies at 0.3125 or 0.8125, every other row (third
    coordinate >= 2) at 4 or more; query 1 = (10, 10, 10, 10) lies at 200 or more of every row. Threshold 1: the hit rows / none;
    threshold 1000: every row, for both. All values exact in float."""
    ctx, dev = gpu
    rng = np.random.default_rng(n_words)
    words = rng.integers(0, 4, (n_words, 4)).astype(f32)
    words[:, 2] = rng.integers(2, 4, n_words)
    hits = np.array(sorted({0, 63, 64, 255, 256, n_words - 1} & set(range(n_words))))
    words[hits] = 0
    words[hits, :2] = rng.integers(0, 2, (len(hits), 2))
    q = np.array([[0.25, 0.5, 0, 0], [10, 10, 10, 10]], f32)
    d = ((q[:, None, :] - words[None, :, :]).astype(f64) ** 2).sum(-1)
    cb = bare_cb(pkg, ctx, words)
    before = ctx.timer("knn_threshold_mfma_launches")[0]
    try:
        for thr in (1.0, 1000.0):
            off, idx, dist = pkg.capi.knn_threshold(ctx, cb, 0, T(q, dev), thr)
            idx = idx.cpu().numpy() if idx is not None else np.zeros(0, np.int32)
            dist = dist.cpu().numpy() if dist is not None else np.zeros(0, f32)
            for i in range(2):
                want = np.nonzero(d[i] < thr)[0]
                assert off[i + 1] - off[i] == len(want), (thr, i)
                assert np.array_equal(idx[off[i]:off[i + 1]], want), (thr, i)
                assert np.array_equal(bits(dist[off[i]:off[i + 1]]), bits(d[i][want].astype(f32))), (thr, i)
            if thr == 1.0:
                assert np.array_equal(np.nonzero(d[0] < thr)[0], hits) and not (d[1] < thr).any()
            else:
                assert (d < thr).all()
        assert ctx.timer("knn_threshold_mfma_launches")[0] == before            # the exact scan answered
    finally:
        cb.close()


def test_statistical_filter_at_257_points_with_a_nan(pkg, gpu):
    """254 lattice points x = 0 .. 253 (shuffled), outliers at x = 317 and 1000, a NaN point at index 100; MeanK 2. The mean distances
    are 1, 1.5, 64.5 and 715 (dyadic), so the double sums are exact in any order and threshold and mask are the float64 rule's."""
    ctx, dev = gpu
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.permutation(254).astype(f64), [317.0, 1000.0]])
    P = np.zeros((257, 3), f32)
    P[np.arange(257) != 100, 0] = xs
    P[100] = [3.0, np.nan, 0.0]
    fin = np.isfinite(P).all(1)
    X = P[fin, 0].astype(f64)
    D = np.sort(np.abs(X[:, None] - X[None, :]), axis=1)[:, 1:3]                # the two nearest others
    md = D.mean(1)
    assert set(np.unique(md)) == {1.0, 1.5, 64.5, 715.0}
    S, Q, N = md.sum(), (md * md).sum(), f64(len(md))
    thr = S / N + 1.0 * np.sqrt((Q - S * S / N) / (N - 1.0))
    b = Batch(pkg, ctx, dev, [(P, np.zeros_like(P))], [np.zeros((0, 3), f32)], 8.0)
    try:
        keep, got_md, got_thr = pkg.capi.filter_statistical(ctx, b.cloud, 2, 1.0)
        ctx.sync()
        keep, got_md = keep.cpu().numpy().astype(bool), got_md.cpu().numpy()
    finally:
        b.close()
    print("threshold device %.17g numpy %.17g" % (got_thr[0], thr))
    assert np.isnan(got_md[100]) and not keep[100]
    assert np.array_equal(bits(got_md[fin]), bits(md.astype(f32)))
    assert abs(got_thr[0] - thr) <= 4 * np.spacing(thr)                         # the same double operations; sqrt and division correctly rounded or a unit off
    assert np.array_equal(keep[fin], ~(md > thr)) and (~keep[fin]).sum() == 2


def test_normals_from_frames_count_invalid_rows_across_waves(pkg, gpu, ora):
    """254 points on a sphere of radius 0.3 (every frame valid) and three isolated points at rows 63, 64 and 256 (no neighbour: frame
    invalid, no PCA normal): k = 3, so rows 0, 1, 2 take pcl::eigen33's unflipped PCA normal, every other sphere row the inverted z
    axis of its frame (the oracle's, to the frame tolerance 1e-4), the isolated rows stay NaN. A miscounted k moves row 2 or 3 to the
    other rule; the two rules differ there by far more than the tolerance (asserted on the references)."""
    ctx, dev = gpu
    rng = np.random.default_rng(99)
    d = rng.normal(size=(257, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    P = (0.3 * d + np.array([0.5, -0.25, 2.0])).astype(f32)
    for j, row in enumerate((63, 64, 256)):
        P[row] = [50.0 + 10 * j, 40.0, -30.0]
    off, radius = np.array([0, 257], np.uint32), 0.25
    frames = ora.shot_lrf(off, *fs.cols(P), off, *fs.cols(P), radius)
    bad = ~np.isfinite(frames[:, 0])
    assert np.array_equal(np.nonzero(bad)[0], [63, 64, 256])
    u = nr.unoriented(off, P, radius)
    flipped, _ = nr.orient(off, P, u, 0)
    raw = nr.raw_sign(u.n)
    first_k = np.arange(257) < 3
    want = np.where(first_k[:, None], raw, np.where((~bad)[:, None], -frames[:, 6:9].astype(f64), flipped))
    assert np.isnan(want[bad]).all() and not np.isnan(want[~bad]).any()
    for row in (2, 3):                                                          # the rows a wrong count would move: the rules differ there
        assert np.abs(raw[row] + frames[row, 6:9]).max() > 1e-3
    zeros = [T(np.zeros(257, f32), dev) for _ in range(3)]
    cloud = pkg.capi.Cloud(ctx, off, *[T(c, dev) for c in fs.cols(P)], *[T(np.zeros(257, f32), dev) for _ in range(3)], 0.1)
    try:
        got = np.stack([a.cpu().numpy() for a in pkg.capi.estimate_normals(ctx, cloud, radius, *zeros)], 1)
    finally:
        ctx.sync(); cloud.close()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~bad
    err = np.abs(got[ok] - want[ok]).max(1)
    undecided = first_k[ok] & (u.margin[ok] < nr.MARGIN_MIN)                     # eigen33's sign is not determined there: either sign
    err = np.where(undecided, np.minimum(err, np.abs(got[ok] + want[ok]).max(1)), err)
    print("normals: max |got - want| %.3g" % err.max())
    assert err.max() <= 1e-4

"""B-SHOT on the device (-m gpu): ismhip_bshot_binarize and ismhip_bshot352 bit for bit against the numpy restatement bshot_ref.py (and,
where the float64 SHOT reference decides a group, against shot_ref.py), the exact integer search ismhip_knn_binary against a brute-force
Hamming search and, idx and dist bit for bit, against ismhip_knn under both metrics, the refusals, and the C++ host's route."""
import json

import numpy as np
import pytest

import bshot_ref as br
import frontend_scenes as fs
import host_binding as hb
import shot_ref
from test_bshot_cpu import KNOWN, mixed_rows
from test_gpu_frontend import Batch, T
from test_gpu_host_routes import _split, _trained
from test_gpu_parity import _cb
from test_gpu_ransac import _host_counter
from test_host_layer import _cfg

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ ismhip_bshot_binarize
def test_binarize_known_answers(pkg, gpu):
    ctx, dev = gpu
    rows = np.zeros((1, br.DIM), f32)
    rows[0, :4 * len(KNOWN)] = np.asarray([v for v, _, _ in KNOWN], f32).reshape(-1)
    got = pkg.capi.bshot_binarize(ctx, T(rows, dev)).cpu().numpy()
    want = np.zeros((1, br.DIM), f32)
    want[0, :4 * len(KNOWN)] = np.asarray([w for _, w, _ in KNOWN], f32).reshape(-1)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(br.binarize(rows)), bits(want))


def test_binarize_random_rows_and_in_place(pkg, gpu):
    """4 096 rows that mix SHOT-like values, negatives, zeros, -0.0, infinities, values whose sums overflow and whole-NaN rows: bit-equal
    to the restatement, out of place, in place, and from a source that is not 16-byte aligned (the four-dword path)"""
    ctx, dev = gpu
    rows = mixed_rows(4096)
    want = br.binarize(rows)
    src = T(rows, dev)
    got = pkg.capi.bshot_binarize(ctx, src)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert np.array_equal(bits(src.cpu().numpy()), bits(rows))             # the source is untouched
    same = pkg.capi.bshot_binarize(ctx, src, out=src)
    assert same.data_ptr() == src.data_ptr() and np.array_equal(bits(src.cpu().numpy()), bits(want))
    import torch
    flat = torch.zeros(rows.size + 1, dtype=torch.float32, device=dev)
    odd = flat[1:].view(rows.shape)
    odd.copy_(T(rows, dev))
    assert odd.data_ptr() % 16 == 4
    assert np.array_equal(bits(pkg.capi.bshot_binarize(ctx, odd).cpu().numpy()), bits(want))
    assert pkg.capi.bshot_binarize(ctx, src[:0]).shape == (0, br.DIM)


# ------------------------------------------------------------------------------------------------ ismhip_bshot352
RADIUS, LRF_RADIUS, CELL = 0.25, 0.5, 0.1


def bshot_scene():
    """an ellipsoid of 6 000 points, 40 keypoints just inside its surface and one keypoint lifted off the surface along the normal until
    its descriptor ball holds one to four points (the frame ball, twice as wide, still holds plenty)"""
    rng = np.random.default_rng(77)
    p, n = fs.ellipsoid(rng, 6000)
    kp = (p[rng.choice(6000, 40, replace=False)] * f32(0.98)).astype(f32)
    r2 = f32(float(f32(RADIUS)) * float(f32(RADIUS)))
    thin = None
    for h in np.linspace(0.2, 0.25, 501):
        c = (p[0].astype(np.float64) + h * n[0].astype(np.float64)).astype(f32)
        d = (p - c).astype(f32)
        d2 = ((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32) + (d[:, 2] * d[:, 2]).astype(f32)
        cnt = int((d2 < r2).sum())
        if 1 <= cnt <= 4:
            thin = c
            break
    assert thin is not None
    return p, n, np.concatenate([kp, thin[None, :]]).astype(f32), cnt


def check_bshot_rows(got, shot, ref):
    """device BSHOT rows against the device's own SHOT rows `shot` (bit-equal to the restatement's binarisation; a NaN row is 352 ones) and
    against the float64 SHOT reference rows `ref`, binarised by the restatement: every group it decides with a margin of four elements x the
    project's 1e-4 descriptor tolerance, and every zero-sum group -> (share of the non-zero groups left out, groups, zero-sum groups)"""
    assert np.array_equal(bits(got), bits(br.binarize(shot)))
    assert set(np.unique(got)) <= {0.0, 1.0}
    nan = np.isnan(ref[:, 0])
    assert (got[nan] == 1).all() and (br.binarize(ref[nan]) == 1).all()     # NaN row -> ones in the reference too
    live = ref[~nan].astype(np.float64)
    s, margin = br.margins(live)
    zero = s == 0
    decided = zero | (margin >= 4e-4)
    want = br.binarize(ref[~nan]).reshape(len(live), -1, 4)
    have = got[~nan].reshape(len(live), -1, 4)
    assert np.array_equal(have[decided], want[decided])
    return (~decided).sum() / max((~zero).sum(), 1), decided.size, int(zero.sum())


def test_bshot352_is_the_binarised_shot352_and_agrees_with_the_float64_reference(pkg, gpu):
    ctx, dev = gpu
    p, n, kp, thin_cnt = bshot_scene()
    b = Batch(pkg, ctx, dev, [(p, n)], [kp], CELL)
    try:
        lrf = pkg.capi.shot_lrf(ctx, b.cloud, b.kp_off, *b.tk, LRF_RADIUS)
        shot, cnt = pkg.capi.shot352(ctx, b.cloud, b.kp_off, *b.tk, lrf, RADIUS, want_counts=True)
        got, bcnt = pkg.capi.bshot352(ctx, b.cloud, b.kp_off, *b.tk, lrf, RADIUS, want_counts=True)
        ctx.sync()
        lrf, shot, cnt, got, bcnt = (x.cpu().numpy() for x in (lrf, shot, cnt, got, bcnt))
    finally:
        b.close()
    assert got.shape == (41, br.DIM) and np.array_equal(cnt, bcnt)
    assert np.isfinite(lrf).all() and cnt[40] == thin_cnt < 5 and (cnt[:40] >= 5).all()
    assert np.isnan(shot[40]).all() and np.isfinite(shot[:40]).all()
    # bit-equal to the restatement applied to ismhip_shot352's own rows; the thin keypoint's NaN row is 352 ones
    assert np.array_equal(bits(got), bits(br.binarize(shot)))
    assert (got[40] == 1).all() and set(np.unique(got)) <= {0.0, 1.0}
    # the float64 SHOT reference (rows as shot_ref returns them), binarised by the restatement: every group it decides with a margin of
    # four elements x the project's 1e-4 descriptor tolerance, and every zero-sum group
    ref, rcnt = shot_ref.describe([(p, n)], [kp], [lrf], RADIUS)
    assert np.array_equal(rcnt, cnt.astype(np.uint32))
    assert np.isnan(ref[40]).all() and np.isfinite(ref[:40]).all()
    left_out, groups, zero = check_bshot_rows(got, shot, ref)
    print(f"groups: {groups}, zero-sum {zero}, non-zero left out share {left_out:.3f}")
    assert left_out <= 0.30


# ------------------------------------------------------------------------------------------------ ismhip_knn_binary
def random_bits(rng, n, dim, density=0.3):
    return (rng.random((n, dim)) < density).astype(f32)


def planted_words(rng, n_words, dim):
    """random rows with planted ones: duplicates of row 0 spread over the codebook (different tiles and splits once n_words allows), an
    all-zero and an all-one row, and a block of asymmetric rows where row r has exactly bit r mod dim set"""
    w = random_bits(rng, n_words, dim)
    for j in (n_words // 3, n_words // 2, n_words - 1):
        w[j] = w[0]
    if n_words >= 8:
        w[5] = 0; w[6] = 1
    for r in range(n_words // 4, n_words // 2 - 1):
        w[r] = 0; w[r, r % dim] = 1
    return w


def planted_queries(rng, words, nq):
    dim = words.shape[1]
    q = random_bits(rng, nq, dim)
    q[0] = words[0]                                                        # equal to several rows: the lowest must win
    if nq >= 8:
        q[1] = 0; q[2] = 1
        q[3] = words[len(words) - 1]
        for i in range(4, min(nq, 40)):                                    # single bits: nearest rows are the asymmetric ones, in row order
            q[i] = 0; q[i, (i * 7) % dim] = 1
        flip = q[7].copy(); flip[:] = words[len(words) // 2]; flip[0] = 1 - flip[0]
        q[7] = flip
    return q


def check_search(pkg, gpu, words, q, ks, cb=None):
    """ismhip_knn_binary == brute force == ismhip_knn (both metrics), idx and dist bit for bit"""
    ctx, dev = gpu
    own = cb is None
    if own:
        _, cb = _cb(pkg, gpu, words)
        cb.make_binary()
    assert cb.has_binary
    tq = T(q, dev)
    for k in ks:
        idx, dist = pkg.capi.knn_binary(ctx, cb, tq, k)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        widx, wdist = br.hamming_knn(words, q, k)
        assert np.array_equal(idx, widx), k
        assert np.array_equal(bits(dist)[widx >= 0], bits(wdist)[widx >= 0]) and np.isnan(dist[widx < 0]).all(), k
        for metric in (pkg.capi.METRIC_L2SQ, pkg.capi.METRIC_CHI2):
            fidx, fdist = pkg.capi.knn(ctx, cb, metric, tq, k)
            assert np.array_equal(idx, fidx.cpu().numpy()), (k, metric)
            assert np.array_equal(bits(dist), bits(fdist.cpu().numpy())), (k, metric)
    if own:
        cb.close()


@pytest.mark.parametrize("n_words", [1, 127, 129, 1000])
@pytest.mark.parametrize("dim", [352, 33, 1344])
def test_knn_binary_equals_brute_force_and_the_float_search(pkg, gpu, dim, n_words):
    """none of the three dims is a multiple of the 128-byte K step: 33, 352 and 1344 exercise the zero padding to 128, 384 and 1408; n_words 1 and 127 fit one 128-row tile, 129
    needs two; 1000 spreads the duplicates over eight tiles. k = 16 exceeds n_words = 1. More than one codebook split, and with it the
    merge over splits, is used as soon as there is more than one tile and fewer than 1024 query tiles: the smallest such launch is
    n_words = 129 with any nq <= 130 944, so every case here with n_words >= 129 takes it."""
    ctx, dev = gpu
    rng = np.random.default_rng(dim * 10007 + n_words)
    words = planted_words(rng, n_words, dim)
    _, cb = _cb(pkg, gpu, words)
    cb.make_binary()
    for nq in (1, 63, 257):
        check_search(pkg, gpu, words, planted_queries(rng, words, nq), (1, 3, 16), cb=cb)
    cb.close()


def test_knn_binary_asymmetric_rows_pin_the_lane_map(pkg, gpu):
    """codeword r has exactly bit r mod dim set, query i exactly bit (5 i + 3) mod dim: the distance is 0 for the rows r = bit (mod dim)
    and 2 elsewhere, so the answer is {bit, bit + dim, ...} then the lowest other rows. A swapped row / column map, a transposed tile or
    a k order that differs between the operands cannot produce it."""
    dim, n_words, nq = 352, 1000, 300
    words = np.zeros((n_words, dim), f32); words[np.arange(n_words), np.arange(n_words) % dim] = 1
    q = np.zeros((nq, dim), f32); bit = (5 * np.arange(nq) + 3) % dim; q[np.arange(nq), bit] = 1
    idx, dist = br.hamming_knn(words, q, 3)
    assert np.array_equal(idx[:, 0], bit) and np.array_equal(idx[:, 1], bit + dim) and (dist[:, :2] == 0).all()
    check_search(pkg, gpu, words, q, (1, 3))


def test_knn_binary_many_tiles_per_split(pkg, gpu):
    """16 500 words = 129 tiles against 2 000 queries = 16 query tiles: 64 splits are asked for, so every workgroup sweeps three tiles
    (the prefetch across a tile boundary) and the merge combines 43 splits; duplicates of row 0 sit in different splits"""
    rng = np.random.default_rng(3)
    words = planted_words(rng, 16500, 352)
    check_search(pkg, gpu, words, planted_queries(rng, words, 2000), (1, 3))


def test_knn_binary_one_split(pkg, gpu):
    """131 200 queries = 1 025 query tiles: one split, every workgroup sweeps all three tiles of 300 words"""
    rng = np.random.default_rng(4)
    words = planted_words(rng, 300, 33)
    check_search(pkg, gpu, words, planted_queries(rng, words, 131200), (1,))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(pkg, gpu):
    ctx, dev = gpu
    rng = np.random.default_rng(9)
    words = random_bits(rng, 200, 352)
    q = random_bits(rng, 20, 352)
    bad = words.copy(); bad[150, 17] = 0.5
    _, cb = _cb(pkg, gpu, bad)
    with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\).*neither 0 nor 1"):
        cb.make_binary()
    assert not cb.has_binary
    with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\).*no binary image"):
        pkg.capi.knn_binary(ctx, cb, T(q, dev), 1)
    idx, _ = pkg.capi.knn(ctx, cb, pkg.capi.METRIC_L2SQ, T(q, dev), 1)     # the float search still answers
    d = ((q[:, None, :] - bad[None, :, :]) ** 2).sum(2)
    assert np.array_equal(idx.cpu().numpy()[:, 0], d.argmin(1))
    cb.close()
    _, cb = _cb(pkg, gpu, np.where(words == 0, f32(-0.0), words))          # -0.0 counts as 0
    cb.make_binary(); cb.make_binary()
    assert cb.has_binary
    q2 = q.copy(); q2[3, 351] = 2.0
    with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\).*query element"):
        pkg.capi.knn_binary(ctx, cb, T(q2, dev), 1)
    q2[3, 351] = np.nan
    with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\).*query element"):
        pkg.capi.knn_binary(ctx, cb, T(q2, dev), 1)
    for k in (0, 17):
        with pytest.raises(pkg.capi.IsmHipError, match=r"\(-1\)"):
            pkg.capi.knn_binary(ctx, cb, T(q, dev), k)
    idx, dist = pkg.capi.knn_binary(ctx, cb, T(q[:0], dev), 1)             # nq = 0
    assert idx.shape == (0, 1)
    cb.close()


# ------------------------------------------------------------------------------------------------ host route
@pytest.mark.parametrize("distance", ["Euclidean", "ChiSquared"])
def test_host_route_gives_the_maxima_of_the_float_route(pkg, gpu, tmp_path, monkeypatch, distance):
    """Train and detect with Features type "BSHOT" (Clustering None, K = 1): the maxima with the binary search are those of the same model
    with ISMHIP_KNN_BINARY=0 (read when the host creates its context), and the counter shows which search ran."""
    train, test, order = _split(pkg)
    m = _trained(_cfg(**{"Children/Features/Type": "BSHOT", "Parameters/DistanceType": distance}), train, order)
    assert m.codebook_size() > 100
    words = m.codebook(br.DIM, 3)[0]
    assert set(np.unique(words)) <= {0.0, 1.0}
    path = str(tmp_path / "bshot.ism")
    m.write(path)
    m.close()
    assert json.load(open(path))["ObjectConfig"]["Children"]["Features"]["Type"] == "BSHOT"
    nb = test.batch(range(6))
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("ISMHIP_KNN_BINARY", route)
        d = hb.Model()
        d.read(path)
        out[route] = d.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=8)
        out[route, "launches"] = _host_counter(d, "knn_binary_launches")
        d.close()
    monkeypatch.delenv("ISMHIP_KNN_BINARY")
    assert out["1", "launches"] == 1 and out["0", "launches"] == 0
    assert (out["1"]["n"] > 0).all()
    np.testing.assert_array_equal(out["1"]["n"], out["0"]["n"])
    for o in range(6):
        k = int(out["1"]["n"][o])
        for key in ("cls", "weight", "pos", "inst", "n_votes"):
            np.testing.assert_array_equal(out["1"][key][o, :k], out["0"][key][o, :k])

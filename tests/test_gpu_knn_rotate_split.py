"""Query batches rotated on the f16 matrix cores (k_rotate_split16, csrc/pca.hip): R and the descriptors are split
into two f16 halves each, Rh xh + Rh xl + Rl xh is accumulated in fp32, and the pass leaves |q|^2 and the image rows' sums of squares
for the proofs. Checked here: the image against float64 with the constants the proofs use, the two norm arrays, answers bit for bit
the oracle's and byte for byte those of the FP32 rotation (ISMHIP_KNN_ROTATE_F32=1), and that a useless image still only costs time."""
import numpy as np
import pytest

from test_gpu_knn_stage2_seed import (CLUSTER, DIM, N_WORDS, NOISE, NQ, Q_BIG, Q_CLUSTER, Q_DUP, Q_EXACT, Q_NAN, Q_TINY, T, bare_cb,
                                      steep_spectrum_data)

pytestmark = pytest.mark.gpu

N_ROWS = 300          # two full 128-row workgroup tiles and a ragged one
R_ZERO, R_ONE, R_TINY, R_NEG, R_EDGE, R_INSIDE, R_BEYOND, R_NAN = 3, 130, 131, slice(132, 140), 257, 258, 259, 299
F16_MAX = 65504.0


def probe_rows(rng, words, dim, R, scale):
    """the rows of check 1; those tied to the image's scale are made from the first basis vector"""
    length = float(np.linalg.norm(words, axis=1).mean())
    x = rng.random((N_ROWS, dim)).astype(np.float32)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True) * length).astype(np.float32)      # random rows as long as a codeword
    x[R_ZERO] = 0.0
    x[R_ONE] = 0.0; x[R_ONE, dim // 2] = 1.0
    x[R_TINY] *= 1e-6
    x[R_NEG] *= np.where(rng.random((8, dim)) < 0.5, -1.0, 1.0).astype(np.float32)
    x[R_EDGE] = 2.0 ** -20                                                # low halves at the f16 subnormal edge
    r0 = R[0, :dim].astype(np.float64); r0 /= np.linalg.norm(r0)
    x[R_INSIDE] = (0.9 * F16_MAX / scale * r0).astype(np.float32)         # leading coordinate at 0.9 of the f16 range
    x[R_BEYOND] = (1.1 * F16_MAX / scale * r0).astype(np.float32)         # ... and past it
    x[R_NAN, 7] = np.nan
    return x


def check_image(cb, dev, rng, words, m):
    dim = words.shape[1]
    head = cb.rotate_probe(T(np.zeros((1, dim), np.float32), dev))
    assert head is not None and head[0].shape[1] == m, (None if head is None else head[0].shape, m)
    _, _, _, R, scale, _, _ = head
    x = probe_rows(rng, words, dim, R, scale)
    img, qn2, qn2h, R2, scale2, d_rel, d_abs = cb.rotate_probe(T(x, dev))
    assert img.shape == (N_ROWS, m) and np.array_equal(R, R2) and scale == scale2 and d_rel > 0 and d_abs > 0
    img64 = img.astype(np.float64)
    x64 = np.zeros((N_ROWS, R.shape[1])); x64[:, :dim] = x
    finite = np.isfinite(img64).all(axis=1)
    assert list(np.flatnonzero(~finite)) == [R_BEYOND, R_NAN], np.flatnonzero(~finite)
    assert np.isinf(img64[R_BEYOND]).any() and not np.isnan(img64[R_BEYOND]).any()       # a too-long row overflows to inf
    assert np.isnan(img64[R_NAN]).all()                                   # NaN spreads to every coordinate, as a product with it does
    assert np.isinf(qn2h[R_BEYOND]) and np.isnan(qn2h[R_NAN]) and np.isnan(qn2[R_NAN])
    assert np.all(img64[R_ZERO] == 0.0)
    # |x^ / scale - R x|_2 <= d_rel |x|_2 + d_abs with the returned constants, in float64
    err = np.linalg.norm(img64[finite] / scale - x64[finite] @ R.astype(np.float64).T, axis=1)
    bound = d_rel * np.linalg.norm(x64[finite], axis=1) + d_abs
    worst = float(np.max(err / bound))
    print(f"dim {dim} m {m}: scale {scale:g} d_rel {d_rel:.3e} d_abs {d_abs:.3e}, largest error / bound {worst:.3f}")
    assert np.all(err <= bound), (np.flatnonzero(finite)[err > bound], worst)
    # the norm arrays: float64 sums of what they claim to sum, to fp32 summation error
    fin2 = np.isfinite(x).all(axis=1)
    want2 = (x64[fin2] ** 2).sum(axis=1)
    assert np.all(np.abs(qn2[fin2] - want2) <= dim * 2.0 ** -24 * want2), np.max(np.abs(qn2[fin2] - want2) / np.maximum(want2, 1e-300))
    want2h = (img64[finite] ** 2).sum(axis=1)
    assert np.all(np.abs(qn2h[finite] - want2h) <= m * 2.0 ** -24 * want2h), np.max(np.abs(qn2h[finite] - want2h) / np.maximum(want2h, 1e-300))


@pytest.mark.parametrize("m", [64, 160, 256])
def test_rotated_image_meets_its_bound_in_float64(pkg, gpu, monkeypatch, m):
    """352 dimensions onto 64, 160 and 256 coordinates: the three instances of the kernel"""
    _, dev = gpu
    rng = np.random.default_rng(1000 + m)
    words, _ = steep_spectrum_data(rng, 4096, 1, 352, noise=0.3)
    monkeypatch.setenv("ISMHIP_KNN_PCA_M", str(m)); monkeypatch.setenv("ISMHIP_KNN_PCA_M2", "0")
    monkeypatch.delenv("ISMHIP_KNN_ROTATE_F32", raising=False)
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    assert cb.stage1_dims == m
    check_image(cb, dev, rng, words, m)
    cb.close(); ctx.close()


def test_identity_image_of_short_descriptors_meets_its_bound(pkg, gpu, monkeypatch):
    """33 values up to 100 padded to 64 coordinates, R = I"""
    _, dev = gpu
    rng = np.random.default_rng(33)
    words = (100.0 * rng.random((4096, 33)) ** 2).astype(np.float32)
    for var in ("ISMHIP_KNN_PCA_M", "ISMHIP_KNN_PCA_M2", "ISMHIP_KNN_ROTATE_F32"):
        monkeypatch.delenv(var, raising=False)
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    assert cb.stage1_dims == 64 and cb.stage1_energy == 1.0
    check_image(cb, dev, rng, words, 64)
    cb.close(); ctx.close()


@pytest.fixture(scope="module")
def data(ora):
    """the codebook and queries of test_gpu_knn_stage2_seed.py (same generator, same special queries), the oracle's answers once"""
    rng = np.random.default_rng(99)
    words, q = steep_spectrum_data(rng, N_WORDS, NQ, DIM, noise=NOISE)
    words[4000:4003] = words[17]                                          # duplicates: ties to the lowest row
    rows = np.asarray([CLUSTER + 16 * (i // 4) + (i % 4) for i in range(6)])
    words[rows] = words[CLUSTER]                                          # six bit-identical rows in one lane slot
    q[Q_EXACT] = words[:8]
    q[Q_DUP] = words[17]
    q[Q_BIG] *= 40.0                                                      # no image: overflows the fixed scale
    q[Q_TINY] *= 1e-6
    q[Q_NAN, 5] = np.nan
    q[Q_CLUSTER] = words[CLUSTER] + (1e-4 * rng.random((4, DIM))).astype(np.float32)
    q[16] = 0.0                                                           # a zero query
    sel = np.r_[0:11, 12:17, 20:NQ:4]                                     # (a NaN query has no defined order: compared between the two modes only)
    ref = {k: ora.knn(0, words, q[sel], k) for k in (1, 2)}
    return words, q, sel, ref


def search(pkg, dev, monkeypatch, words, q, env):
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    assert cb.stage1_dims == 64 and cb.stage2_dims == 192
    ctx.timers_enable(True)
    out = []
    for k in (1, 2):
        idx, dist = pkg.capi.knn(ctx, cb, 0, T(q, dev), k)
        gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
        out.append((gi, gd, int(ctx.timer("knn_stage2_queries")[0]), int(ctx.timer("knn_flagged_items")[0])))
    seeds = int(ctx.timer("knn_seed_launches")[0])
    cb.close(); ctx.close()
    return out, seeds


def test_answers_are_the_oracles_and_the_f32_rotations(pkg, gpu, data, monkeypatch):
    """Stage 1 on 64 rotated coordinates, the seeded stage 2 on 192 (ring kernel) and the exact scan all run, with both rotations."""
    _, dev = gpu
    words, q, sel, ref = data
    env = {"ISMHIP_KNN_PCA_M": "64", "ISMHIP_KNN_PCA_M2": "192"}
    new, seeds_new = search(pkg, dev, monkeypatch, words, q, dict(env, ISMHIP_KNN_ROTATE_F32="0"))
    old, seeds_old = search(pkg, dev, monkeypatch, words, q, dict(env, ISMHIP_KNN_ROTATE_F32="1"))
    assert (seeds_new, seeds_old) == (2, 2), (seeds_new, seeds_old)      # one seeded stage-2 launch per search, in both modes
    for k, (gi, gd, n2, items), (oi, od, on2, oitems) in zip((1, 2), new, old):
        print(f"k={k}: stage-2 queries f16 rotation {n2}, FP32 rotation {on2}; exact-scan items {items} / {oitems}")
        assert 4096 <= n2 < NQ and 4096 <= on2 < NQ, (n2, on2)            # stage 2 ran on the ring
        assert items >= 1 and oitems >= 1                                 # the six equal rows overflow their slot: the exact scan ran
        widx, wdist = ref[k]
        assert np.array_equal(gi[sel], widx), f"rows differ in {int((gi[sel] != widx).any(1).sum())} queries"
        assert np.array_equal(gd[sel].view(np.uint32), wdist.view(np.uint32))
        assert gi.tobytes() == oi.tobytes() and gd.tobytes() == od.tobytes()
        assert gi[Q_DUP, 0] == 17 and (gi[Q_CLUSTER, 0] == CLUSTER).all()  # ties: the lowest row


def test_a_flat_spectrum_still_only_costs_time(pkg, gpu, ora, monkeypatch):
    """Random vectors forced onto 192 of 352 coordinates: the partial distances bound almost nothing, nearly every stage-1 proof fails
    (the share test_knn_rotated_stage1_on_a_flat_spectrum_falls_back asks for) and the answers stay the oracle's. A bound that is too
    tight shows here as wrong rows."""
    _, dev = gpu
    rng = np.random.default_rng(5)
    words = rng.normal(size=(4096, 352)).astype(np.float32)
    q = rng.normal(size=(8192, 352)).astype(np.float32)
    q[:5] = words[:5]
    monkeypatch.setenv("ISMHIP_KNN_PCA_M", "192")
    monkeypatch.delenv("ISMHIP_KNN_ROTATE_F32", raising=False)
    ctx = pkg.capi.Ctx(0)
    cb = bare_cb(pkg, ctx, words)
    assert cb.stage1_dims == 192 and cb.stage1_energy < 0.7
    ctx.timers_enable(True)
    idx, dist = pkg.capi.knn(ctx, cb, 0, T(q, dev), 2)
    n2 = int(ctx.timer("knn_stage2_queries")[0])
    print(f"stage-2 queries {n2} of {len(q)}")
    widx, wdist = ora.knn(0, words, q, 2)
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(dist.cpu().numpy(), wdist)
    assert n2 > len(q) * 2000 // 4500, n2
    cb.close(); ctx.close()

"""ESF_LOCAL on the device (-m gpu): ismhip_esf_local through capi on the scenes of esf_scenes.py against the restatement esf_ref.py,
which is run on the DEVICE's own centroid and largest distance (scale_out, held to the bound of the order-free sum first). Neighbour
counts and NaN patterns are equal; for every keypoint the restatement decides as a whole, lo <= bin_counts_out <= hi in every bin, hence
bit-equal where lo == hi; desc_out is bit for bit (float)N_i / (float)sum N of the device's own counts. Then byte equality across two
calls, two cell sizes, the forced staging capacity and the copied neighbourhood, the refusals, and the codeword search at D = 640.
test_esf_local_cpu.py proves on the host that the scenes sit where they claim."""
import numpy as np
import pytest

import esf_ref as ref
import esf_scenes as scenes
from test_gpu_parity import T, _cb

pytestmark = pytest.mark.gpu
F = np.float32


def run_scene(pkg, gpu, s, cell_scale=0.4, radius=None, n_samples=None, seed=ref.SEED):
    """-> (rows [K, 640], cnt [K], bins [K, 640], scale [K, 4]) of the device on the scene dict s"""
    ctx, dev = gpu
    capi = pkg.capi
    nrm = np.zeros_like(s["xyz"]); nrm[:, 2] = 1
    t = [T(s["xyz"][:, i], dev) for i in range(3)] + [T(nrm[:, i], dev) for i in range(3)]
    tk = [T(s["kp"][:, i], dev) for i in range(3)]
    cloud = capi.Cloud(ctx, s["pt_off"], *t, cell_scale * s["radius"])
    try:
        rows, cnt, bins, scale = capi.esf_local(ctx, cloud, s["kp_off"], *tk, s["radius"] if radius is None else radius,
                                                n_samples=s["n_samples"] if n_samples is None else n_samples, seed=seed,
                                                want_counts=True, want_bins=True, want_scale=True)
        ctx.sync()
        return rows.cpu().numpy(), cnt.cpu().numpy().astype(np.int64), bins.cpu().numpy().astype(np.int64), scale.cpu().numpy()
    finally:
        cloud.close()


def check_rows_from_counts(rows, bins):
    """desc_out is one rounding from the device's own integers; a finite row sums to 1 within 640 roundings"""
    nan = np.isnan(rows[:, 0])
    assert np.array_equal(np.isnan(rows), np.broadcast_to(nan[:, None], rows.shape)) and not bins[nan].any()
    tot = bins[~nan].sum(1)
    assert (tot > 0).all()
    want = (bins[~nan].astype(F) / tot.astype(F)[:, None]).astype(F)
    assert np.array_equal(rows[~nan].view(np.uint32), want.view(np.uint32))
    assert (np.abs(rows[~nan].astype(np.float64).sum(1) - 1.0) <= 640 * 2.0 ** -24).all()


def check_scene(s, out):
    rows, cnt, bins, scale = out
    K = len(s["kp"])
    assert rows.shape == (K, ref.DIM) and bins.shape == (K, ref.DIM) and scale.shape == (K, 4)
    a = ref.esf_local(s["pt_off"], s["xyz"], s["kp_off"], s["kp"], s["radius"], s["n_samples"], scale=scale)
    assert np.array_equal(cnt, a["cnt"])
    check_rows_from_counts(rows, bins)
    # the scale: NaN where there is no row to scale, else within the bounds of the order-free sum and of the float32 distance
    assert np.isnan(scale[a["cnt"] < 3]).all() and np.isfinite(scale[a["cnt"] >= 3]).all()
    for k in np.nonzero(a["cnt"] >= 3)[0]:
        c64, c_err, m64, m_err = ref.scale_bounds(s["xyz"][a["balls"][k]], s["kp"][k], s["radius"], scale[k, :3])
        assert (np.abs(scale[k, :3].astype(np.float64) - c64) <= c_err).all(), (k, scale[k], c64, c_err)
        assert abs(float(scale[k, 3]) - m64) <= m_err, (k, scale[k, 3], m64, m_err)
    v = ~a["whole"]
    assert np.array_equal(np.isnan(rows[v, 0]), a["nan"][v])
    ok = v & ~a["nan"]
    below, above = bins[ok] < a["lo"][ok], bins[ok] > a["hi"][ok]
    assert not below.any() and not above.any(), (np.nonzero(ok)[0][(below | above).any(1)], np.nonzero(below | above))
    return a


@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_esf_local_matches_the_restatement(pkg, gpu, name):
    """(a) generic, (b) the neighbour counts, (c) the hand-derived triangle, (d) collinear points, (e) the disc, (f) two clusters, (g) the
    copied neighbourhood, the library's own sample count; (h) no sample count is a multiple of the 256-attempt blocks"""
    s = scenes.scene(name)
    out = run_scene(pkg, gpu, s)
    a = check_scene(s, out)
    rows, cnt, bins, scale = out
    decided = (a["lo"] == a["hi"])[~a["whole"] & ~a["nan"]]
    print("%s: %d keypoints, %d undecided as a whole, %d NaN rows, %.2f %% of the bins decided bit for bit"
          % (name, len(cnt), a["whole"].sum(), np.isnan(rows[:, 0]).sum(), 100.0 * decided.mean() if decided.size else 100.0))
    if name == "counts":
        assert cnt.tolist() == scenes.COUNTS and np.isnan(rows[:3]).all() and np.isfinite(rows[3:]).all()
    if name == "triangle":
        b = bins[0].reshape(10, 64)
        assert scale[0].tolist() == [0.0, 0.0, 0.0, 2.0]
        assert b[1, 37] == 1000 and b[1, 44] == 2000 and b[4, 63] == 3000 and b[7, 63] == 24000 and b[7, 56] == 12000 and bins[0].sum() == 42000
    if name == "collinear":
        assert np.isnan(rows).all() and cnt.tolist() == [9, 5, 5]
    if name == "disc":
        b = bins.reshape(-1, 10, 64)
        assert not b[:, [2, 5, 7, 8, 9]].any() and (b[:, 6].sum(1) == 9000).all()
    if name == "two_clusters":
        assert (bins.reshape(-1, 10, 64)[:, 9].sum(1) > 0).all()
    if name == "copy":
        assert np.array_equal(rows[:4].view(np.uint32), rows[4:].view(np.uint32)) and np.array_equal(bins[:4], bins[4:])
        assert np.array_equal(scale[:4].view(np.uint32), scale[4:].view(np.uint32)) and np.array_equal(cnt[:4], cnt[4:])


def test_not_finite_inputs(pkg, gpu):
    """a keypoint that is not finite, a ball that misses the object: NaN rows, count 0; cloud points that are not finite are no neighbours"""
    rng = np.random.default_rng(2201)
    P = (rng.normal(size=(40, 3)) * 0.05).astype(F)
    P[[3, 17]] = [[np.nan, 0, 0], [0, np.inf, 0]]
    kp = np.asarray([[np.nan, 0, 0], [100, 0, 0], [0, 0, 0], [0, 0, np.inf]], F)
    s = dict(pt_off=np.array([0, 40], np.uint32), xyz=P, kp_off=np.array([0, 4], np.uint32), kp=kp, radius=float(F(0.5)), n_samples=1000)
    out = run_scene(pkg, gpu, s)
    check_scene(s, out)
    rows, cnt, bins, scale = out
    assert cnt.tolist() == [0, 0, 38, 0] and np.isnan(rows[[0, 1, 3]]).all() and np.isfinite(rows[2]).all() and np.isnan(scale[[0, 1, 3]]).all()


@pytest.mark.parametrize("name", ["counts", "generic"])
def test_listed_path_gives_the_bytes_of_the_native_capacity(pkg, gpu, monkeypatch, name):
    """ISMHIP_ESF_CAP = 64: balls of 65 and 130 points (and most of `generic`) are read through the work list in device memory, 64 and
    below stay staged. Same bytes either way, for other capacities too."""
    s = scenes.scene(name)
    native = run_scene(pkg, gpu, s)
    for cap in (str(scenes.CAP), "3", "100"):
        monkeypatch.setenv("ISMHIP_ESF_CAP", cap)
        forced = run_scene(pkg, gpu, s)
        monkeypatch.delenv("ISMHIP_ESF_CAP")
        for x, y in zip(native, forced):
            assert np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y), cap
    check_scene(s, native)


def test_same_bytes_twice_and_on_two_cell_sizes(pkg, gpu):
    ctx, _ = gpu
    s = scenes.scene("generic")
    ctx.timers_enable(True); ctx.timers_reset()
    a = run_scene(pkg, gpu, s)
    b = run_scene(pkg, gpu, s)
    ctx.sync()
    t = ctx.timer("esf_local")
    ctx.timers_enable(False)
    assert t[1] == 2 and t[0] > 0
    c = run_scene(pkg, gpu, s, cell_scale=0.23)
    for x, y, z in zip(a, b, c):
        bits = (lambda v: v.view(np.uint32)) if x.dtype == F else (lambda v: v)
        assert np.array_equal(bits(x), bits(y)) and np.array_equal(bits(x), bits(z))
    # another seed draws other triples; fewer samples are a prefix of the same stream, not the same row
    d = run_scene(pkg, gpu, s, seed=ref.SEED + 1)
    assert np.array_equal(d[1], a[1]) and not np.array_equal(d[2], a[2])
    e = run_scene(pkg, gpu, s, n_samples=999)
    assert not np.array_equal(e[2], a[2]) and (e[2].reshape(-1, 10, 64)[:, :3].sum((1, 2))[~np.isnan(e[0][:, 0])] == 3 * 999).all()


@pytest.mark.parametrize("cap", [None, str(scenes.CAP)])
def test_more_keypoints_than_workgroups(pkg, gpu, monkeypatch, cap):
    """a launch has at most 768 workgroups, each walks its keypoints one after the other through the same LDS and the same slab of the
    work list: the eight keypoints of `counts` 96 times over (768) and then 5 times in reverse order (40), so that workgroups 0 .. 39
    meet a ball of another size the second time, give the rows of the eight, staged and listed"""
    s = dict(scenes.scene("counts"))
    first = run_scene(pkg, gpu, s)
    sel = np.concatenate([np.tile(np.arange(8), 96), np.tile(np.arange(8)[::-1], 5)])
    s["kp"] = s["kp"][sel]; s["kp_off"] = np.array([0, len(sel)], np.uint32)
    if cap:
        monkeypatch.setenv("ISMHIP_ESF_CAP", cap)
    many = run_scene(pkg, gpu, s)
    assert len(many[1]) == 808
    for x, y in zip(first, many):
        bits = (lambda v: v.view(np.uint32)) if x.dtype == F else (lambda v: v)
        assert np.array_equal(bits(x[sel]), bits(y))


def test_refused_arguments(pkg, gpu):
    Err = pkg.capi.IsmHipError
    s = scenes.scene("triangle")
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(Err, match=r"\(-1\).*esf_local: bad argument"):
            run_scene(pkg, gpu, s, radius=radius)
    for n in (0, -5, 65537):
        with pytest.raises(Err, match=r"\(-1\).*esf_local: bad argument"):
            run_scene(pkg, gpu, s, n_samples=n)
    ctx, dev = gpu
    capi = pkg.capi
    z = T(np.zeros(3, F), dev)
    cloud = capi.Cloud(ctx, s["pt_off"], z, z, z, z, z, z, 0.5)
    try:
        out = T(np.zeros((1, 640), F), dev)
        ko = np.array([0, 1], np.uint32)
        with pytest.raises(Err, match=r"\(-1\).*esf_local: bad argument"):           # a missing array
            ctx.check(capi.lib().ismhip_esf_local(ctx._h, cloud._h, capi._p(ko), capi._p(z), None, capi._p(z), capi.C.c_float(1.0),
                                                  capi.C.c_int(10), capi.C.c_uint32(1), capi._p(out), None, None, None), "ismhip_esf_local")
    finally:
        cloud.close()
    rows, cnt, bins, scale = run_scene(pkg, gpu, s, n_samples=65536)                 # the largest count is taken, and the call still works
    assert cnt.tolist() == [3] and bins[0].sum() == 42 * 65536


# ------------------------------------------------------------------------------------------------ codeword search on real rows
@pytest.fixture(scope="module")
def sphere_rows(pkg, gpu):
    """750 rows on 1500 points of a bumpy sphere: the first 750 points as keypoints, 1000 samples each"""
    rng = np.random.default_rng(2301)
    p = rng.normal(size=(1500, 3)); p /= np.linalg.norm(p, axis=1, keepdims=True)
    p *= 1.0 + 0.1 * np.sin(5 * p[:, :1]) * np.cos(4 * p[:, 1:2])
    s = dict(pt_off=np.array([0, 1500], np.uint32), xyz=p.astype(F), kp_off=np.array([0, 750], np.uint32), kp=p[:750].astype(F),
             radius=float(F(0.4)), n_samples=1000)
    rows, cnt, bins, _ = run_scene(pkg, gpu, s)
    assert rows.shape == (750, 640) and np.isfinite(rows).all() and cnt.min() > 20
    check_rows_from_counts(rows, bins)
    return rows[:600].copy(), rows[600:].copy()


@pytest.mark.parametrize("metric", [0, 1])
def test_knn_on_esf_rows(pkg, gpu, ora, sphere_rows, metric):
    """ismhip_knn at D = 640, 600 words and 150 queries with five exact hits, squared L2 and chi-square: bit-equal to ismref_knn"""
    ctx, dev = gpu
    words, q = sphere_rows
    q = q.copy(); q[:5] = words[:5]
    host, cb = _cb(pkg, gpu, words)
    try:
        for k in (1, 3):
            idx, dist = pkg.capi.knn(ctx, cb, metric, T(q, dev), k)
            widx, wdist = ora.knn(metric, words, q, k)
            assert np.array_equal(idx.cpu().numpy(), widx)
            assert np.array_equal(dist.cpu().numpy().view(np.uint32), wdist.view(np.uint32))
    finally:
        cb.close()

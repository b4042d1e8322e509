"""RSD on the device (-m gpu): ismhip_rsd through capi on the scenes of rsd_scenes.py against the restatement rsd_ref.py, in both modes.
Neighbour counts and the NaN and zero patterns are equal. Histogram mode: every bin whose count the restatement decides is compared BIT
FOR BIT ((float)count / 300.0f on either side); a bin an undecided pair may fall into must hold one of the counts of its interval.
Radii mode: a keypoint with an undecided pair is left out, the others agree within one float32 unit in the last place -- both sides apply
the same double formulas to the same extremal floats, and what two libraries' acos and division can differ by (1e-16 relative) moves the
float result by at most one rounding. test_rsd_cpu.py proves on the host that the scenes sit where they claim. Then: the tiled path
against the native capacity, two calls, a copied object and two cell sizes byte for byte, the refusals, and the codeword search on real
rows at D = 25 and D = 2."""
import numpy as np
import pytest

import rsd_ref as ref
import rsd_scenes as scenes
from test_gpu_parity import T, _cb

pytestmark = pytest.mark.gpu
F = np.float32


def run_scene(pkg, gpu, s, full, cell_scale=0.4, radius=None):
    """-> (rows [K, 25 or 2], cnt [K]) of the device on the scene dict s"""
    ctx, dev = gpu
    capi = pkg.capi
    t = [T(s["xyz"][:, i], dev) for i in range(3)] + [T(s["normals"][:, i], dev) for i in range(3)]
    tk = [T(s["kp"][:, i], dev) for i in range(3)]
    cloud = capi.Cloud(ctx, s["pt_off"], *t, cell_scale * s["radius"])
    try:
        rows, cnt = capi.rsd(ctx, cloud, s["kp_off"], *tk, s["radius"] if radius is None else radius, full_histogram=full, want_counts=True)
        ctx.sync()
        return rows.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)
    finally:
        cloud.close()


def check_histogram(rows, cnt, a):
    assert rows.shape == a["row_lo"].shape and np.array_equal(cnt, a["cnt"])
    assert np.array_equal(np.isnan(rows), np.isnan(a["row_lo"]))
    v = a["valid"]
    decided = a["lo"] == a["hi"]
    assert np.array_equal(rows[v][decided[v]].view(np.uint32), a["row_lo"][v][decided[v]].view(np.uint32))
    for k, j in zip(*np.nonzero(~decided & v[:, None])):
        allowed = (np.arange(a["lo"][k, j], a["hi"][k, j] + 1).astype(F) / ref.NORM).astype(F)
        assert rows[k, j] in allowed, (k, j)
    assert not rows[a["cnt"] == 1].any()


def check_radii(rows, cnt, a):
    assert rows.shape == a["radii"].shape and np.array_equal(cnt, a["cnt"])
    assert np.isnan(rows[~a["valid"]]).all() and np.isfinite(rows[a["valid"]]).all()
    ok = a["valid"] & a["radii_ok"]
    want = a["radii"][ok]
    ulps = np.abs(rows[ok].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    assert (ulps <= 1.0).all(), ulps.max()
    assert not rows[a["cnt"] == 1].any() and (rows[ok][:, 0] <= rows[ok][:, 1]).all()
    return float(ulps.max()) if ok.any() else 0.0


@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_rsd_matches_the_restatement(pkg, gpu, name):
    """(a) generic, (b) the neighbour counts about one and two wavefronts, (c) the angle edges, (d) the distance edges, (e) the tiled
    neighbourhoods (at the native capacity here), (f) the hand-derived radii -- both modes"""
    s, a = scenes.scene(name), scenes.answer(name)
    rows, cnt = run_scene(pkg, gpu, s, True)
    check_histogram(rows, cnt, a)
    rad, cnt2 = run_scene(pkg, gpu, s, False)
    worst = check_radii(rad, cnt2, a)
    print("%s: %d keypoints, %d pairs, %d undecided; radii within %.2f ulp" % (name, len(cnt), a["pairs"].sum(), a["undecided"].sum(), worst))
    if name == "counts":
        assert cnt.tolist() == scenes.COUNTS and np.isnan(rows[0]).all() and np.isnan(rad[0]).all()
        assert not rows[1].any() and not rad[1].any()
    if name == "dist_edges":                                             # dist == R exactly: bin 4, as the definition says (deviation 4)
        assert rows[0].reshape(5, 5)[4].sum() == F(1) / ref.NORM and np.count_nonzero(rows[0]) == 1
        k = scenes.DIST_EDGE_KEYPOINTS.index("one ulp wider")
        assert not rows[k].any()
    if name == "radii":
        want = F(F(s["radius"]) * F(1.1))
        assert rad[0].tolist() == [want, want]


def test_not_finite_inputs(pkg, gpu):
    """a keypoint that is not finite, a ball that misses the grid: NaN rows, count 0; normals that are not finite: their pairs skipped"""
    P = np.asarray([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0], [0.02, 0.02, 0.02]], F)
    N = np.asarray([[1, 0, 0], [np.nan, 0, 0], [0, 1, 0], [0, np.inf, 0]], F)
    kp = np.asarray([[np.nan, 0, 0], [100, 0, 0], [0, 0, 0], [0, 0, np.inf]], F)
    s = dict(pt_off=np.array([0, 4], np.uint32), xyz=P, normals=N, kp_off=np.array([0, 4], np.uint32), kp=kp, radius=float(F(0.3)))
    a = ref.rsd(s["pt_off"], P, N, s["kp_off"], kp, s["radius"])
    assert a["cnt"].tolist() == [0, 0, 4, 0] and a["skipped"][2] == 5 and a["lo"][2].sum() == 1
    rows, cnt = run_scene(pkg, gpu, s, True)
    check_histogram(rows, cnt, a)
    rad, cnt = run_scene(pkg, gpu, s, False)
    check_radii(rad, cnt, a)
    assert np.isnan(rows[[0, 1, 3]]).all() and np.isnan(rad[[0, 1, 3]]).all()


@pytest.mark.parametrize("full", [True, False])
def test_tiled_path_gives_the_bytes_of_the_native_capacity(pkg, gpu, monkeypatch, full):
    """ISMHIP_RSD_CAP=64: 64 and 65 neighbours are the capacity and one more, 130 and 200 take three and four tiles; 520 takes three
    tiles natively. Same bytes either way, and those of the restatement."""
    s, a = scenes.scene("overflow"), scenes.answer("overflow")
    native, cnt = run_scene(pkg, gpu, s, full)
    for cap in ("64", "128", "100"):                                     # 100: rounded down to 64
        monkeypatch.setenv("ISMHIP_RSD_CAP", cap)
        rows, cnt2 = run_scene(pkg, gpu, s, full)
        monkeypatch.delenv("ISMHIP_RSD_CAP")
        assert np.array_equal(rows.view(np.uint32), native.view(np.uint32)) and np.array_equal(cnt, cnt2)
    (check_histogram if full else check_radii)(native, cnt, a)
    g = scenes.scene("generic")
    native, _ = run_scene(pkg, gpu, g, full)
    monkeypatch.setenv("ISMHIP_RSD_CAP", "64")
    rows, _ = run_scene(pkg, gpu, g, full)
    assert np.array_equal(rows.view(np.uint32), native.view(np.uint32))


@pytest.mark.parametrize("full", [True, False])
def test_same_bytes_twice_on_a_copy_and_on_two_cell_sizes(pkg, gpu, full):
    ctx, _ = gpu
    s = scenes.scene("generic")
    ctx.timers_enable(True); ctx.timers_reset()
    a, ca = run_scene(pkg, gpu, s, full)
    b, cb = run_scene(pkg, gpu, s, full)
    ctx.sync()
    t = ctx.timer("rsd")
    ctx.timers_enable(False)
    assert t[1] == 2 and t[0] > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ca, cb)
    c, cc = run_scene(pkg, gpu, s, full, cell_scale=0.23)               # other cells: the neighbours arrive in another order
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(ca, cc)
    # object 0 appended again as a fifth object, its points in reverse order
    e0, k0 = int(s["pt_off"][1]), int(s["kp_off"][1])
    two = dict(s)
    two["xyz"] = np.concatenate([s["xyz"], s["xyz"][:e0][::-1]]); two["normals"] = np.concatenate([s["normals"], s["normals"][:e0][::-1]])
    two["pt_off"] = np.concatenate([s["pt_off"], [s["pt_off"][-1] + e0]]).astype(np.uint32)
    two["kp"] = np.concatenate([s["kp"], s["kp"][:k0]]); two["kp_off"] = np.concatenate([s["kp_off"], [s["kp_off"][-1] + k0]]).astype(np.uint32)
    d, cd = run_scene(pkg, gpu, two, full)
    assert np.array_equal(d[:len(a)].view(np.uint32), a.view(np.uint32))
    assert np.array_equal(d[len(a):].view(np.uint32), a[:k0].view(np.uint32)) and np.array_equal(cd[len(a):], ca[:k0])


def test_refused_arguments(pkg, gpu):
    Err = pkg.capi.IsmHipError
    s = scenes.scene("radii")
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(Err, match=r"\(-1\).*rsd: bad argument"):
            run_scene(pkg, gpu, s, True, radius=radius)
    rows, cnt = run_scene(pkg, gpu, s, False)                            # and the call itself still works
    assert rows.shape == (len(cnt), 2) and cnt[0] == 50


def test_tiny_radius_takes_the_double_formulas(pkg, gpu):
    """R = 2^-63: (R / 5)^2 is no normal float, the guard bands cannot enclose their edges and every pair is decided in double. Cluster 0
    of the distance scene scaled by 2^-62 (exact): dist == R in bin 4, one ulp wider neglected, the coincident pair in bin 0. The three
    pair distances squared are 2^-126, its successor and 0: none of them is a subnormal number."""
    scale = F(2.0 ** -62)
    d = scenes.scene("dist_edges")
    s = dict(pt_off=np.array([0, 6], np.uint32), xyz=(d["xyz"][:6] * scale).astype(F), normals=d["normals"][:6],
             kp=(np.asarray([[0, 0, 0], [0, 3.0, 0], [0.1, 6.0, 0.05]], F) * scale).astype(F), kp_off=np.array([0, 3], np.uint32),
             radius=float(F(scenes.DIST_R) * scale))
    a = ref.rsd(s["pt_off"], s["xyz"], s["normals"], s["kp_off"], s["kp"], s["radius"])
    assert a["cnt"].tolist() == [2, 2, 2] and a["neglected"].tolist() == [0, 1, 0]
    rows, cnt = run_scene(pkg, gpu, s, True)
    check_histogram(rows, cnt, a)
    one = F(1) / ref.NORM
    assert rows[0].reshape(5, 5)[4].sum() == one and not rows[1].any() and rows[2].reshape(5, 5)[0].sum() == one


# ------------------------------------------------------------------------------------------------ codeword search on real rows
@pytest.fixture(scope="module")
def sphere_rows(pkg, gpu):
    """2500 rows in either mode on 3000 points of the unit sphere with disturbed normals: the first 2500 points as keypoints"""
    rng = np.random.default_rng(601)
    p = rng.normal(size=(3000, 3)); p /= np.linalg.norm(p, axis=1, keepdims=True)
    n = p + 0.35 * rng.normal(size=p.shape); n /= np.linalg.norm(n, axis=1, keepdims=True)
    s = dict(pt_off=np.array([0, 3000], np.uint32), xyz=p.astype(F), normals=n.astype(F), kp_off=np.array([0, 2500], np.uint32),
             kp=p[:2500].astype(F), radius=float(F(0.3)))
    out = {}
    for full in (True, False):
        rows, cnt = run_scene(pkg, gpu, s, full)
        assert rows.shape == (2500, 25 if full else 2) and np.isfinite(rows).all() and cnt.min() > 20
        out[full] = (rows[:2000].copy(), rows[2000:].copy())
    return out


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("metric", [0, 1])
def test_knn_on_rsd_rows(pkg, gpu, ora, sphere_rows, metric, full):
    """ismhip_knn at D = 25 and at D = 2 (the shortest row any descriptor gives), 2000 words and 500 queries with five exact hits,
    squared L2 and chi-square: bit-equal to ismref_knn"""
    ctx, dev = gpu
    words, q = sphere_rows[full]
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

"""SpinImage on the device (-m gpu): ismhip_keypoint_normals and ismhip_spin_image through capi on the scenes of spin_image_scenes.py
against the restatement spin_image_ref.py. Indices, axes, counts and the NaN and zero patterns are equal; finite rows agree within
TOL = 1e-7 absolute. test_spin_image_cpu.py proves on the host that no scene leaves a neighbour's fate to the last bit, so the device
and the restatement deposit the same neighbours at the same entries, and what is left is the fixed point:
  - a bin takes at most one deposit per neighbour, each round(v * 2^28) with an error <= 2^-29: |h_i - H_i| <= n 2^-29 for n deposited
    neighbours, and |S - sum H| <= 4 n 2^-29;
  - the four weights of a neighbour sum to 1, so sum H = n (but for the entries dropped outside the matrix, of rounding size): the
    quotient h_i / S differs from H_i / sum H by <= (1 + 4) 2^-29 / (1 - 2^-27) < 1e-8, for any n;
  - one float rounding of a value <= 1: <= 2^-25 = 3e-8; the restatement rounds once too: 6e-8 in all, 7e-8 with the above.
Then reproducibility and the timers, the refused widths, and the codeword search on real rows at D = 153."""
import numpy as np
import pytest

import spin_image_scenes as scenes
from test_gpu_parity import T, _cb

pytestmark = pytest.mark.gpu
TOL = 1e-7


def run_scene(pkg, gpu, s, w=None, radius=None):
    """-> (axes [K, 3], idx [K], rows [K, D], cnt [K]) of the device on the scene dict s (w, radius: instead of the scene's)"""
    ctx, dev = gpu
    capi = pkg.capi
    t = [T(s["xyz"][:, i], dev) for i in range(3)] + [T(s["normals"][:, i], dev) for i in range(3)]
    tk = [T(s["kp"][:, i], dev) for i in range(3)]
    cloud = capi.Cloud(ctx, s["pt_off"], *t, 0.4 * s["radius"])
    try:
        ax, ay, az, idx = capi.keypoint_normals(ctx, cloud, s["kp_off"], *tk, want_index=True)
        rows, cnt = capi.spin_image(ctx, cloud, s["kp_off"], *tk, ax, ay, az, s["radius"] if radius is None else radius,
                                    s["w"] if w is None else w, want_counts=True)
        ctx.sync()
        axes = np.stack([ax.cpu().numpy(), ay.cpu().numpy(), az.cpu().numpy()], 1)
        return axes, idx.cpu().numpy(), rows.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)
    finally:
        cloud.close()


def check_rows(axes, idx, rows, cnt, a):
    """device indices, axes, counts and rows against the restatement's answer a: indices, axes (bits), counts, NaN and zero patterns equal,
    finite values within TOL -> the largest deviation"""
    assert np.array_equal(idx, a["idx"])
    assert np.array_equal(axes.view(np.uint32), a["axes"].view(np.uint32))
    assert np.array_equal(cnt, a["cnt"])
    assert rows.shape == a["rows"].shape
    assert np.array_equal(np.isnan(rows), np.isnan(a["rows"]))
    assert np.array_equal(rows == 0, a["rows"] == 0)
    fin = ~np.isnan(a["rows"])
    dev = float(np.abs(rows[fin].astype(np.float64) - a["rows"][fin].astype(np.float64)).max()) if fin.any() else 0.0
    assert dev <= TOL, dev
    return dev


@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_spin_image_matches_the_restatement(pkg, gpu, name):
    """(a) sphere, (b) the hand case, (c) keypoints off the cloud, (d) coincident points, (e) scaled axes, (f) counts and special rows,
    (g) the cylinder limit, (h) 4000 same-address deposits, (i) 20 000 neighbours through the queue, (j) widths 1 and 25, (k) a batch"""
    s, a = scenes.scene(name), scenes.answer(name)
    axes, idx, rows, cnt = run_scene(pkg, gpu, s)
    dev = check_rows(axes, idx, rows, cnt, a)
    print("%s: %d rows, %d neighbours, largest deviation %.3e" % (name, len(rows), cnt.sum(), dev))
    if name == "counts":
        assert cnt.tolist() == [0, 0, 1, 3, 0, 0] and not rows[:3].any() and np.isnan(rows[3:]).all()
    if name == "ring":
        img = rows[0].reshape(9, 17)
        assert all(abs(img[e] - 0.25) <= 1e-6 for e in scenes.RING_ENTRIES) and np.count_nonzero(img) == 4


def test_two_calls_give_the_same_bits_and_the_timers_count(pkg, gpu):
    ctx, _ = gpu
    ctx.timers_enable(True); ctx.timers_reset()
    a = run_scene(pkg, gpu, scenes.scene("batch"))
    b = run_scene(pkg, gpu, scenes.scene("batch"))
    ctx.sync()
    t_desc, t_norm = ctx.timer("spin_image"), ctx.timer("keypoint_normals")
    ctx.timers_enable(False)
    assert t_desc[1] == 2 and t_desc[0] > 0 and t_norm[1] == 2 and t_norm[0] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    c = run_scene(pkg, gpu, scenes.scene("long_queue"))
    d = run_scene(pkg, gpu, scenes.scene("long_queue"))
    assert np.array_equal(c[2].view(np.uint32), d[2].view(np.uint32))


def test_refused_widths_and_arguments(pkg, gpu):
    """image_width 0: ISMHIP_ERR_INVALID (-1); 26, whose 1431 floats ismhip_knn would not take: ISMHIP_ERR_UNSUPPORTED (-4)"""
    Err = pkg.capi.IsmHipError
    s = scenes.scene("hand3")
    with pytest.raises(Err, match=r"\(-1\).*spin_image: bad argument"):
        run_scene(pkg, gpu, s, w=0)
    with pytest.raises(Err, match=r"\(-4\).*spin_image: image width above 25"):
        run_scene(pkg, gpu, s, w=26)
    for radius in (0.0, -1.0, float("nan")):
        with pytest.raises(Err, match=r"\(-1\).*spin_image: bad argument"):
            run_scene(pkg, gpu, s, radius=radius)
    axes, idx, rows, cnt = run_scene(pkg, gpu, s)                        # and the call itself still works
    assert rows.shape == (1, 153) and cnt.tolist() == [3]


# ------------------------------------------------------------------------------------------------ codeword search on real rows
@pytest.fixture(scope="module")
def sphere_rows(pkg, gpu):
    """2500 rows on scene (a)'s cloud: its first 2500 points as keypoints"""
    s = dict(scenes.scene("sphere"))
    s["kp"] = s["xyz"][:2500].copy(); s["kp_off"] = np.array([0, 2500], np.uint32)
    rows = run_scene(pkg, gpu, s)[2]
    assert rows.shape == (2500, 153) and np.isfinite(rows).all()
    return rows[:2000].copy(), rows[2000:].copy()


@pytest.mark.parametrize("metric", [0, 1])
def test_knn_on_spin_image_rows(pkg, gpu, ora, sphere_rows, metric):
    """ismhip_knn at D = 153 (no multiple of 4), 2000 words and 500 queries with five exact hits: bit-equal to ismref_knn"""
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

"""USC on the device (-m gpu): ismhip_point_density, ismhip_usc_tables and ismhip_usc through capi on the scenes of usc_scenes.py against
the restatement usc_ref.py, run on the DEVICE's own frames. The density equals brute-force numpy; the tables are libm against numpy;
on every keypoint the restatement decides q_out is equal in all 1960 bins, on the others it lies inside [q_lo, q_hi]; desc_out is bit
for bit (float)(Q * 2^-32 * lut) of the device's own q_out and table; NaN pattern and counts are equal. Then byte equality across two calls
and two grid cell sizes, the two row filters, and the refusals. test_usc_cpu.py proves on the host that at most one finite keypoint in
ten of a scene is undecided."""
import numpy as np
import pytest

import usc_ref as ref
import usc_scenes as scenes
from test_gpu_parity import T

pytestmark = pytest.mark.gpu
F = np.float32


def run_scene(pkg, gpu, s, cell_scale=0.4):
    """-> dict(dens [n_pts], lrf [K, 9], rows [K, 1960], cnt [K], q [K, 1960]) of the device on the scene dict s"""
    ctx, dev = gpu
    capi = pkg.capi
    nrm = np.zeros_like(s["xyz"]); nrm[:, 2] = 1
    t = [T(s["xyz"][:, i], dev) for i in range(3)] + [T(nrm[:, i], dev) for i in range(3)]
    tk = [T(s["kp"][:, i], dev) for i in range(3)]
    cloud = capi.Cloud(ctx, s["pt_off"], *t, cell_scale * min(s["radius"], s["frame_radius"]))
    try:
        dens = capi.point_density(ctx, cloud, s["density_radius"])
        lrf = capi.shot_lrf(ctx, cloud, s["kp_off"], *tk, s["frame_radius"]) if s["lrf"] is None else T(s["lrf"], dev)
        rows, cnt, q = capi.usc(ctx, cloud, s["kp_off"], *tk, lrf, s["radius"], s["min_radius"], dens, want_counts=True, want_q=True)
        ctx.sync()
        return dict(dens=dens.cpu().numpy().astype(np.int64), lrf=lrf.cpu().numpy(), rows=rows.cpu().numpy(), cnt=cnt.cpu().numpy().astype(np.int64),
                    q=q.cpu().numpy(), t=(lrf, tk, rows))
    finally:
        cloud.close()


@pytest.fixture(scope="module")
def results(pkg, gpu):
    """every scene once, shared by the tests below"""
    return {name: run_scene(pkg, gpu, scenes.scene(name)) for name in scenes.NAMES}


@pytest.mark.parametrize("name", scenes.NAMES)
def test_point_density_is_brute_force(results, name):
    s = scenes.scene(name)
    want = ref.density(s["pt_off"], s["xyz"], s["density_radius"])
    assert np.array_equal(results[name]["dens"], want)


def test_tables(pkg):
    for R, rmin in ((0.4, 0.04), (0.3, 0.03), (0.25, 0.025), (1.0, 0.1)):
        lut, e32 = pkg.capi.usc_tables(R, rmin)
        want, _, we32 = ref.tables(R, rmin)
        assert np.array_equal(e32, we32)
        err = np.abs(lut - want) / np.spacing(want)
        print(f"R {R}: lut within {err.max():.2f} double ulps of numpy")
        assert err.max() <= 4


@pytest.mark.parametrize("name", scenes.NAMES)
def test_usc_matches_the_restatement(pkg, results, name):
    s, out = scenes.scene(name), results[name]
    K = len(s["kp"])
    assert out["rows"].shape == (K, ref.DIM) and out["q"].shape == (K, ref.DIM)
    d = ref.describe(s["pt_off"], s["xyz"], s["kp_off"], s["kp"], out["lrf"], s["radius"], s["min_radius"], out["dens"])
    rows, q = out["rows"], out["q"]
    nan = np.isnan(rows[:, 0])
    # whole-row NaN contract, never an infinity; the NaN pattern and the neighbour counts are the restatement's
    assert np.array_equal(np.isnan(rows), np.broadcast_to(nan[:, None], rows.shape)) and not np.isinf(rows).any()
    assert np.array_equal(nan, d["nan_row"]) and np.array_equal(out["cnt"], d["count"]) and not q[nan].any()
    ok = ~nan
    dec = ok & d["decided"]
    print(f"{name}: {int(ok.sum())} finite keypoints, {int((ok & ~d['decided']).sum())} undecided")
    assert np.array_equal(q[dec], d["q_lo"][dec])                                      # all 1960 bins
    und = ok & ~d["decided"]
    assert (q[und] >= d["q_lo"][und]).all() and (q[und] <= d["q_hi"][und]).all()
    # every point of the ball that is not skipped is deposited exactly once
    for k in np.nonzero(ok)[0]:
        assert int(q[k].sum()) == int(d["q_hi"][k].sum()) if d["decided"][k] else int(q[k].sum()) >= int(d["q_lo"][k].sum())
    # the row from the device's own integers and the device's own table
    lut, _ = pkg.capi.usc_tables(s["radius"], s["min_radius"])
    want = ref.row_from_q(q[ok], lut)
    assert np.array_equal(rows[ok].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", scenes.NAMES)
def test_two_calls_and_two_cell_sizes_give_the_same_bits(pkg, gpu, results, name):
    s, a = scenes.scene(name), results[name]
    for cell_scale in (0.4, 1.1):
        b = run_scene(pkg, gpu, s, cell_scale)
        assert np.array_equal(a["dens"], b["dens"]) and np.array_equal(a["cnt"], b["cnt"]) and np.array_equal(a["q"], b["q"])
        if s["lrf"] is not None:                                                       # (computed frames are the LRF tests' subject)
            assert np.array_equal(a["rows"].view(np.uint32), b["rows"].view(np.uint32))
        else:
            same = np.array_equal(a["lrf"].view(np.uint32), b["lrf"].view(np.uint32))
            assert not same or np.array_equal(a["rows"].view(np.uint32), b["rows"].view(np.uint32))


@pytest.mark.parametrize("name", ("off", "ragged"))
def test_both_row_filters_keep_the_same_rows(pkg, gpu, results, name):
    """k_keep_rows (one element per row) and k_keep (every element) on rows that are NaN throughout or not at all"""
    ctx, _ = gpu
    s = scenes.scene(name)
    lrf, tk, rows = results[name]["t"]
    a = pkg.capi.compact_descriptor_rows(ctx, s["kp_off"], rows, lrf, *tk)
    b = pkg.capi.compact_features(ctx, s["kp_off"], rows, lrf, *tk)
    ctx.sync()
    assert np.array_equal(np.asarray(a[0]), np.asarray(b[0]))
    assert np.array_equal(a[6].cpu().numpy(), b[6].cpu().numpy())
    assert np.array_equal(a[1].cpu().numpy().view(np.uint32), b[1].cpu().numpy().view(np.uint32))
    keep = ~np.isnan(results[name]["rows"][:, 0])              # (a NaN frame gives a NaN row: the frames drop nothing more)
    assert np.array_equal(a[6].cpu().numpy(), np.nonzero(keep)[0])


def test_refusals(pkg, gpu):
    ctx, dev = gpu
    capi = pkg.capi
    s = scenes.scene("patch")
    nrm = np.zeros_like(s["xyz"]); nrm[:, 2] = 1
    t = [T(s["xyz"][:, i], dev) for i in range(3)] + [T(nrm[:, i], dev) for i in range(3)]
    tk = [T(s["kp"][:, i], dev) for i in range(3)]
    cloud = capi.Cloud(ctx, s["pt_off"], *t, 0.1)
    try:
        lrf = capi.shot_lrf(ctx, cloud, s["kp_off"], *tk, 0.2)
        dens = capi.point_density(ctx, cloud, 0.1)
        for R, rmin in ((0.0, 0.01), (-1.0, 0.01), (float("inf"), 0.01), (float("nan"), 0.01), (0.3, 0.0), (0.3, 0.3), (0.3, 0.5), (0.3, float("nan"))):
            with pytest.raises(capi.IsmHipError, match=r"\(-1\).*usc: bad argument"):
                capi.usc(ctx, cloud, s["kp_off"], *tk, lrf, R, rmin, dens)
        with pytest.raises(capi.IsmHipError, match=r"\(-1\).*usc: bad argument"):
            capi.usc(ctx, cloud, s["kp_off"], *tk, lrf, 0.3, 0.03, None)
        for r in (0.0, -0.1, float("inf"), float("nan")):
            with pytest.raises(capi.IsmHipError, match=r"\(-1\).*point_density: bad argument"):
                capi.point_density(ctx, cloud, r)
        rows = capi.usc(ctx, cloud, s["kp_off"], *tk, lrf, 0.3, 0.03, dens)          # the context stays usable
        ctx.sync()
        assert np.isfinite(rows.cpu().numpy()).all()
    finally:
        cloud.close()

"""The raw CGF histogram on the MI355X (ismhip_keypoint_normals_pca, ismhip_cgf_raw) against the restatement tests/cgf_ref.py.

The restatement reads the DEVICE's frames and keypoint normals (as test_gpu_rift.py feeds the device's gradients to its restatement) and
repeats every float32 step of the kernel with the same operations, so a decided row is held BIT-equal: the same counts over the same sum.
At most 5 % of a scene's keypoints may be undecided. The keypoint normals themselves are held to the float64 PCA of cgf_ref.pca_normal
within 1e-5 scaled by the eigenvalue gap (the direction of a smallest eigenvector is only as stable as its gap is wide)."""
import numpy as np
import pytest

import cgf_ref as ref
import cgf_scenes as scenes

pytestmark = pytest.mark.gpu
F = np.float32


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _run(pkg, ctx, dev, s, cell_scale):
    """-> dict(lrf, normals [nkp, 3], rows, count) as numpy, by the calls of capi.cgf taken apart"""
    R, rmin, rl = pkg.capi.cgf_radii(s["radius"])
    x, y, z = (_dev(s["xyz"][:, i], dev) for i in range(3))
    zero = _dev(np.zeros(len(s["xyz"]), F), dev)
    kx, ky, kz = (_dev(s["kp"][:, i], dev) for i in range(3))
    cloud = pkg.capi.Cloud(ctx, s["pt_off"], x, y, z, zero, zero, zero, cell_scale * R)
    lrf = pkg.capi.shot_lrf(ctx, cloud, s["kp_off"], kx, ky, kz, rl)
    n = pkg.capi.keypoint_normals_pca(ctx, cloud, s["kp_off"], kx, ky, kz, 0.1 * R)
    rows, cnt = pkg.capi.cgf_raw(ctx, cloud, s["kp_off"], kx, ky, kz, lrf, *n, R, rmin, want_counts=True)
    ctx.sync()
    out = dict(lrf=lrf.cpu().numpy().reshape(-1, 9), normals=np.stack([t.cpu().numpy() for t in n], 1), rows=rows.cpu().numpy(), count=cnt.cpu().numpy())
    cloud.close()
    return out


@pytest.fixture(scope="module")
def runs(pkg, gpu):
    """every scene at two cell sizes, run once, with the restatement's answer on the first run's frames and normals"""
    ctx, dev = gpu
    out = {}
    for k in range(scenes.N_SCENES):
        s = scenes.scene(k)
        a, b = _run(pkg, ctx, dev, s, 0.4), _run(pkg, ctx, dev, s, 0.15)
        out[k] = (s, a, b, scenes.answer(s, a["lrf"], a["normals"]))
    return out


def check_raw_rows(got, want):
    """device raw rows and counts (dict rows, count) against cgf_ref.raw's answer: counts equal and rows bit-equal on every decided keypoint
    -> the decided mask"""
    dec = ~want["undecided"]
    assert np.array_equal(got["count"][dec], want["sum"][dec])
    bad = [i for i in np.flatnonzero(dec) if not np.array_equal(got["rows"][i].view(np.uint32), want["rows"][i].view(np.uint32))]
    for i in bad[:5]:
        d = np.flatnonzero(got["rows"][i] != want["rows"][i])
        print("keypoint %d (ball %d): bins %s device %s restatement %s" % (i, want["ball"][i], d[:6], got["rows"][i][d[:6]], want["rows"][i][d[:6]]))
    assert not bad
    return dec


@pytest.mark.parametrize("k", range(scenes.N_SCENES))
def test_rows_are_bit_equal_to_the_restatement(runs, k):
    s, got, _, want = runs[k]
    dec = ~want["undecided"]
    print("scene %d: %d keypoints, %d undecided; frames %s" % (k, len(dec), (~dec).sum(), {kd: want["kind"].count(kd) for kd in set(want["kind"])}))
    assert (~dec).sum() <= scenes.MAX_UNDECIDED * len(dec)
    check_raw_rows(got, want)
    assert np.isfinite(got["rows"]).all()                                     # an empty ball is a row of zeros, never NaN
    assert not got["rows"][want["sum"] == 0].any()


def test_scene_zero_holds_its_cases_on_the_device(runs):
    s, got, _, want = runs[0]
    kinds = want["kind"]
    assert {"identity", "flipped", "kept"} <= set(kinds)
    for n in (0, 1, 2, 63, 64, 65):
        assert n in want["ball"].tolist()
    assert want["ball"].max() >= 250
    a, _ = scenes.object_of(s, "edges")                                       # fewer than 5 frame neighbours: the device's frame is NaN
    assert np.isnan(got["lrf"][a]).all() and kinds[a] == "identity" and not want["undecided"][a]
    hand = np.zeros(ref.DIM, np.int64)
    for _p, bins in scenes.EDGE_POINTS[1:]:
        hand[ref.index(*bins)] += 1
    assert np.array_equal(got["rows"][a], (hand / float(hand.sum())).astype(F))   # the bins worked out by hand
    for name, total in (("empty ball", 0), ("one point", 0), ("two points", 1), ("coincident", 1), ("duplicate nearest", 2)):
        a, _ = scenes.object_of(s, name)
        assert got["count"][a] == total, name
    a, _ = scenes.object_of(s, "ball 64")                                     # a valid frame, fewer than 3 points in the normal ball: no flip
    assert np.isfinite(got["lrf"][a]).all() and np.isnan(got["normals"][a]).all() and kinds[a] == "kept"
    a, b = scenes.object_of(s, "patch above the origin")
    assert set(kinds[a:b]) == {"flipped"}
    a, b = scenes.object_of(s, "patch below the origin")
    assert set(kinds[a:b]) == {"kept"}


@pytest.mark.parametrize("k", range(scenes.N_SCENES))
def test_two_cell_sizes_and_two_runs_give_the_same_bytes(pkg, gpu, runs, k):
    ctx, dev = gpu
    s, a, b, _ = runs[k]
    again = _run(pkg, ctx, dev, s, 0.4)
    assert np.array_equal(a["rows"].view(np.uint32), again["rows"].view(np.uint32)) and np.array_equal(a["count"], again["count"])
    # the frames and normals of the other cell size differ in the last bits (float sums in another order): rows are compared where they agree
    same = (a["lrf"].view(np.uint32) == b["lrf"].view(np.uint32)).all(1) & (a["normals"].view(np.uint32) == b["normals"].view(np.uint32)).all(1)
    print("scene %d: %d of %d keypoints with the same frame and normal bits at both cell sizes" % (k, same.sum(), len(same)))
    assert np.array_equal(a["rows"][same].view(np.uint32), b["rows"][same].view(np.uint32)) and np.array_equal(a["count"][same], b["count"][same])


def test_same_frames_any_cell_size_same_bytes(pkg, gpu):
    """ismhip_cgf_raw alone, fed the SAME frames and normals at two cell sizes: every row has the same bytes"""
    ctx, dev = gpu
    s = scenes.scene(1)
    R, rmin, rl = pkg.capi.cgf_radii(s["radius"])
    x, y, z = (_dev(s["xyz"][:, i], dev) for i in range(3))
    zero = _dev(np.zeros(len(s["xyz"]), F), dev)
    kx, ky, kz = (_dev(s["kp"][:, i], dev) for i in range(3))
    rows = []
    lrf = n = None
    for cell in (0.4 * R, 0.11 * R, 1.3 * R):
        cloud = pkg.capi.Cloud(ctx, s["pt_off"], x, y, z, zero, zero, zero, cell)
        if lrf is None:
            lrf = pkg.capi.shot_lrf(ctx, cloud, s["kp_off"], kx, ky, kz, rl)
            n = pkg.capi.keypoint_normals_pca(ctx, cloud, s["kp_off"], kx, ky, kz, 0.1 * R)
        rows.append(pkg.capi.cgf_raw(ctx, cloud, s["kp_off"], kx, ky, kz, lrf, *n, R, rmin).cpu().numpy())
        cloud.close()
    assert np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32)) and np.array_equal(rows[0].view(np.uint32), rows[2].view(np.uint32))


def check_keypoint_normals(normals, want, cnt, gap):
    """device PCA keypoint normals against cgf_ref.pca_normal: NaN below three points, else within 1e-5 / gap + 2^-23, unit length
    -> (compared mask, errors, tolerances)"""
    assert np.array_equal(np.isnan(normals).any(1), cnt < 3)
    ok = (cnt >= 3) & (gap > 1e-6)
    err = np.abs(normals[ok].astype(np.float64) - want[ok]).max(1)
    tol = 1e-5 / np.minimum(gap[ok], 1.0) + 2.0 ** -23
    assert (err <= tol).all()
    assert np.allclose(np.linalg.norm(normals[cnt >= 3], axis=1), 1.0, atol=1e-6)
    return ok, err, tol


@pytest.mark.parametrize("k", range(scenes.N_SCENES))
def test_keypoint_normals_against_the_float64_pca(runs, k):
    s, got, _, _ = runs[k]
    want, cnt, gap = scenes.keypoint_normals(s)
    ok, err, tol = check_keypoint_normals(got["normals"], want, cnt, gap)
    print("scene %d: %d normals, largest error %.3g (%.3g of its tolerance)" % (k, ok.sum(), err.max() if ok.any() else 0.0, (err / tol).max() if ok.any() else 0.0))
    assert k != 0 or ok.sum() >= 20                                           # scene 0: the keypoints of both patches


def test_refusals(pkg, gpu):
    ctx, dev = gpu
    s = scenes.scene(1)
    R, rmin, rl = pkg.capi.cgf_radii(s["radius"])
    x, y, z = (_dev(s["xyz"][:, i], dev) for i in range(3))
    kx, ky, kz = (_dev(s["kp"][:, i], dev) for i in range(3))
    cloud = pkg.capi.Cloud(ctx, s["pt_off"], x, y, z, x, y, z, 0.4 * R)
    lrf = pkg.capi.shot_lrf(ctx, cloud, s["kp_off"], kx, ky, kz, rl)
    n = pkg.capi.keypoint_normals_pca(ctx, cloud, s["kp_off"], kx, ky, kz, 0.1 * R)
    for bad_r, bad_rmin in ((0.0, rmin), (R, R), (R, 0.0), (float("nan"), rmin), (float("inf"), rmin)):
        with pytest.raises(pkg.capi.IsmHipError, match="cgf_raw: bad argument"):
            pkg.capi.cgf_raw(ctx, cloud, s["kp_off"], kx, ky, kz, lrf, *n, bad_r, bad_rmin)
    with pytest.raises(pkg.capi.IsmHipError, match="keypoint_normals_pca: bad argument"):
        pkg.capi.keypoint_normals_pca(ctx, cloud, s["kp_off"], kx, ky, kz, 0.0)
    with pytest.raises(pkg.capi.IsmHipError, match="offsets not monotone"):
        pkg.capi.cgf_raw(ctx, cloud, np.uint32([0, 5, 3]), kx, ky, kz, lrf, *n, R, rmin)
    nan_kp = _dev(np.full(len(s["kp"]), np.nan, F), dev)                       # a keypoint that is no point: the whole row NaN
    rows, cnt = pkg.capi.cgf_raw(ctx, cloud, s["kp_off"], nan_kp, ky, kz, lrf, *n, R, rmin, want_counts=True)
    assert np.isnan(rows.cpu().numpy()).all() and not cnt.cpu().numpy().any()
    cloud.close()

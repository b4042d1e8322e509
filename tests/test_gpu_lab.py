"""The device's CIELab conversion (-m gpu), observed directly through the diagnostic entry ismhip_rgb2lab: rgb2lab / rgb2lab_norm of
common.h on the context's LUTs, over the WHOLE 24-bit colour cube in one launch (64 MiB in, 192 MiB out).

 * bit for bit the oracle's batch: both are float32, the same operations in the same order, contraction off, LUTs made by the same host
   powf. Any difference is a finding.
 * the float64 restatement lab_ref.py's rule (within the derived bound where decided, on one candidate entry elsewhere), which
   test_lab_cpu.py holds the oracle to.
 * the cloud path (rgba_to_lab4 of grid.hip, which fills the cloud's Lab array in either grid build) agrees with it bit for bit: in a
   neighbourhood whose every point has the keypoint's colour, CSHOT's colour distance is |L - L'| + ... = 0 exactly iff the cloud's Lab
   of that colour equals rgb2lab_norm's in all three channels, and then every colour bin but step 0 receives exactly 0; one ulp of
   difference in any channel is a colour distance >= 1e-9 and a deposit of >= 2^-28 into bin 1 or 29. Checked on 6144 colours (the cube's
   corners, a 16^3 lattice, 2048 colours lab_ref calls undecided) on both grid builds, whose rows are also compared with each other.

Measured on the MI355X: no colour of the cube differs from the oracle, raw or normalised; largest |device - lab_ref| / bound 0.46 / 0.51 /
0.51 (L, a, b); 105 888 colours (0.63 %) on a candidate entry; no colour of the 6144 differs between the cloud and the probe on either
build, and the two builds' rows are the same bytes."""
import numpy as np
import pytest

import lab_ref
import shot_ref_scenes as srs
import test_gpu_frontend as gf

pytestmark = pytest.mark.gpu
CHUNK = 1 << 20


@pytest.mark.parametrize("normalised", [False, True], ids=["raw", "normalised"])
def test_whole_cube_equals_the_oracle_and_obeys_the_float64_rule(pkg, gpu, ora, normalised):
    import torch
    ctx, dev = gpu
    cube = torch.arange(1 << 24, dtype=torch.int32, device=dev)
    got = pkg.capi.rgb2lab(ctx, cube, normalised).cpu().numpy()
    ctx.sync()
    want = ora.rgb2lab_n(np.arange(1 << 24, dtype=np.uint32), normalised)
    differ = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert len(differ) == 0, (len(differ), [hex(int(c)) for c in differ[:8]], got[differ[:8]], want[differ[:8]])
    worst, und = np.zeros(3), 0
    for base in range(0, 1 << 24, CHUNK):
        lab = lab_ref.convert(np.arange(base, base + CHUNK, dtype=np.uint32))
        und += int((~lab.decided).sum())
        worst = np.maximum(worst, lab_ref.excess(got[base:base + CHUNK], lab, normalised).max(0))
    print("cube (%s): device == oracle on all 2^24 colours; largest |device - lab_ref| / bound %s, %d undecided colours on a candidate"
          % ("normalised" if normalised else "raw", worst, und))
    assert (worst <= 1).all()


def test_probe_ignores_bits_24_to_31_and_refuses_bad_arguments(pkg, gpu):
    import torch
    ctx, dev = gpu
    rng = np.random.default_rng(8)
    c = rng.integers(0, 1 << 24, size=1000).astype(np.int64)
    hi = c | (rng.integers(1, 256, size=1000).astype(np.int64) << 24)
    a = pkg.capi.rgb2lab(ctx, torch.as_tensor(c, dtype=torch.int32, device=dev))
    b = pkg.capi.rgb2lab(ctx, torch.as_tensor(hi.astype(np.uint32).astype(np.int32), device=dev))
    assert torch.equal(a, b) and a.shape == (1000, 3)
    assert pkg.capi.rgb2lab(ctx, torch.empty((0,), dtype=torch.int32, device=dev)).shape == (0, 3)
    with pytest.raises(pkg.capi.IsmHipError, match="rgb2lab: bad argument"):
        ctx.check(pkg.capi.lib().ismhip_rgb2lab(ctx._h, 5, None, 0, None), "ismhip_rgb2lab")


# ---------------------------------------------------------------------------------------------- the cloud path
CLUSTER_RADIUS = 0.3
LATTICE = 19                   # 19^3 = 6859 cluster sites, one unit apart


def uniform_clusters():
    """6144 clusters of 5 points within 0.2 of their keypoint, one unit apart; all five points of a cluster and its keypoint share one
    colour: the 4096 colours of srs.palette_pool() (corners, edges, a 16^3 lattice of the cube) and 2048 UNDECIDED colours"""
    rng = np.random.default_rng(9)
    c = rng.integers(0, 1 << 24, size=1 << 19).astype(np.uint32)
    und = c[~lab_ref.convert(c).decided][:2048]
    assert len(und) == 2048
    colours = np.concatenate([srs.palette_pool(), und]).astype(np.uint32)
    site = np.stack(np.unravel_index(np.arange(len(colours)), (LATTICE,) * 3), -1).astype(np.float64)
    d = rng.normal(size=(len(colours), 5, 3))
    d = d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(0.05, 0.2, size=(len(colours), 5, 1))
    p = (site[:, None, :] + d).reshape(-1, 3).astype(np.float32)
    n = rng.normal(size=p.shape); n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return p, n, np.repeat(colours, 5), site.astype(np.float32), colours


def run_cshot(pkg, ctx, dev, points, normals, rgba, kp, kp_rgba, frames, radius, cell):
    s = gf.Batch(pkg, ctx, dev, [(points, normals)], [kp], cell, [rgba], [kp_rgba])
    try:
        rows, cnt = pkg.capi.cshot1344(ctx, s.cloud, s.kp_off, *s.tk, s.t_kp_rgba, gf.T(frames, dev), radius, want_counts=True)
        rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
        ctx.sync()
    finally:
        s.close()
    return rows, cnt


_build_rows = {}


def rows_on_build(pkg, dev, monkeypatch, build):
    """CSHOT rows of the uniform clusters and of the sphere scene (identity frames) on a context of the given grid build, computed once"""
    if build not in _build_rows:
        if build == "fused":
            monkeypatch.delenv("ISMHIP_GRID_FUSED", raising=False)
        else:
            monkeypatch.setenv("ISMHIP_GRID_FUSED", "0")
        ctx = pkg.capi.Ctx(0)                                        # the switch is read when a context is created
        try:
            p, n, rgba, kp, colours = uniform_clusters()
            rows, cnt = run_cshot(pkg, ctx, dev, p, n, rgba, kp, colours, np.tile(srs.IDENTITY, (len(kp), 1)), CLUSTER_RADIUS, 0.5)
            s = srs.scene("sphere")
            sphere_rows, _ = run_cshot(pkg, ctx, dev, s.points, s.normals, s.rgba, s.keypoints, s.kp_rgba, np.tile(srs.IDENTITY, (24, 1)), s.radius, s.cell)
        finally:
            ctx.close()
        _build_rows[build] = (rows, cnt, colours, sphere_rows)
    return _build_rows[build]


@pytest.mark.parametrize("build", ["fused", "five-kernel"])
def test_cloud_path_agrees_with_the_probe_bit_for_bit(pkg, gpu, build, monkeypatch):
    rows, cnt, colours, _ = rows_on_build(pkg, gpu[1], monkeypatch, build)
    assert (cnt == 5).all() and np.isfinite(rows).all()
    col = rows[:, 352:].reshape(len(rows), 32, 31)
    bad = np.nonzero((col[:, :, 1:] != 0).any((1, 2)))[0]
    assert len(bad) == 0, [hex(int(c)) for c in colours[bad][:16]]   # the cloud's Lab of these colours is not rgb2lab_norm's
    assert (col[:, :, 0].sum(1) > 0.5).all()                          # ... and the colour weight really is in step 0


def test_both_grid_builds_give_identical_cshot_rows(pkg, gpu, monkeypatch):
    a, b = (rows_on_build(pkg, gpu[1], monkeypatch, build) for build in ("fused", "five-kernel"))
    assert a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert np.isfinite(a[3][:21]).all() and np.isnan(a[3][21:]).all()

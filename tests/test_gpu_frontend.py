"""GPU parity of the descriptor front end (-m gpu) on the scenes of frontend_scenes.py: dense balls (several row batches and
candidate windows of ball_for_each, one row longer than a window), a wide batch (XCD block map with padding blocks, objects far
from the origin, both grid builds), LRF sign ties at every key store of k_lrf_tie, neighbour counts around the queue sizes, and
inputs that sit EXACTLY on the hard decisions of SHOT and on the bin edges of FPFH. test_frontend_cpu.py proves on the host that
each scene reaches its path. Tolerances are the project's: frames 1e-5, SHOT / CSHOT 1e-4 with exact counts, FPFH 1e-2 on its
0..100 scale with exact counts, PCA normals 2e-3; NaN patterns exact."""
import numpy as np
import pytest

import frontend_scenes as fs

pytestmark = pytest.mark.gpu
TOL = 1e-4
LRF_TOL = 1e-5
FPFH_TOL = 1e-2


def T(a, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


class Batch:
    """a ragged batch on the device: SoA tensors, keypoints, a Cloud"""

    def __init__(self, pkg, ctx, dev, objs, kps, cell, rgba=None, kp_rgba=None):
        import torch
        self.ctx, self.dev = ctx, dev
        self.pt_off, self.p, self.n, self.kp_off, self.kp = fs.soa(objs, kps)
        self.rgba = None if rgba is None else np.concatenate(rgba).astype(np.uint32)
        self.kp_rgba = None if kp_rgba is None else np.concatenate(kp_rgba).astype(np.uint32)
        self.t = [T(c, dev) for c in fs.cols(self.p)] + [T(c, dev) for c in fs.cols(self.n)]
        self.tk = [T(c, dev) for c in fs.cols(self.kp)]
        self.t_rgba = None if rgba is None else T(self.rgba.astype(np.int64), dev, torch.int32)
        self.t_kp_rgba = None if kp_rgba is None else T(self.kp_rgba.astype(np.int64), dev, torch.int32)
        self.cloud = pkg.capi.Cloud(ctx, self.pt_off, *self.t, cell, rgba=self.t_rgba)

    def keypoints(self, kps):
        """another keypoint set on the same cloud -> (kp_off, numpy keypoints, device columns)"""
        off = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.uint32)
        kp = np.concatenate([np.asarray(k, np.float32).reshape(-1, 3) for k in kps])
        return off, kp, [T(c, self.dev) for c in fs.cols(kp)]

    def close(self):
        self.cloud.close()


def assert_close_nan(a, b, atol):
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"NaN pattern differs: {na.sum()} vs {nb.sum()}"
    if (~na).any():
        err = np.abs(a[~na] - b[~nb]).max()
        assert err <= atol, err


# ------------------------------------------------------------------------------------------------ dense and wide
# scene key -> (builder, cell, LRF / SHOT radius, FPFH radius); scenes, oracle results and default-context outputs are computed once
WIDE_FUSED, WIDE_FIVE, THIN = "wide-fused", "wide-five-kernel", "thin"
SCENES = {WIDE_FUSED: (lambda: fs.wide_batch(fs.FUSED_SURFACE), fs.DENSE_CELL, fs.DENSE_RADIUS, fs.FPFH_RADIUS),
          WIDE_FIVE: (lambda: fs.wide_batch(fs.WIDE_SURFACE), fs.DENSE_CELL, fs.DENSE_RADIUS, fs.FPFH_RADIUS),
          THIN: (fs.thin_batch, fs.THIN_CELL, fs.THIN_RADIUS, fs.THIN_FPFH_RADIUS)}
_scenes, _oracle_cache, _default = {}, {}, {}


def scene(key):
    if key not in _scenes:
        _scenes[key] = SCENES[key][0]()
    return _scenes[key]


def batch_on(pkg, ctx, dev, key):
    b = scene(key)
    return Batch(pkg, ctx, dev, b["objs"], b["kps"], SCENES[key][1], b["rgba"], b["kp_rgba"])


def oracle_frames(ora, s, key):
    if ("lrf", key) not in _oracle_cache:
        _oracle_cache["lrf", key] = ora.shot_lrf(s.pt_off, *fs.cols(s.p), s.kp_off, *fs.cols(s.kp), SCENES[key][2])
    return _oracle_cache["lrf", key]


def oracle_fpfh(ora, s, key):
    if ("fpfh", key) not in _oracle_cache:
        off, kp, _ = s.keypoints(scene(key)["fpfh_kps"])
        _oracle_cache["fpfh", key] = ora.fpfh33(s.pt_off, *fs.cols(s.p), *fs.cols(s.n), off, *fs.cols(kp), SCENES[key][3])
    return _oracle_cache["fpfh", key]


def run_front_end(pkg, s, key, lrf=None):
    """frames, SHOT, CSHOT (on these frames, or on `lrf` when given) and FPFH of a scene on the batch's context -> numpy"""
    capi, ctx = pkg.capi, s.ctx
    radius, fpfh_radius = SCENES[key][2:]
    own = capi.shot_lrf(ctx, s.cloud, s.kp_off, *s.tk, radius)
    use = own if lrf is None else T(lrf, s.dev)
    shot, cnt = capi.shot352(ctx, s.cloud, s.kp_off, *s.tk, use, radius, want_counts=True)
    cshot, ccnt = capi.cshot1344(ctx, s.cloud, s.kp_off, *s.tk, s.t_kp_rgba, use, radius, want_counts=True)
    off, kp, tk = s.keypoints(scene(key)["fpfh_kps"])
    fpfh, fcnt = capi.fpfh33(ctx, s.cloud, off, *tk, fpfh_radius, want_counts=True)
    return dict(lrf=own.cpu().numpy(), shot=shot.cpu().numpy(), cnt=cnt.cpu().numpy().astype(np.uint32), cshot=cshot.cpu().numpy(),
                ccnt=ccnt.cpu().numpy().astype(np.uint32), fpfh=fpfh.cpu().numpy(), fcnt=fcnt.cpu().numpy().astype(np.uint32))


def default_outputs(pkg, gpu, key):
    """the scene on the shared default context"""
    if key not in _default:
        ctx, dev = gpu
        s = batch_on(pkg, ctx, dev, key)
        try:
            _default[key] = (s, run_front_end(pkg, s, key))
        finally:
            ctx.sync(); s.close()
    return _default[key]


def assert_matches_oracle(ora, s, got, key):
    """every output of run_front_end (SHOT / CSHOT on the device's own frames) against the oracle; no keypoint is exempted"""
    radius = SCENES[key][2]
    want_lrf = oracle_frames(ora, s, key)
    assert_close_nan(got["lrf"], want_lrf, LRF_TOL)
    (x, y, z), (nx, ny, nz), (kx, ky, kz) = fs.cols(s.p), fs.cols(s.n), fs.cols(s.kp)
    want, wcnt = ora.shot352(s.pt_off, x, y, z, nx, ny, nz, s.kp_off, kx, ky, kz, got["lrf"], radius)
    assert np.array_equal(got["cnt"], wcnt)
    assert_close_nan(got["shot"], want, TOL)
    want, ccnt = ora.cshot1344(s.pt_off, x, y, z, nx, ny, nz, s.rgba, s.kp_off, kx, ky, kz, s.kp_rgba, got["lrf"], radius)
    assert np.array_equal(got["ccnt"], ccnt)
    assert_close_nan(got["cshot"], want, TOL)
    want, fcnt = oracle_fpfh(ora, s, key)
    assert np.array_equal(got["fcnt"], fcnt)
    assert_close_nan(got["fpfh"], want, FPFH_TOL)
    return want_lrf, wcnt, want, fcnt


@pytest.mark.parametrize("key", [WIDE_FUSED, WIDE_FIVE])
def test_wide_dense_batch_matches_oracle(pkg, gpu, ora, key):
    """11 objects, the dense one (5 000 - 28 000 neighbours per keypoint, >= 140 cell rows, single rows of > 6 000 candidates) at the
    origin and at (1000, -2500, 400); 65 000 points (one-kernel grid build) and 80 000 (five-kernel build)."""
    s, got = default_outputs(pkg, gpu, key)
    want_lrf, wcnt, want_fpfh, fcnt = assert_matches_oracle(ora, s, got, key)
    assert np.isnan(want_lrf[:, 0]).any() and np.isfinite(want_lrf[:40]).all() and np.isfinite(want_lrf[83:123]).all()
    assert wcnt[:40].min() > 4000 and wcnt[:40].max() > 20000 and wcnt[83:123].max() > 20000       # the dense object and its far copy
    assert fcnt.max() > 250 and np.isfinite(want_fpfh).any() and len(want_fpfh) == 12 + 5 + 1 + 4 + 5 + 3


def test_thin_dense_batch_matches_oracle(pkg, gpu, ora):
    """the scene of the ISMHIP_GRID_XFRAC cases on the default grid: the dense object with its short axis along x"""
    s, got = default_outputs(pkg, gpu, THIN)
    want_lrf, wcnt, want_fpfh, fcnt = assert_matches_oracle(ora, s, got, THIN)
    assert np.isfinite(want_lrf).all() and wcnt[:80].max() > 40000 and np.isfinite(want_fpfh).all()


@pytest.mark.parametrize("key", [WIDE_FUSED, WIDE_FIVE, THIN])
def test_cshot_sector_sums_agree_between_the_channels(pkg, gpu, key):
    """In every sector the 11 shape bins and the 31 colour bins of a CSHOT row sum to the same value: a home neighbour adds 1 + winc to
    either channel and the side deposits are the same numbers. Needs no reference; the bound (shot_ref_scenes.sector_sum_bound: float
    rounding of the two home weights, 2^-29 per fixed-point deposit, the output's cast and divide) is derived there. Balls of 5 000 to
    40 000 neighbours: a deposit lost in one channel of a sector moves its sum by 1 / N, a thousand bounds."""
    import shot_ref_scenes as srs
    _, got = default_outputs(pkg, gpu, key)
    fin = np.isfinite(got["cshot"][:, 0])
    a, c = srs.sector_sums(got["cshot"][fin])
    diff, bound = np.abs(a - c), srs.sector_sum_bound(a, c)
    print("%s: largest sector-sum difference %.3g (bound there %.3g) at sector sums up to %.3g, %d rows, up to %d neighbours"
          % (key, diff.max(), bound.flat[np.argmax(diff)], a.max(), fin.sum(), got["ccnt"].max()))
    assert fin.sum() >= 80 and got["ccnt"].max() > 20000
    assert (diff <= bound).all()


@pytest.mark.parametrize("env,value,key", [("ISMHIP_SHOT_VAR", "2", WIDE_FUSED), ("ISMHIP_XCD_MAP", "0", WIDE_FUSED)] +
                         [("ISMHIP_GRID_XFRAC", str(v), THIN) for v in fs.XFRACS])
def test_switches_leave_the_bytes_alone(pkg, gpu, ora, env, value, key, monkeypatch):
    """The SHOT histogram is integer fixed point: neither the sweep order (SHOT_VAR=2), nor the block order (XCD_MAP=0), nor the
    shape of the grid cells (GRID_XFRAC) may change one bit of SHOT / CSHOT or a neighbour count. Frames and FPFH sum in floating
    point in sweep order: they stay within their oracle tolerances. The XFRAC cases run on the thin batch, whose x axis stays below
    the per-axis cell cap, so that every value really builds another grid (test_frontend_cpu.py asserts that it does)."""
    _, dev = gpu
    _, base = default_outputs(pkg, gpu, key)
    monkeypatch.setenv(env, value)
    ctx = pkg.capi.Ctx(0)                                                   # the switches are read when a context is created
    s = batch_on(pkg, ctx, dev, key)
    try:
        got = run_front_end(pkg, s, key, lrf=base["lrf"])                   # SHOT on the SAME frames as the default run
    finally:
        ctx.sync(); s.close(); ctx.close()
    assert np.array_equal(got["cnt"], base["cnt"]) and np.array_equal(got["ccnt"], base["ccnt"]) and np.array_equal(got["fcnt"], base["fcnt"])
    assert got["cnt"].max() > 20000
    assert got["shot"].tobytes() == base["shot"].tobytes()
    assert got["cshot"].tobytes() == base["cshot"].tobytes()
    assert_close_nan(got["lrf"], oracle_frames(ora, s, key), LRF_TOL)
    assert_close_nan(got["fpfh"], oracle_fpfh(ora, s, key)[0], FPFH_TOL)


def test_fpfh33_through_a_second_candidate_window(pkg, gpu, ora):
    """three keypoints inside a 7000-point clump at radius 0.006: every marked clump point's sweep in k_spfh holds all 7000
    candidates in ONE row batch (> 1.5 windows), of which ~1 500 are neighbours"""
    ctx, dev = gpu
    p, n, kp = fs.fpfh_clump_object()
    s = Batch(pkg, ctx, dev, [(p, n)], [kp], fs.DENSE_CELL)
    got, cnt = pkg.capi.fpfh33(ctx, s.cloud, s.kp_off, *s.tk, fs.FPFH_CLUMP_RADIUS, want_counts=True)
    got, cnt = got.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)
    s.close()
    want, wcnt = ora.fpfh33(s.pt_off, *fs.cols(s.p), *fs.cols(s.n), s.kp_off, *fs.cols(s.kp), fs.FPFH_CLUMP_RADIUS)
    assert np.array_equal(cnt, wcnt) and wcnt.min() >= 500 and np.isfinite(want).all()
    assert_close_nan(got, want, FPFH_TOL)


def test_pca_normals_over_more_than_one_row_batch(pkg, gpu, ora):
    """k_pca_normals with a ball of 65 - 117 cell rows at every surface point of an 8 000-point object with a dense disc; criteria
    of test_estimate_normals_pca (the oracle follows PCL's float covariance: 2e-3)."""
    import torch
    ctx, dev = gpu
    objs = fs.normals_scene()
    off = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.uint32)
    P = np.concatenate(objs).astype(np.float32)
    t = [T(c, dev) for c in fs.cols(P)]
    zn = [torch.zeros(len(P), dtype=torch.float32, device=dev) for _ in range(3)]
    cloud = pkg.capi.Cloud(ctx, off, *t, *zn, fs.NORMALS_CELL)
    out = [torch.empty(len(P), dtype=torch.float32, device=dev) for _ in range(3)]
    pkg.capi.estimate_normals_pca(ctx, cloud, fs.NORMALS_RADIUS, 1, *out)
    got = np.stack([a.cpu().numpy() for a in out], 1)
    cloud.close()
    want = ora.pca_normals(off, *fs.cols(P), fs.NORMALS_RADIUS, 1)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[33]).all() and np.isnan(got[-1]).all()
    m = ~np.isnan(want).any(1)
    assert m.sum() == len(P) - 3
    dots = (got[m] * want[m]).sum(1)
    assert (dots > 0).mean() > 0.999
    ang = np.arccos(np.clip(np.abs(dots), 0, 1))
    assert np.quantile(ang, 0.995) < 2e-3, np.quantile(ang, 0.995)
    np.testing.assert_allclose(np.linalg.norm(got[m], axis=1), 1.0, atol=1e-5)


# ------------------------------------------------------------------------------------------------ LRF ties
@pytest.mark.parametrize("m", fs.MIRROR_M)
def test_lrf_ties_at_every_key_store(pkg, gpu, ora, m):
    """Neighbourhoods of 800 and 1280 (keys in registers), 1282, 3000 and 8192 (LDS), 8194 and 12 000 (global scratch); both signs
    of every frame are tied (test_frontend_cpu), so the five median neighbours by (d^2, index) decide them."""
    ctx, dev = gpu
    pts = fs.mirror_cloud(m)
    s = Batch(pkg, ctx, dev, [(pts, np.zeros_like(pts))], [np.zeros((1, 3), np.float32)], fs.MIRROR_CELL)
    got = pkg.capi.shot_lrf(ctx, s.cloud, s.kp_off, *s.tk, fs.MIRROR_RADIUS).cpu().numpy()
    s.close()
    want = ora.shot_lrf(s.pt_off, *fs.cols(s.p), s.kp_off, *fs.cols(s.kp), fs.MIRROR_RADIUS)
    assert np.isfinite(want).all()
    assert_close_nan(got, want, LRF_TOL)


def test_lrf_more_ties_than_tie_workgroups(pkg, gpu, ora):
    """1100 keypoints at the centre of an 800-point mirror cloud (+ one that is not tied, in a second object): more ties than the
    1024 workgroups of k_lrf_tie, so some take a second item from the queue"""
    ctx, dev = gpu
    pts = fs.mirror_cloud(400)
    other = fs.mirror_cloud(641)[:700] + np.float32([5, 0, 0])
    kps = [np.zeros((fs.QUEUE_KEYPOINTS, 3), np.float32), np.float32([[5, 0, 0]])]
    s = Batch(pkg, ctx, dev, [(pts, np.zeros_like(pts)), (other, np.zeros_like(other))], kps, fs.MIRROR_CELL)
    got = pkg.capi.shot_lrf(ctx, s.cloud, s.kp_off, *s.tk, fs.MIRROR_RADIUS).cpu().numpy()
    s.close()
    want = ora.shot_lrf(s.pt_off, *fs.cols(s.p), s.kp_off, *fs.cols(s.kp), fs.MIRROR_RADIUS)
    assert np.isfinite(want).all() and (want[:fs.QUEUE_KEYPOINTS] == want[0]).all()
    assert_close_nan(got, want, LRF_TOL)


# ------------------------------------------------------------------------------------------------ exact boundaries
def lattice_batch(pkg, ctx, dev, with_color):
    """the three lattices (one per frame, its edge normals along that frame's z) as three objects, keypoints at the origin"""
    objs = [fs.lattice(fr) for fr in fs.LATTICE_FRAMES]
    kps = [np.zeros((1, 3), np.float32)] * 3
    rgba = kp_rgba = None
    if with_color:
        rgba = [fs.lattice_colors(o[0], 61 + i) for i, o in enumerate(objs)]
        kp_rgba = [np.array([fs.EDGE_KP_COLOR], np.uint32) for _ in objs]
    return Batch(pkg, ctx, dev, objs, kps, 0.125, rgba, kp_rgba), np.stack(fs.LATTICE_FRAMES)


@pytest.mark.parametrize("radius", fs.LATTICE_RADII)
def test_shot352_on_the_boundary_lattice(pkg, gpu, ora, radius):
    """xl, yl, zl == 0, |xl| == |yl|, d^2 == r^2/4, the cosine on / beside every bin edge, d^2 == r^2 (excluded): the oracle takes
    these decisions in double like the reference, shot_hard_bin and r12sq_f must take them the same way. The points also lie
    exactly on cell faces of the grid (cell 1/8)."""
    ctx, dev = gpu
    s, frames = lattice_batch(pkg, ctx, dev, False)
    got, cnt = pkg.capi.shot352(ctx, s.cloud, s.kp_off, *s.tk, T(frames, dev), radius, want_counts=True)
    got, cnt = got.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)
    s.close()
    want, wcnt = ora.shot352(s.pt_off, *fs.cols(s.p), *fs.cols(s.n), s.kp_off, *fs.cols(s.kp), frames, radius)
    assert np.array_equal(cnt, wcnt) and wcnt.tolist() == [fs.lattice_census(s.p[:729], fs.LATTICE_FRAMES[0], radius)["n"]] * 3
    assert np.isfinite(want).all()
    assert_close_nan(got, want, TOL)


@pytest.mark.parametrize("radius", fs.LATTICE_RADII)
def test_cshot1344_on_the_boundary_lattice(pkg, gpu, ora, radius):
    """the same lattice; the neighbours nearest the keypoint carry colours whose colour distance cd makes cd * 30 + 0.5 the float at,
    just below or just above an integer (frontend_scenes.EDGE_COLORS): the hard decision of the colour bin"""
    ctx, dev = gpu
    s, frames = lattice_batch(pkg, ctx, dev, True)
    got, cnt = pkg.capi.cshot1344(ctx, s.cloud, s.kp_off, *s.tk, s.t_kp_rgba, T(frames, dev), radius, want_counts=True)
    got, cnt = got.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)
    s.close()
    want, wcnt = ora.cshot1344(s.pt_off, *fs.cols(s.p), *fs.cols(s.n), s.rgba, s.kp_off, *fs.cols(s.kp), s.kp_rgba, frames, radius)
    assert np.array_equal(cnt, wcnt)
    assert_close_nan(got, want, TOL)


@pytest.mark.parametrize("color", [False, True], ids=["shot352", "cshot1344"])
def test_shot_neighbour_counts_around_the_queue_sizes(pkg, gpu, ora, color):
    """4 (NaN), 5, 63, 64, 65, 127, 128, 129 neighbours, and 5 of which one IS the keypoint: the frame estimate skips it (4 valid
    neighbours -> NaN frame), SHOT on a supplied frame counts it (5 -> a finite row)."""
    ctx, dev = gpu
    pts, nrm, kps, frames, counts = fs.queue_clusters()
    rng = np.random.default_rng(71)
    rgba = [rng.integers(0, 1 << 24, size=len(pts)).astype(np.uint32)] if color else None
    kp_rgba = [rng.integers(0, 1 << 24, size=len(kps)).astype(np.uint32)] if color else None
    s = Batch(pkg, ctx, dev, [(pts, nrm)], [kps], 0.12, rgba, kp_rgba)
    lrf = pkg.capi.shot_lrf(ctx, s.cloud, s.kp_off, *s.tk, fs.QUEUE_RADIUS).cpu().numpy()
    if color:
        got, cnt = pkg.capi.cshot1344(ctx, s.cloud, s.kp_off, *s.tk, s.t_kp_rgba, T(frames, dev), fs.QUEUE_RADIUS, want_counts=True)
    else:
        got, cnt = pkg.capi.shot352(ctx, s.cloud, s.kp_off, *s.tk, T(frames, dev), fs.QUEUE_RADIUS, want_counts=True)
    got, cnt = got.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)
    s.close()
    a = (s.pt_off, *fs.cols(s.p))
    want_lrf = ora.shot_lrf(*a, s.kp_off, *fs.cols(s.kp), fs.QUEUE_RADIUS)
    assert_close_nan(lrf, want_lrf, LRF_TOL)
    assert np.isnan(want_lrf[0]).all() and np.isnan(want_lrf[-1]).all() and np.isfinite(want_lrf[1:-1]).all()
    if color:
        want, wcnt = ora.cshot1344(*a, *fs.cols(s.n), s.rgba, s.kp_off, *fs.cols(s.kp), s.kp_rgba, frames, fs.QUEUE_RADIUS)
    else:
        want, wcnt = ora.shot352(*a, *fs.cols(s.n), s.kp_off, *fs.cols(s.kp), frames, fs.QUEUE_RADIUS)
    assert cnt.tolist() == counts.tolist() and wcnt.tolist() == counts.tolist()
    assert np.isnan(want[0]).all() and np.isfinite(want[1:]).all()
    assert_close_nan(got, want, TOL)


def test_fpfh33_on_the_bin_edges(pkg, gpu, ora):
    """30 four-point objects whose f3 is the float below / at / above every bin edge 2j/11 - 1: inside the guard band of the fast
    bins, where the exact double-precision floor must decide as the reference does. One wrong bin moves a value by >= 14."""
    ctx, dev = gpu
    objs, kps = fs.fpfh_edge_objects()
    s = Batch(pkg, ctx, dev, objs, kps, 0.1)
    got, cnt = pkg.capi.fpfh33(ctx, s.cloud, s.kp_off, *s.tk, fs.FPFH_EDGE_RADIUS, want_counts=True)
    got, cnt = got.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)
    s.close()
    want, wcnt = ora.fpfh33(s.pt_off, *fs.cols(s.p), *fs.cols(s.n), s.kp_off, *fs.cols(s.kp), fs.FPFH_EDGE_RADIUS)
    assert np.array_equal(cnt, wcnt) and (wcnt == 4).all() and np.isfinite(want).all()
    for j in range(10):                                                     # one float below and one above the edge: different bins
        assert np.abs(want[3 * j, 22:] - want[3 * j + 2, 22:]).max() > 14
    assert_close_nan(got, want, FPFH_TOL)

"""The one-kernel grid build (k_grid_fused, one workgroup per object) against the five-kernel build it replaces: everything that
depends on the cell-sorted order of a cloud must come out with the same BYTES, on inputs chosen to break a counting sort."""
import numpy as np
import pytest

from conftest import make_cloud

pytestmark = pytest.mark.gpu

CELL, R_LRF, R_SHOT, R_FPFH, R_NRM = 0.12, 0.3, 0.3, 0.25, 0.15
FUSED_MAX_PTS = 65536          # GRID_FUSED_MAX_PTS of csrc/grid.hip: a batch with a larger object takes the five-kernel build


def _objects(rng):
    """list of (xyz float32 [n, 3], normals float32 [n, 3]) -- the batch of the issue's check 3"""
    objs = []
    p, n = make_cloud(rng, 17, "sphere"); objs.append((p, n))                      # 17 points next to ...
    p, n = make_cloud(rng, 40000, "ellipsoid"); objs.append((p, n))                # ... 40 000
    objs.append((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)))       # empty object
    p, n = make_cloud(rng, 1, "sphere"); objs.append((p, n))                        # one point
    p, n = make_cloud(rng, 9000, "sphere", noise=0.01)                              # thousands of points in ONE cell:
    p[2000:6500] = p[1999]; objs.append((p, n))                                     # 4500 copies of one coordinate, in the middle
    p, n = make_cloud(rng, 6000, "plane", noise=0.02)                               # NaN / Inf points in the middle
    p[1000:1300, 0] = np.nan; p[3000:3100, 2] = np.inf; p[4000, 1] = -np.inf; objs.append((p, n))
    p, n = make_cloud(rng, 30000, "sphere", noise=0.02)                             # extent 6 = 50 cells requested: the 32-cells-per-axis cap
    objs.append((p * np.float32(3.0), n))                                           # engages on every axis (32768 cells: table in global memory)
    p, n = make_cloud(rng, 5000, "ellipsoid"); objs.append((p + np.float32(3.0), n))
    p, n = make_cloud(rng, 3000, "sphere"); objs.append((p, n))
    return objs


def _batch(objs, dev, colour=False, rng=None):
    import torch
    xyz = np.concatenate([o[0] for o in objs]); nrm = np.concatenate([o[1] for o in objs])
    po = np.concatenate([[0], np.cumsum([len(o[0]) for o in objs])]).astype(np.uint32)
    kps, ko = [], [0]
    for p, _ in objs:                                                               # keypoints: a spread of the object's own points
        k = p[:: max(1, len(p) // 48)][:64]
        kps.append(k); ko.append(ko[-1] + len(k))
    kp = np.concatenate(kps)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    pts = [T(xyz[:, i]) for i in range(3)] + [T(nrm[:, i]) for i in range(3)]
    rgba = T(rng.integers(0, 1 << 24, size=len(xyz), dtype=np.uint32).view(np.int32)) if colour else None
    krgba = T(rng.integers(0, 1 << 24, size=len(kp), dtype=np.uint32).view(np.int32)) if colour else None
    return dict(po=po, pts=pts, ko=np.asarray(ko, np.uint32), kp=[T(kp[:, i]) for i in range(3)], rgba=rgba, krgba=krgba)


def _outputs(pkg, ctx, dev, b):
    """every result that depends on the sorted copy, as host byte strings"""
    import torch
    capi = pkg.capi
    pts = [t.clone() for t in b["pts"]]
    cloud = capi.Cloud(ctx, b["po"], *pts, CELL, rgba=b["rgba"])
    out = {}
    out["centroids"] = capi.cloud_centroids(ctx, cloud, dev)
    out["lrf"] = capi.shot_lrf(ctx, cloud, b["ko"], *b["kp"], R_LRF)
    out["shot"], out["shot_cnt"] = capi.shot352(ctx, cloud, b["ko"], *b["kp"], out["lrf"], R_SHOT, want_counts=True)
    out["fpfh"], out["fpfh_cnt"] = capi.fpfh33(ctx, cloud, b["ko"], *b["kp"], R_FPFH, want_counts=True)
    if b["rgba"] is not None:
        out["cshot"], out["cshot_cnt"] = capi.cshot1344(ctx, cloud, b["ko"], *b["kp"], b["krgba"], out["lrf"], R_SHOT, want_counts=True)
    n = pts[0].numel()
    nn = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)]
    capi.estimate_normals_pca(ctx, cloud, R_NRM, 0, *nn)
    out["pca_nx"], out["pca_ny"], out["pca_nz"] = nn
    out["shot_pca"] = capi.shot352(ctx, cloud, b["ko"], *b["kp"], out["lrf"], R_SHOT)   # reads the sorted normals the PCA pass has rewritten
    ctx.sync()
    res = {k: v.cpu().numpy().tobytes() for k, v in out.items()}
    cloud.close()
    return res


def _ctx(pkg, monkeypatch, fused):
    if fused:
        monkeypatch.delenv("ISMHIP_GRID_FUSED", raising=False)
    else:
        monkeypatch.setenv("ISMHIP_GRID_FUSED", "0")
    return pkg.capi.Ctx(0)                                                          # the switches are read when a ctx is created


def _compare(pkg, monkeypatch, dev, b):
    res = []
    for fused in (False, True):
        ctx = _ctx(pkg, monkeypatch, fused)
        try:
            res.append(_outputs(pkg, ctx, dev, b))
        finally:
            ctx.close()
    assert res[0].keys() == res[1].keys()
    for k in res[0]:
        assert len(res[0][k]) > 0
        assert res[0][k] == res[1][k], f"{k}: the one-kernel grid build changes the bytes"
    return res[1]


def test_fused_grid_same_bytes_adversarial_batch(pkg, gpu, monkeypatch):
    _, dev = gpu
    rng = np.random.default_rng(11)
    objs = _objects(rng)
    assert len(objs) >= 8 and max(len(o[0]) for o in objs) <= FUSED_MAX_PTS        # XCD-local block map, fused build
    res = _compare(pkg, monkeypatch, dev, _batch(objs, dev))
    lrf = np.frombuffer(res["lrf"], np.float32)
    assert np.isfinite(lrf).sum() > lrf.size // 2                                   # the comparison is not one of NaN against NaN


def test_fused_grid_same_bytes_coloured(pkg, gpu, monkeypatch):
    _, dev = gpu
    rng = np.random.default_rng(12)
    objs = _objects(rng)
    _compare(pkg, monkeypatch, dev, _batch(objs, dev, colour=True, rng=rng))


def test_fused_grid_same_bytes_few_objects(pkg, gpu, monkeypatch):
    """fewer than 8 objects: plain object-major block order"""
    _, dev = gpu
    rng = np.random.default_rng(13)
    objs = _objects(rng)
    _compare(pkg, monkeypatch, dev, _batch([objs[4], objs[1], objs[5]], dev))
    _compare(pkg, monkeypatch, dev, _batch([objs[6]], dev))


def test_large_object_takes_five_kernel_build(pkg, gpu, monkeypatch):
    """an object beyond GRID_FUSED_MAX_PTS sends the batch to the five-kernel build: same bytes with either switch setting, and the
    same bytes for the small objects of the batch as when they are built (fused) without the large one"""
    _, dev = gpu
    rng = np.random.default_rng(14)
    p, n = make_cloud(rng, FUSED_MAX_PTS + 5000, "ellipsoid")
    small = _objects(rng)[4:6]
    res = _compare(pkg, monkeypatch, dev, _batch([(p, n)] + small, dev))
    ctx = _ctx(pkg, monkeypatch, True)
    try:
        alone = _outputs(pkg, ctx, dev, _batch(small, dev))
    finally:
        ctx.close()
    nk = [len(o[0][:: max(1, len(o[0]) // 48)][:64]) for o in [(p, n)] + small]
    for k, width in (("lrf", 9), ("shot", 352), ("fpfh", 33)):
        assert res[k][nk[0] * width * 4:] == alone[k], k


def test_fused_grid_is_deterministic(pkg, gpu, monkeypatch):
    """the same batch built three times gives identical bytes; enough objects that workgroups of different objects share every CU"""
    _, dev = gpu
    rng = np.random.default_rng(15)
    b = _batch(_objects(rng) + [make_cloud(rng, 16384, "ellipsoid") for _ in range(600)], dev)
    ctx = _ctx(pkg, monkeypatch, True)
    try:
        runs = [_outputs(pkg, ctx, dev, b) for _ in range(3)]
    finally:
        ctx.close()
    for r in runs[1:]:
        for k in runs[0]:
            assert r[k] == runs[0][k], k

"""Keypoints in cell order (ISMHIP_KP_ORDER, on by default): LRF and SHOT give wave w of block b the keypoint perm[4 b + w] and write its
row at the keypoint's own index, so every output must have the same BYTES as with the keypoints taken in the caller's order."""
import numpy as np
import pytest

from conftest import make_cloud

pytestmark = pytest.mark.gpu

CELL, R = 0.12, 0.3


def _scene(rng, dev, n_kp):
    """objects with n_kp[o] keypoints each, in random order; a NaN keypoint and a keypoint far outside the cloud among them"""
    import torch
    objs = [make_cloud(rng, 6000 + 1500 * o, ("ellipsoid", "sphere", "plane")[o % 3], noise=0.01) for o in range(len(n_kp))]
    xyz = np.concatenate([o[0] for o in objs]); nrm = np.concatenate([o[1] for o in objs])
    po = np.concatenate([[0], np.cumsum([len(o[0]) for o in objs])]).astype(np.uint32)
    kps = []
    for (p, _), n in zip(objs, n_kp):
        k = p[rng.integers(0, len(p), size=n)].copy()
        if n > 20:
            k[7] = np.nan; k[11] = 50.0
        kps.append(k)
    ko = np.concatenate([[0], np.cumsum(n_kp)]).astype(np.uint32)
    kp = np.concatenate(kps).astype(np.float32)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    rgba = T(rng.integers(0, 1 << 24, size=len(xyz), dtype=np.uint32).view(np.int32))
    krgba = T(rng.integers(0, 1 << 24, size=len(kp), dtype=np.uint32).view(np.int32))
    return dict(po=po, pts=[T(xyz[:, i]) for i in range(3)] + [T(nrm[:, i]) for i in range(3)], ko=ko, kp=[T(kp[:, i]) for i in range(3)],
                rgba=rgba, krgba=krgba)


def _run(pkg, ctx, s, s2):
    """LRF, SHOT and CSHOT of keypoint set s, then of a second set s2 on the SAME cloud (the cached order must not leak), then s again"""
    capi = pkg.capi
    cloud = capi.Cloud(ctx, s["po"], *s["pts"], CELL, rgba=s["rgba"])
    out = {}
    for tag, q in (("a", s), ("b", s2), ("c", s)):
        lrf = capi.shot_lrf(ctx, cloud, q["ko"], *q["kp"], R)
        desc, cnt = capi.shot352(ctx, cloud, q["ko"], *q["kp"], lrf, R, want_counts=True)
        cdesc = capi.cshot1344(ctx, cloud, q["ko"], *q["kp"], q["krgba"], lrf, R)
        out.update({tag + "_lrf": lrf, tag + "_shot": desc, tag + "_cnt": cnt, tag + "_cshot": cdesc})
    ctx.sync()
    res = {k: v.cpu().numpy().tobytes() for k, v in out.items()}
    cloud.close()
    return res


@pytest.mark.parametrize("n_kp", [[300, 0, 1, 1024, 64, 5, 2048, 33, 700], [500, 40], [5000, 100, 9]])
def test_cell_order_same_bytes(pkg, gpu, monkeypatch, n_kp):
    """9 objects (XCD-local block map, objects without and with one keypoint), 2 objects (plain block map), and an object with more
    keypoints than the order is built for (the batch then keeps the caller's order)"""
    _, dev = gpu
    rng = np.random.default_rng(21)
    s = _scene(rng, dev, n_kp)
    s2 = dict(s, **{k: v for k, v in _scene(np.random.default_rng(22), dev, n_kp).items() if k in ("ko", "kp", "krgba")})
    # the second set lies on the first set's cloud: same objects, other keypoints (generated from the same shapes with another seed)
    res = []
    for on in (False, True):
        if on:
            monkeypatch.delenv("ISMHIP_KP_ORDER", raising=False)
        else:
            monkeypatch.setenv("ISMHIP_KP_ORDER", "0")
        ctx = pkg.capi.Ctx(0)
        try:
            res.append(_run(pkg, ctx, s, s2))
        finally:
            ctx.close()
    for k in res[0]:
        assert res[0][k] == res[1][k], f"{k}: the keypoint order changes the bytes"
    assert res[1]["a_lrf"] == res[1]["c_lrf"] and res[1]["a_shot"] == res[1]["c_shot"]
    lrf = np.frombuffer(res[1]["a_lrf"], np.float32)
    assert np.isfinite(lrf).sum() > lrf.size // 2

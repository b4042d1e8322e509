"""ismhip_region_mvbb on the device (-m gpu) on the batch of mvbb_scenes.py, against the float64 restatement mvbb_ref.py and, on the
fixture scenes, against the real libgdiam-1.3's recorded answers.

n_sel exact. The trace equals the restatement's up to its first undecided decision (its `soft` entries aside). Where nothing is
undecided, centre, sizes and axes lie within the restatement's `tol`, the volume within its `vol_tol`. Properties that need no
restatement: every selected point inside the box, axes orthonormal and right-handed, sizes descending, volume <= the axis-aligned
volume, two calls the same bits, one launch = many launches, whole object = a ball that contains it, NULL trace / volume change nothing, bad arguments refused."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mvbb_ref as mr
import mvbb_scenes as ms
from test_gpu_frontend import Batch
from test_mvbb_cpu import GDIAM_TOL, OTHER_BOX, golden

pytestmark = pytest.mark.gpu
_state = {}


def region_arrays(regions):
    obj = [r[1] for r in regions]
    cen = [(0, 0, 0) if r[2] is None else r[2] for r in regions]
    rad = [-1.0 if r[3] is None else r[3] for r in regions]
    return np.asarray(obj, np.int32), np.asarray(cen, np.float32), np.asarray(rad, np.float32)


def run(pkg, gpu):
    """every call on the batch, once -> (batch, dict of numpy outputs per call)"""
    if "run" in _state:
        return _state["run"]
    ctx, dev = gpu
    bt = ms.batch()
    objs = [(bt["objects"][k], np.zeros_like(bt["objects"][k])) for k in bt["names"]]
    b = Batch(pkg, ctx, dev, objs, [np.zeros((0, 3), np.float32)] * len(objs), 0.1)
    try:
        obj, cen, rad = region_arrays(bt["regions"])
        host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
        out = dict(full=host(pkg.capi.region_mvbb(ctx, b.cloud, dev, obj, cen, rad)),
                   again=host(pkg.capi.region_mvbb(ctx, b.cloud, dev, obj, cen, rad)),
                   bare=host(pkg.capi.region_mvbb(ctx, b.cloud, dev, obj, cen, rad, want_volume=False, want_trace=False)))
        ctx.sync()
    finally:
        b.close()
    _state["run"] = (bt, out)
    return _state["run"]


def refs(bt):
    if "refs" not in _state:
        _state["refs"] = [mr.region_box(*ms.region_points(bt, r)) for r in bt["regions"]]
    return _state["refs"]


def selected(bt, region):
    p, cen, rad = ms.region_points(bt, region)
    return p[mr.select(p, cen, rad)].astype(np.float64)


def test_n_sel_and_empty_regions(pkg, gpu):
    bt, out = run(pkg, gpu)
    got = out["full"]
    n = len(bt["regions"])
    assert got["center"].shape == (n, 3) and got["size"].shape == (n, 3) and got["axes"].shape == (n, 9) and got["trace"].shape == (n, 48)
    for r, region in enumerate(bt["regions"]):
        k = len(selected(bt, region))
        assert int(got["n_sel"][r]) == k, region[0]
        if k == 0:
            assert np.isnan(got["center"][r]).all() and np.isnan(got["axes"][r]).all() and (got["size"][r] == 0).all() and got["volume"][r] == 0
    names = [r[0] for r in bt["regions"]]
    for k in ("ball_empty", "object_below", "object_above"):
        assert got["n_sel"][names.index(k)] == 0
    assert got["n_sel"][names.index("with_nan")] == 199 and got["n_sel"][names.index("ball_all")] == 400


def test_trace_follows_the_restatement(pkg, gpu):
    bt, out = run(pkg, gpu)
    got, ref = out["full"], refs(bt)
    undecided = 0
    for r, region in enumerate(bt["regions"]):
        b = ref[r]
        keep = [k for k in range(b["undecided_at"]) if k not in b["soft"]]
        assert got["trace"][r][keep].tolist() == [b["trace"][k] for k in keep], (region[0], b["undecided_at"])
        undecided += b["undecided_at"] < mr.TRACE
    assert undecided * 20 <= len(bt["regions"])


def test_box_within_the_restatements_bound(pkg, gpu):
    bt, out = run(pkg, gpu)
    got, ref = out["full"], refs(bt)
    checked = equal_bits = 0
    for r, region in enumerate(bt["regions"]):
        b = ref[r]
        if b["n"] == 0 or b["undecided_at"] < mr.TRACE:
            continue
        checked += 1
        want = np.concatenate([b["center"], b["size"], np.ravel(b["axes"])])
        have = np.concatenate([got["center"][r], got["size"][r], got["axes"][r]]).astype(np.float64)
        print(region[0], "max deviation", np.abs(have - want).max(), "tol", b["tol"], "volume", got["volume"][r] - b["volume"], "tol", b["vol_tol"])
        assert np.abs(have[:6] - want[:6]).max() <= b["tol"], region[0]
        assert np.abs(have[6:] - want[6:]).max() <= b["tol"] / max(np.abs(selected(bt, region)).max(), 1e-300) + 2.0 ** -22, region[0]
        assert abs(got["volume"][r] - b["volume"]) <= b["vol_tol"], region[0]
        equal_bits += bool(np.array_equal(have.astype(np.float32).view(np.uint32), want.astype(np.float32).view(np.uint32)) and got["volume"][r] == b["volume"])
    print("regions compared", checked, "bit-equal", equal_bits)
    assert checked >= len(bt["regions"]) * 0.9
    assert equal_bits == checked                              # sqrt and division are correctly rounded on the device: the same bits


def test_fixture_scenes_against_gdiam(pkg, gpu):
    bt, out = run(pkg, gpu)
    got = out["full"]
    names = [r[0] for r in bt["regions"]]
    for name, e in golden().items():
        v = got["volume"][names.index(name)]
        print(name, "volume / gdiam - 1 =", v / e["volume"] - 1)
        if name in OTHER_BOX:
            assert v < e["volume"] * (1 - 1e-3), name
        else:
            assert abs(v / e["volume"] - 1) <= GDIAM_TOL, name


def test_properties(pkg, gpu):
    bt, out = run(pkg, gpu)
    got = out["full"]
    for r, region in enumerate(bt["regions"]):
        p = selected(bt, region)
        if len(p) == 0:
            continue
        c, s, a = got["center"][r].astype(np.float64), got["size"][r].astype(np.float64), got["axes"][r].astype(np.float64).reshape(3, 3)
        scale = np.abs(p).max() + np.ptp(p, axis=0).max()
        assert np.abs(a @ a.T - np.eye(3)).max() <= 8 * 2.0 ** -24, region[0]
        assert np.linalg.det(a) > 0.999, region[0]
        assert s[0] >= s[1] >= s[2] >= 0, region[0]
        local = (p - c) @ a.T
        assert (np.abs(local) <= s / 2 + scale * 2.0 ** -19).all(), (region[0], np.abs(local).max(0), s / 2)
        aabb = np.prod(np.ptp(p, axis=0))
        assert got["volume"][r] <= aabb * (1 + 2.0 ** -40), region[0]
        assert abs(np.prod(s) - got["volume"][r]) <= 2.0 ** -20 * max(np.prod(s), got["volume"][r]) + scale ** 3 * 2.0 ** -40, region[0]
        for k in (0, 1):                                       # axes 1 and 2: the component of largest magnitude is positive
            assert a[k][np.argmax(np.abs(a[k]))] > 0, region[0]
    names = [x[0] for x in bt["regions"]]
    assert got["trace"][names.index("aligned_box")][4] == 1 and got["trace"][names.index("rotated_box")][4] == 0
    assert got["trace"][names.index("collinear")][5] == 1 and got["trace"][names.index("two_points")][5] == 1
    for k in ("one_point", "coincident"):
        r = names.index(k)
        assert got["trace"][r][6] == 1 and (got["size"][r] == 0).all() and got["volume"][r] == 0
        assert np.array_equal(got["axes"][r], np.eye(3, dtype=np.float32).ravel()) and np.array_equal(got["center"][r], bt["objects"][k][0])
    assert got["trace"][names.index("circle")][9::4].max() == 300          # a round sees the circle face on: every point a hull vertex
    # the work-buffer scenes really left the LDS staging: the kernel reports the most survivors of a round in trace [7]
    assert (got["trace"][:, 7] <= got["n_sel"]).all()
    for k in ms.WORK_BUFFER_SCENES:
        assert got["trace"][names.index(k)][7] > ms.LDS_SURVIVORS, (k, got["trace"][names.index(k)][7])
    r = names.index("circle_1000")
    assert got["trace"][r][9::4].max() == 1000 and got["trace"][r][7] == 1000       # every point survives and is a hull vertex
    assert refs(bt)[names.index("ellipsoid_surface")]["undecided_at"] == mr.TRACE      # and this one is compared bit for bit above
    assert got["volume"][names.index("planar_patch")] < 1e-6 and got["size"][names.index("planar_patch")][2] < 1e-6


def test_same_bits_on_every_call_and_without_the_optional_outputs(pkg, gpu):
    _, out = run(pkg, gpu)
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8)
    for k in ("n_sel", "center", "size", "axes", "volume", "trace"):
        assert np.array_equal(raw(out["full"][k]), raw(out["again"][k])), k
    for k in ("n_sel", "center", "size", "axes"):
        assert np.array_equal(raw(out["full"][k]), raw(out["bare"][k])), k
    assert "volume" not in out["bare"] and "trace" not in out["bare"]


def test_several_launches_give_the_same_bits(pkg, gpu, monkeypatch):
    """a work buffer of 1 MiB holds three regions of this batch (76 B per point of its largest object, 4000 points): the call is
    served by some forty launches that reuse the buffer, and every output equals the single launch's"""
    bt, out = run(pkg, gpu)
    _, dev = gpu
    monkeypatch.setenv("ISMHIP_MVBB_WORK_MB", "1")
    ctx = pkg.capi.Ctx(0)
    try:
        objs = [(bt["objects"][k], np.zeros_like(bt["objects"][k])) for k in bt["names"]]
        b = Batch(pkg, ctx, dev, objs, [np.zeros((0, 3), np.float32)] * len(objs), 0.1)
        try:
            assert (1 << 20) // (76 * int(np.diff(bt["pt_off"].astype(np.int64)).max())) == 3
            got = {k: v.cpu().numpy() for k, v in pkg.capi.region_mvbb(ctx, b.cloud, dev, *region_arrays(bt["regions"])).items()}
            ctx.sync()
        finally:
            b.close()
    finally:
        ctx.close()
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8)
    for k in ("n_sel", "center", "size", "axes", "volume", "trace"):
        assert np.array_equal(raw(out["full"][k]), raw(got[k])), k


def test_whole_object_equals_a_ball_that_contains_it(pkg, gpu):
    bt, out = run(pkg, gpu)
    got = out["full"]
    names = [r[0] for r in bt["regions"]]
    a, b = names.index("rotated_box"), names.index("ball_all")
    raw = lambda x: np.ascontiguousarray(x).view(np.uint8)
    for k in ("n_sel", "center", "size", "axes", "volume", "trace"):
        assert np.array_equal(raw(got[k][a]), raw(got[k][b])), k


def test_bad_arguments_are_refused_and_the_context_stays_usable(pkg, gpu):
    import torch
    ctx, dev = gpu
    capi = pkg.capi
    p = ms.box_cloud(64, (1.0, 2.0, 3.0), 21)
    b = Batch(pkg, ctx, dev, [(p, np.zeros_like(p))], [np.zeros((0, 3), np.float32)], 0.1)
    try:
        L = capi.lib()
        obj = torch.zeros(1, dtype=torch.int32, device=dev)
        cen = torch.zeros(3, dtype=torch.float32, device=dev)
        rad = torch.full((1,), -1.0, dtype=torch.float32, device=dev)
        f = lambda k: torch.empty(k, dtype=torch.float32, device=dev)
        n_sel, c, s, a = torch.empty(1, dtype=torch.int32, device=dev), f(3), f(3), f(9)
        P, null = capi._p, C.c_void_p(0)
        good = [ctx._h, b.cloud._h, C.c_int(1), P(obj), P(cen), P(rad), P(n_sel), P(c), P(s), P(a), null, null]
        for k in (1, 3, 4, 5, 6, 7, 8, 9):
            bad = list(good)
            bad[k] = null
            assert L.ismhip_region_mvbb(*bad) != 0, k
            assert b"region_mvbb" in L.ismhip_last_error(ctx._h)
        bad = list(good)
        bad[2] = C.c_int(-1)
        assert L.ismhip_region_mvbb(*bad) != 0
        assert L.ismhip_region_mvbb(null, *good[1:]) != 0
        none = list(good)
        none[2] = C.c_int(0)
        for k in range(3, 10):
            none[k] = null
        assert L.ismhip_region_mvbb(*none) == 0                 # no region: nothing is read or written
        assert L.ismhip_region_mvbb(*good) == 0
        ctx.sync()
        assert int(n_sel.cpu()[0]) == 64 and 0 < np.prod(s.cpu().numpy().astype(np.float64)) <= np.prod(np.ptp(p, axis=0).astype(np.float64)) * (1 + 1e-6)
    finally:
        b.close()

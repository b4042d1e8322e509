"""Routes of the C++ host (libism3d_amd.so) that no other test drives: colour through every point-array path (pre-filters -> device
normals -> ismhip_filter_normals with rgba), a batch that mixes clouds with and without normals, and Threshold activation with the
RANSAC vote filter (ismhip_vote_keypoints_csr)."""
import json

import numpy as np
import pytest

import host_binding as hb
import prefilter_ref as ref
from test_gpu_prefilter import FILTER_SETS
from test_gpu_ransac import _host_counter
from test_host_layer import _cfg
from test_threshold_host import _last_features, _last_votes, _threshold_cfg

pytestmark = pytest.mark.gpu


def _split(pkg, with_color=False):
    syn = pkg.synthetic
    train = syn.Dataset(3, 9, split=0, n_points=4096, leaf=0.2, with_color=with_color)
    test = syn.Dataset(3, 6, split=1, n_points=4096, leaf=0.2, with_color=with_color)
    return train, test, sorted(range(9), key=lambda i: (train.label(i), i))


def _trained(cfg, train, order, with_color=False):
    m = hb.Model()
    m.config_from_json(cfg)
    for i in order:
        o = train.get(i)
        m.add_training(o["xyz"], o["normals"], o["label"], i, rgba=o["rgba"] if with_color else None)
    m.train()
    return m


def _assert_maxima_close(got, want, n_obj):
    """the tolerances of test_host_detect_with_filters_equals_detect_on_filtered_clouds"""
    assert np.array_equal(got["n"], want["n"]) and (got["n"] > 0).any()
    for o in range(n_obj):
        k = int(got["n"][o])
        assert np.array_equal(got["cls"][o, :k], want["cls"][o, :k])
        assert np.allclose(got["weight"][o, :k], want["weight"][o, :k], rtol=1e-5, atol=1e-7)
        assert np.allclose(got["pos"][o, :k], want["pos"][o, :k], rtol=0, atol=1e-5)


def _dirty_coloured(ds, indices, seed):
    """test_gpu_prefilter._dirty with colours: 3 % uniform outliers of random colour shuffled in between the points of every object"""
    rng = np.random.default_rng(seed)
    crng = np.random.default_rng(seed + 1)                           # colours from a stream of their own: the geometry is _dirty's
    out = []
    for i in indices:
        o = ds.get(i)
        n_out = int(0.03 * len(o["xyz"]))
        p = np.concatenate([o["xyz"], rng.uniform(-1.2, 1.2, size=(n_out, 3))]).astype(np.float32)
        rng.normal(size=(n_out, 3))                                  # (_dirty draws the outliers' normals here)
        c = np.concatenate([o["rgba"], crng.integers(0, 1 << 24, n_out).astype(np.uint32)])
        perm = rng.permutation(len(p))
        out.append((p[perm], c[perm]))
    return out


def _cat_coloured(objs):
    po = np.zeros(len(objs) + 1, np.uint32); po[1:] = np.cumsum([len(o[0]) for o in objs])
    xyz = np.concatenate([o[0] for o in objs])
    return po, xyz, np.zeros_like(xyz), np.concatenate([o[1] for o in objs])


def test_colour_through_prefilters_and_device_normals(pkg, gpu, tmp_path, monkeypatch):
    """A CSHOT model detects coloured, contaminated clouds that carry no normals, with SOR + ROR + z cut-off enabled: the rgba array
    goes through the upload, three compactions, the device normals and ismhip_filter_normals. The same maxima come out with the
    NaN-normal filter on the host, and the same features (bitwise) and maxima when the clouds were filtered beforehand.
    (On this small split few CSHOT activations carry a vote: without input normals some objects end with no valid vote slot and
    therefore no maximum, in all three detections alike, so the maxima check asks for equal counts and for some maxima, not for a
    maximum per object.)"""
    train, test, order = _split(pkg, with_color=True)
    m = _trained(_cfg(**{"Children/Features/Type": "CSHOT", "Parameters/NormalRadius": 0.15}), train, order, with_color=True)
    path = str(tmp_path / "cshot.ism")
    m.write(path)
    m.close()
    saved = json.load(open(path))
    params = FILTER_SETS[2]
    saved["ObjectConfig"]["Parameters"].update(params)
    p_on = str(tmp_path / "cshot_filters.ism")
    json.dump(saved, open(p_on, "w"))
    dirty = _dirty_coloured(test, range(6), 21)
    po, xyz, zeros, rgba = _cat_coloured(dirty)
    on = hb.Model()
    on.read(p_on)
    got = on.detect_batch(po, xyz, zeros, max_maxima=8, rgba=rgba)
    f_on = _last_features(on, 1)
    monkeypatch.setenv("ISM3D_HOST_NORMAL_FILTER", "1")
    via_host = on.detect_batch(po, xyz, zeros, max_maxima=8, rgba=rgba)
    monkeypatch.delenv("ISM3D_HOST_NORMAL_FILTER")
    on.close()
    for k in ("cls", "weight", "pos"):
        np.testing.assert_array_equal(got[k], via_host[k])
    clean = []
    for p, c in dirty:
        idx = ref.prefilter(p, use_sor=True, mean_k=params["OutlierRemovalMeanK"], stddev_mul=params["OutlierRemovalStddevMul"], use_ror=True,
                            radius=params["OutlierRemovalRadius"], min_neighbors=params["OutlierRemovalMinNeighbors"],
                            cutoff_z=params["CutoffDistanceZAxis"])
        clean.append((p[idx], c[idx]))
    assert all(0 < len(c[0]) < len(d[0]) for c, d in zip(clean, dirty))
    plain = hb.Model()
    plain.read(path)
    po_c, xyz_c, zeros_c, rgba_c = _cat_coloured(clean)
    want = plain.detect_batch(po_c, xyz_c, zeros_c, max_maxima=8, rgba=rgba_c)
    f_off = _last_features(plain, 1)
    plain.close()
    assert f_on["desc"].shape[1] == 1344 and len(f_on["off"]) == 7 and np.diff(f_on["off"].astype(np.int64)).min() >= 1
    assert np.array_equal(f_on["off"], f_off["off"])
    for key in ("desc", "lrf", "kp"):
        assert np.array_equal(f_on[key].view(np.uint32), f_off[key].view(np.uint32)), key
    _assert_maxima_close(got, want, 6)


def test_batch_that_mixes_clouds_with_and_without_normals(pkg, gpu, monkeypatch):
    """Objects 1 and 4 of six come without normals: theirs are estimated on the device, filtered on the host and uploaded with the
    rest. Every object's features are, bitwise, those it gets in a batch of its own kind (all with normals; all without, with the
    NaN-normal filter on the host as in the mixed route), and so are its maxima."""
    train, test, order = _split(pkg)
    m = _trained(_cfg(**{"Parameters/NormalRadius": 0.15}), train, order)
    nb = test.batch(range(6))
    po = nb["pt_off"]
    without = (1, 4)
    mixed_nrm = nb["normals"].copy()
    for o in without:
        mixed_nrm[po[o]:po[o + 1]] = 0
    got = m.detect_batch(po, nb["xyz"], mixed_nrm, max_maxima=8)
    f_mix = _last_features(m, 1)
    with_all = m.detect_batch(po, nb["xyz"], nb["normals"], max_maxima=8)
    f_with = _last_features(m, 1)
    monkeypatch.setenv("ISM3D_HOST_NORMAL_FILTER", "1")
    without_all = m.detect_batch(po, nb["xyz"], np.zeros_like(nb["normals"]), max_maxima=8)
    monkeypatch.delenv("ISM3D_HOST_NORMAL_FILTER")
    f_without = _last_features(m, 1)
    m.close()
    assert len(f_mix["off"]) == 7
    for o in range(6):
        f_pure, pure = (f_without, without_all) if o in without else (f_with, with_all)
        a, b = int(f_mix["off"][o]), int(f_mix["off"][o + 1])
        c, d = int(f_pure["off"][o]), int(f_pure["off"][o + 1])
        assert b - a == d - c > 0, o
        for key in ("desc", "lrf", "kp"):
            assert np.array_equal(f_mix[key][a:b].view(np.uint32), f_pure[key][c:d].view(np.uint32)), (o, key)
        k = int(got["n"][o])
        assert k == pure["n"][o] and k > 0
        assert np.array_equal(got["cls"][o, :k], pure["cls"][o, :k])
        assert np.allclose(got["weight"][o, :k], pure["weight"][o, :k], rtol=1e-5, atol=1e-7)
        assert np.allclose(got["pos"][o, :k], pure["pos"][o, :k], rtol=0, atol=1e-5)
    # the two kinds really differ: estimated normals are not the objects' own
    assert not np.array_equal(f_with["desc"][f_with["off"][1]:f_with["off"][2]], f_mix["desc"][f_mix["off"][1]:f_mix["off"][2]])


def test_host_threshold_with_ransac_vote_filtering(pkg, gpu):
    """Threshold activation with Voting.RansacVoteFiltering through the host (the list path's vote keypoints) against a rebuild
    through the C ABI on the host's own detection features: knn_threshold -> cast_votes_csr -> vote_keypoints_csr ->
    find_maxima(ransac=...). Vote-slot ranges and votes bitwise, maxima to the tolerances of
    test_host_and_python_harness_agree_with_ransac_vote_filtering."""
    import torch
    capi = pkg.capi
    ctx, dev = gpu
    train, test, order = _split(pkg)

    def cfg(thr):
        j = json.loads(_threshold_cfg(thr))
        j["Children"]["Voting"]["Parameters"]["RansacVoteFiltering"] = True
        return json.dumps(j)

    # the threshold of test_host_threshold_train_and_detect: a few activations per training feature
    m0 = _trained(cfg(0.25), train, order)
    tf = _last_features(m0, 0)
    m0.close()
    d = torch.as_tensor(tf["desc"]).to(dev)
    d2 = ((d * d).sum(1, keepdim=True) - 2 * d @ d.T + (d * d).sum(1)[None, :]).cpu().numpy()
    thr = float(np.quantile(d2, 6.0 / len(d2)))
    m = _trained(cfg(thr), train, order)
    cb = m.codebook_all()
    nb = test.batch(range(6))
    got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=32)
    df = _last_features(m, 1)
    votes = _last_votes(m, 6)
    clusters = _host_counter(m, "ransac_clusters")
    m.close()
    assert clusters > 0                                              # the filter really ran
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    dcb = capi.Codebook(ctx, cb["words"], cb["vote_offsets"], cb["vote_xyz"], cb["vote_class"], cb["vote_instance"], 3, cb["class_sigma"],
                        word_weight=cb["word_weight"], vote_weight=cb["vote_weight"], vote_class_weight=cb["vote_class_weight"],
                        vote_bbox_quat=cb["vote_bbox_quat"], vote_bbox_size=cb["vote_bbox_size"])
    dcb.set_word_class(cb["word_class"])
    dcb.set_word_keypoint(cb["word_keypoint"])
    off_d, idx_d, dist_d = capi.knn_threshold(ctx, dcb, 0, T(df["desc"]), thr)
    assert len(np.unique(np.diff(off_d))) > 2                        # a genuinely variable fan-out
    kq = [T(df["kp"][:, i]) for i in range(3)]
    mine = capi.cast_votes_csr(ctx, dcb, 0, T(df["lrf"]), kq[0], kq[1], kq[2], off_d, idx_d, dist_d, want_bbox=True)
    vkp, vkpt = capi.vote_keypoints_csr(ctx, dcb, kq[0], kq[1], kq[2], off_d, idx_d)
    slot_off = (off_d[df["off"].astype(np.int64)] * dcb.max_votes).astype(np.uint32)
    assert np.array_equal(votes["slot_off"], slot_off)
    for k in ("cls", "inst", "weight", "pos"):
        assert np.array_equal(votes[k], mine[k].cpu().numpy()), k
    # Voting of the shipped config: MeanShift, Bandwidth 0.6, single-object mode "None"; RansacInlierThreshold at its default 0.1
    want = capi.find_maxima(ctx, slot_off, mine, 3, 0.6, max_maxima=32, ransac=dict(vote_keypoint=vkp, vote_keypoint_training=vkpt, inlier_threshold=0.1))
    ctx.sync()
    dcb.close()
    wn = want["n"].cpu().numpy()
    assert wn.max() < 32 and (wn > 0).all()                          # (the host asks again with more room only when an object fills all 32)
    assert np.array_equal(got["n_total"], wn), (got["n_total"], wn)
    for o in range(6):
        k = int(wn[o])
        assert np.array_equal(got["cls"][o, :k], want["cls"][o, :k].cpu().numpy())
        np.testing.assert_allclose(got["weight"][o, :k], want["weight"][o, :k].cpu().numpy(), atol=1e-4)
        assert np.array_equal(got["n_votes"][o, :k], want["n_votes"][o, :k].cpu().numpy())

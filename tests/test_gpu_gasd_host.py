"""Global verification with GlobalFeatures type "GASD" through the C++ host (-m gpu): three classes x two objects of 2 048 points
trained (GasdWithColor false: the training set has no colours), written, read back, then detectBatch in single-object and in detection
mode with two merge functions. As test_gpu_global_host.py does for the other types: what the host returns must equal global_ref.py's
host sequence applied to the DEVICE's own maxima, rows and neighbours. The stored rows are those of ismhip_global_gasd on the same
objects up to a few deposits, with a zero frame. One coloured training gives 984-float rows; an uncoloured cloud is refused there."""
import json

import numpy as np
import pytest

import gasd_ref as ga
import global_host as gh
import host_binding as hb
from test_gpu_global_host import N_CLASSES, N_POINTS, N_TEST, N_TRAIN, check_against_the_restatement, config

pytestmark = pytest.mark.gpu
GASD = {"Type": "GASD", "Parameters": {"GasdWithColor": True}}
GASD_SHAPE = {"Type": "GASD", "Parameters": {"GasdWithColor": False}}
_state = {}


def trained(pkg, tmp_path_factory, colour=False):
    """train once per setting, write the model -> (directory, training order, train set, test batch, stored rows)"""
    if colour not in _state:
        syn = pkg.synthetic
        train = syn.Dataset(N_CLASSES, N_TRAIN, split=0, n_points=N_POINTS, leaf=0.2, with_color=colour)
        test = syn.Dataset(N_CLASSES, N_TEST, split=1, n_points=N_POINTS, leaf=0.2, with_color=colour)
        order = sorted(range(N_TRAIN), key=lambda i: (train.label(i), i))
        m = hb.Model()
        m.config_from_json(json.dumps(config(GASD if colour else GASD_SHAPE)))
        for i in order:
            o = train.get(i)
            m.add_training(o["xyz"], o["normals"], o["label"], i, rgba=o.get("rgba"))
        m.train()
        d = tmp_path_factory.mktemp("global_gasd_%d" % int(colour))
        m.write(str(d / "model.ism"))
        _state[colour] = (d, order, train, test.batch(range(N_TEST)), gh.global_features(m))
    return _state[colour]


def variant(d, name, child=GASD_SHAPE, **voting):
    """the written model under other Voting parameters: a second .ism beside the same .ismd"""
    path = str(d / (name + ".ism"))
    open(path, "w").write(json.dumps({"ObjectConfig": config(child, **voting), "ObjectData": "model.ismd"}))
    m = hb.Model()
    m.read(path)
    return m


def device_rows(pkg, gpu, train, order, colour):
    import torch
    ctx, dev = gpu
    b = train.batch(order)
    t = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (b["xyz"], b["normals"]) for i in range(3)]
    rgba = torch.as_tensor(b["rgba"].astype(np.int64), dtype=torch.int32).to(dev) if colour else None
    cloud = pkg.capi.Cloud(ctx, b["pt_off"], *t, 0.16, rgba=rgba)
    try:
        out = pkg.capi.global_gasd(ctx, cloud, dev, np.arange(N_TRAIN), with_color=colour, want_counts=True)
        return {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        cloud.close()


@pytest.mark.parametrize("colour", [False, True], ids=["shape-512", "colour-984"])
def test_training_stores_one_gasd_row_per_cloud_and_the_data_file_keeps_it(pkg, gpu, tmp_path_factory, colour):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory, colour)
    dim = 984 if colour else 512
    assert stored["n_clouds"] == N_TRAIN and stored["cls"].tolist() == [train.label(i) for i in order] and stored["inst"].tolist() == order
    assert stored["desc"].shape == (N_TRAIN, dim) and np.isfinite(stored["desc"]).all() and (stored["radius"] > 0).all()
    assert (stored["rf"] == 0).all()                                                  # the reference leaves the frame of this type untouched
    if not colour:
        assert (stored["desc"][:, 216:] == 0).all()
    out = device_rows(pkg, gpu, train, order, colour)
    assert np.array_equal(out["radius"], stored["radius"])
    # the host's cloud has another cell size, so its sorted order and with it the last bits of the covariance sums, of the frame and of
    # max_coord may differ: a deposit within ~1e-6 cells of a face may fall either way. One deposit moves a bin by 100 / (n - 1); as for
    # VFH, allow three of 2 048 per row (each point deposits once per block; a face is met with probability ~1e-5 per point)
    assert np.abs(out["desc"] - stored["desc"]).max() <= 3 * 100.0 / (N_POINTS - 1) + 1e-4
    for r in range(N_TRAIN):
        assert np.array_equal(out["desc"][r], ga.row_of_counts(out["counts"][r], int(out["n_sel"][r]), with_color=colour))
    again = gh.global_features(variant(d, "reread", GASD if colour else GASD_SHAPE))
    for k in ("cls", "cloud", "inst", "rf", "desc", "radius"):
        assert np.array_equal(again[k], stored[k]), k
    if colour:                                                                        # an uncoloured cloud under GasdWithColor: refused
        m = variant(d, "refuse", GASD, SingleObjectMode=True)
        with pytest.raises(hb.HostError, match="GASD needs coloured point clouds"):
            m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=16)
        got = m.detect_batch(nb["pt_off"], nb["xyz"], nb["normals"], max_maxima=16, rgba=nb["rgba"])
        g = gh.last_global(m)
        assert g["dim"] == 984 and np.isfinite(g["desc"]).all() and (got["n"] >= 1).all()


@pytest.mark.parametrize("single", [True, False], ids=["single-object", "detection"])
@pytest.mark.parametrize("fn", [3, 7])
def test_detect_batch_matches_the_host_sequence(pkg, gpu, tmp_path_factory, fn, single):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory)
    m = variant(d, f"gasd_fn{fn}_{int(single)}", GlobalFeatureInfluenceType=fn, SingleObjectMode=single, GlobalFeatureMinPoints=50)
    got, g = check_against_the_restatement(m, nb, stored, fn, single, min_points=50)
    n_obj = len(nb["pt_off"]) - 1
    assert g["k"] == 3 and g["dim"] == 512
    if single:
        assert g["region_obj"].tolist() == list(range(n_obj)) and (g["region_max"] == -1).all()
        assert np.array_equal(g["n_sel"], np.diff(nb["pt_off"]))
        assert np.isfinite(g["desc"]).all() and (g["desc"][:, 216:] == 0).all()
    else:
        assert len(g["region_obj"]) == int(g["max_off"][-1]) and (g["region_max"] >= 0).all()
    assert (got["n"] >= 1).all()

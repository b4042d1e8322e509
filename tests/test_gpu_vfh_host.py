"""Global verification with GlobalFeatures type "VFH" through the C++ host (-m gpu): three classes x two objects of 2 048 points
trained, written, read back, then detectBatch in single-object and in detection mode with two merge functions. As test_gpu_global_host.py
does for the other two types: what the host returns must equal global_ref.py's host sequence applied to the DEVICE's own maxima, rows and
neighbours. The stored rows are those of ismhip_global_vfh on the same objects, bit for bit (no frame stands between the cloud and the
row), with a zero frame."""
import numpy as np
import pytest

import global_host as gh
import vfh_ref as vr
from test_gpu_global_host import N_TRAIN, check_against_the_restatement, trained, variant

pytestmark = pytest.mark.gpu


def test_training_stores_one_vfh_row_per_cloud_and_the_data_file_keeps_it(pkg, gpu, tmp_path_factory):
    ctx, dev = gpu
    d, order, train, nb, stored = trained(pkg, tmp_path_factory, "VFH")
    assert stored["n_clouds"] == N_TRAIN and stored["cls"].tolist() == [train.label(i) for i in order] and stored["inst"].tolist() == order
    assert stored["desc"].shape == (N_TRAIN, 308) and np.isfinite(stored["desc"]).all() and (stored["radius"] > 0).all()
    assert (stored["rf"] == 0).all()                                                  # VFH has no frame
    assert (stored["desc"][:, 135:180] == 0).all()                                    # the size component is off
    import torch
    b = train.batch(order)
    t = [torch.as_tensor(np.ascontiguousarray(a[:, i])).to(dev) for a in (b["xyz"], b["normals"]) for i in range(3)]
    cloud = pkg.capi.Cloud(ctx, b["pt_off"], *t, 0.16)
    try:
        out = pkg.capi.global_vfh(ctx, cloud, dev, np.arange(N_TRAIN), want_counts=True)
        assert np.array_equal(out["radius"].cpu().numpy(), stored["radius"])
        counts, desc = out["counts"].cpu().numpy(), out["desc"].cpu().numpy()
        # the host's cloud has another cell size, so its sorted order and the last bits of nc may differ: a deposit on a bin edge may
        # fall either way. One deposit moves a bin by 100 / (m - 1); allow three of 2 048 per row
        assert np.abs(desc - stored["desc"]).max() <= 3 * 100.0 / 2047 + 1e-4
        for r in range(N_TRAIN):
            m = int(counts[r, 180:].sum())
            assert np.array_equal(desc[r], vr.row_of_counts(counts[r], m))
    finally:
        cloud.close()
    again = gh.global_features(variant(d, "reread", "VFH"))
    for k in ("cls", "cloud", "inst", "rf", "desc", "radius"):
        assert np.array_equal(again[k], stored[k]), k


@pytest.mark.parametrize("single", [True, False], ids=["single-object", "detection"])
@pytest.mark.parametrize("fn", [3, 7])
def test_detect_batch_matches_the_host_sequence(pkg, gpu, tmp_path_factory, fn, single):
    d, order, train, nb, stored = trained(pkg, tmp_path_factory, "VFH")
    m = variant(d, f"vfh_fn{fn}_{int(single)}", "VFH", GlobalFeatureInfluenceType=fn, SingleObjectMode=single, GlobalFeatureMinPoints=50)
    got, g = check_against_the_restatement(m, nb, stored, fn, single, min_points=50)
    n_obj = len(nb["pt_off"]) - 1
    assert g["k"] == 3 and g["dim"] == 308
    if single:
        assert g["region_obj"].tolist() == list(range(n_obj)) and (g["region_max"] == -1).all()
        assert np.array_equal(g["n_sel"], np.diff(nb["pt_off"]))
        assert np.isfinite(g["desc"]).all() and (g["desc"][:, 135:180] == 0).all()
    else:
        assert len(g["region_obj"]) == int(g["max_off"][-1]) and (g["region_max"] >= 0).all()
    assert (got["n"] >= 1).all()

"""The wide ragged batch of batch_scenes.py proves on the host, by the modules' own restatements alone, that it reaches what the device
tests (test_gpu_feature_batch.py, test_gpu_keypoint_batch.py) use it for: the XCD-local block map with padding blocks and a unique longest
keypoint run, all-NaN, all-zero and finite rows of every Features type that can produce them, keypoints that only their frame drops,
per-object maxima that differ, and inputs on which no restatement leaves a keypoint or a point to the last bit.

Decidedness is a condition on the INPUTS, asserted here. Where a restatement's criterion cannot reach zero on a generic surface the cap is
the one the type's own scene test asserts, and the share is printed:
    FPFH       fpfh_ref.py calls a pair that reads a NaN normal degenerate and its keypoint exempt: the one keypoint of `holes` placed beside
               the NaN normals is exempt BY CONSTRUCTION and no other (test_gpu_fpfh.py: the exempt keypoints are exactly the planted ones;
               their rows are held to the oracle). Undecided deposits are not exemptions: the interval carries them, and on the rows that
               are neither NaN nor exempt they stay within test_fpfh_cpu.py's caps: at most 2 % of the deposits undecided, and one wrong
               pair moves a row by at least four tolerances (min_move).
    SHORT_*    no raw value within 1e-9 of a switch of its cast, no float32 fraction within 1e-9 of 0.5 unless exactly on it
               (test_short_shot_cpu.py, test_short_cshot_cpu.py); a keypoint that misses either counts as undecided
    CoSPAIR    at least 90 % of the rows fully decided, at most 8 undecided deposits in a row (test_cospair_cpu.py); the intervals carry them
    RSD        at most 1 % of the pairs undecided (test_rsd_cpu.py); the intervals carry them
    BSHOT      at most 30 % of the non-zero groups inside the 4e-4 margin (test_gpu_bshot.py)
    SIFT3D     at most 2 % of the extremum tests undecided (test_gpu_sift3d.py); here only the isolated point, whose three columns are 0 = 0
Every other criterion is at zero."""
import numpy as np
import pytest

import batch_scenes as bs
from test_fpfh_cpu import TOL as FPFH_TOL

CAN_BE_NAN = set(bs.TYPES) - {"BSHOT"}                                    # a NaN SHOT row becomes 352 ones
CAN_BE_ZERO = {"FPFH", "CoSPAIR", "SpinImage", "RSD", "RIFT"}             # SHOT, SHORT_*: 0 / 0 = NaN; CGF: the bias; ESF_LOCAL: sums to 1 or NaN
FRAME_FREE = ("FPFH", "CoSPAIR", "SpinImage", "RSD", "RIFT", "ESF_LOCAL")   # no frame enters the descriptor


def test_the_batch_is_wide_ragged_and_has_padding_blocks():
    b = bs.batch()
    n_obj = len(b["pt_off"]) - 1
    runs = np.diff(b["kp_off"].astype(np.int64))
    sizes = np.diff(b["pt_off"].astype(np.int64))
    print("points", sizes.tolist(), "keypoints", runs.tolist())
    assert n_obj == bs.N_OBJ >= 9 and n_obj % 8 != 0
    assert runs.max() == 13 and (runs == runs.max()).sum() == 1 and runs.max() % 4 != 0
    assert sizes.max() <= 900 and runs.tolist() == [13, 2, 3, 1, 4, 0, 1, 6, 2, 7, 5]
    assert sizes[[bs.obj(n) for n in ("empty", "all_nan", "one_point", "four_points", "holes", "p65")]].tolist() == [0, 3, 1, 4, 257, 65]
    ps, _ = bs.objects()[bs.obj("all_nan")]
    assert np.isnan(b["xyz"][ps]).all()
    ps, ks = bs.objects()[bs.obj("holes")]
    assert np.isnan(b["normals"][ps]).any(1).sum() == 5 and np.isnan(b["xyz"][ps]).any(1).sum() == 1 and np.isposinf(b["xyz"][ps]).any(1).sum() == 1
    _, ks = bs.objects()[bs.obj("off_cloud")]
    assert (~np.isfinite(b["kp"][ks]).all(1)).sum() == 1 and (np.abs(b["kp"][ks][:, 0]) > 20).sum() == 1
    nrm = np.linalg.norm(b["normals"].astype(np.float64), axis=1)
    ps, _ = bs.objects()[bs.obj("no_kp")]
    unit = np.ones(len(nrm), bool); unit[ps] = False
    assert np.allclose(nrm[unit & np.isfinite(nrm)], 1.0, atol=1e-6) and np.allclose(nrm[ps], 3.0, atol=1e-5)
    # keypoints: cloud points and points next to the cloud, both
    on = np.array([(b["xyz"][ps] == q).all(1).any() for (ps, ks) in bs.objects() for q in b["kp"][ks]])
    assert on.sum() >= 25 and (~on).sum() >= 10
    one = bs.single(bs.obj("p65"))
    assert one["pt_off"].tolist() == [0, 65] and one["kp_off"].tolist() == [0, 7] and len(one["rgba"]) == 65


def test_frames_are_decided_and_some_keypoints_lose_to_the_frame_only(ora):
    fr = bs.frames()
    nan = np.isnan(fr["frame"]).any(1)
    assert np.array_equal(nan, np.isnan(fr["frame"]).all(1)) and fr["decided"].all()
    assert (fr["gap"][~nan] >= 1e-3).all()                               # what test_gpu_shotna.assert_matches_restatement asks of a scene
    print("frames: %d keypoints, %d without a frame, undecided share %.3f" % (len(nan), nan.sum(), 1.0 - fr["decided"].mean()))
    a, b = bs.kp_range("four_points")
    assert nan[a:b].all() and (fr["valid"][a:b] < 5).all()
    for T in FRAME_FREE:
        rows = bs.answer(T, rgb2lab=ora.rgb2lab)["rows"]
        only = nan & ~np.isnan(rows).any(1)
        print("%s: keypoints dropped for their frame only: %s" % (T, np.nonzero(only)[0].tolist()))
        assert only[a:b].all()


@pytest.mark.parametrize("T", bs.TYPES)
def test_restatement_rows_are_decided_and_nan_as_a_whole(ora, T):
    a = bs.answer(T, rgb2lab=ora.rgb2lab)
    rows = np.asarray(a["rows"])
    K = len(bs.batch()["kp"])
    assert rows.shape[0] == K == 44
    nan, zero, fin = bs.special_rows(T, a)
    und = a["undecided"]
    share = float(und.mean())
    print("%s: dim %d, undecided share %.4f, NaN rows %d, zero rows %d, finite rows %d" % (T, rows.shape[1], share, nan.sum(), zero.sum(), fin.sum()))
    # the whole-row rule, in the float64 reference itself
    assert np.array_equal(np.isnan(rows).any(1), np.isnan(rows).all(1))
    assert not np.isinf(rows).any()
    assert fin.sum() >= 20
    assert (nan.sum() >= 1) == (T in CAN_BE_NAN)
    assert (zero.sum() >= 1) == (T in CAN_BE_ZERO)
    if T == "FPFH":
        planted = bs.kp_range("holes")[0] + bs.HOLES_NEAR
        assert np.nonzero(und)[0].tolist() == [planted]
        r = a["ref"]
        ok = ~r.nan & ~r.exempt                                           # the rows the device is held to the intervals on
        print("    undecided deposits per category %s of %d, smallest min_move %.3g on %d rows" %
              (r.undecided[ok].sum(0).tolist(), r.deposits[ok].sum(), r.min_move[ok].min(), ok.sum()))
        assert r.undecided[ok].sum() <= 0.02 * r.deposits[ok].sum()       # test_fpfh_cpu.test_generic_scene_has_power
        assert (FPFH_TOL <= r.min_move[ok] / 4).all()                     # test_fpfh_cpu.test_one_wrong_pair_is_four_tolerances
    else:
        assert share == 0.0
    if T == "BSHOT":
        assert not np.isnan(rows).any() and set(np.unique(rows)) <= {0.0, 1.0}
        shot_nan = np.isnan(a["shot"][:, 0])
        assert shot_nan.sum() >= 1 and (rows[shot_nan] == 1).all()
        live = ~shot_nan
        s = a["shot"][live].reshape(live.sum(), -1, 4).sum(2)
        left_out = (~a["groups_decided"][live]).sum() / max((s != 0).sum(), 1)
        print("    groups inside the margin: %.3f of the non-zero ones" % left_out)
        assert left_out <= 0.30
    if T == "CoSPAIR":
        r = a["ref"]
        live = ~r.nan
        print("    rows fully decided %.3f, at most %d undecided deposits in a row" % (r.decided_row[live].mean(), r.undecided.max()))
        assert r.decided_row[live].mean() >= 0.9 and r.undecided.max() <= 8
    if T == "RSD":
        r = a["ref"]
        print("    undecided pairs %d of %d" % (r["undecided"].sum(), r["pairs"].sum()))
        assert r["undecided"].sum() <= 0.01 * r["pairs"].sum()
    if T in ("SHORT_SHOT", "SHORT_CSHOT"):
        print("    smallest switch margin %.3g" % a["switch"].min())
        assert a["switch"].min() >= bs.SWITCH_MARGIN                      # test_short_shot_cpu.py, test_short_cshot_cpu.py
    if T == "SHORT_SHOT":
        print("    smallest frac margin %.3g" % a["frac"].min())
        assert ((a["frac"] == 0.0) | (a["frac"] >= bs.SWITCH_MARGIN)).all()
    if T == "CGF":
        empty = (a["ball"] == 0) & np.isfinite(bs.batch()["kp"]).all(1)
        assert not a["raw"][empty].any() and empty.sum() >= 2                               # an empty ball is a raw row of zeros, never NaN
        assert np.isnan(a["raw"][~np.isfinite(bs.batch()["kp"]).all(1)]).all()               # only a keypoint that is not finite is


def test_rift_gradients_are_decided_and_zero_on_the_one_colour_object():
    und = np.concatenate([bs.rift_gradients(o)["undecided"] for o in range(bs.N_OBJ)])
    print("RIFT gradients: %d points, undecided share %.4f" % (len(und), und.mean()))
    assert not und.any()
    g = bs.rift_gradients(bs.obj("four_points"))["grad"]
    assert g.shape == (4, 3) and not g.any()


def test_per_object_maxima_differ():
    m = bs.object_maxima()
    for name, v in m.items():
        exps = sorted({int(np.frexp(x)[1]) if x > 0 else None for x in v}, key=lambda e: (e is not None, e))
        print("%s: %s -> %d different, exponents %s" % (name, np.array2string(v, precision=4), len(set(v.tolist())), exps))
        assert len(set(v.tolist())) >= 3
        assert len(exps) >= 3                                             # zero, and two powers of two apart: another object's maximum moves the fixed point


def test_detectors_and_cloud_passes_are_decided(ora):
    keep = []
    for o in range(bs.N_OBJ):
        a = bs.iss3d_answer(o)
        assert not a["undecided"].any() and not a["undecided_saliency"].any(), o
        keep.append(int(a["keep"].sum()))
    print("ISS3D keypoints per object", keep)
    assert keep[bs.obj("empty")] == keep[bs.obj("all_nan")] == 0 and keep[bs.obj("longest")] > 0 and keep[bs.obj("holes")] > 0 and keep[bs.obj("small5")] > 0
    kept, n_kp = [], []
    for o in range(bs.N_OBJ):
        c = bs.culling_answer(o, ora.rgb2lab)
        assert not c["curvature"]["undecided"].any() and not c["kpq"]["undecided"].any(), o
        kept.append(int(c["select"]["keep"].sum())); n_kp.append(len(c["select"]["keep"]))
    print("VoxelGridCulling: voxel keypoints per object", n_kp, "kept", kept)
    assert kept[bs.obj("empty")] == kept[bs.obj("all_nan")] == 0 and kept[bs.obj("longest")] > 0 and kept[bs.obj("small5")] > 0
    und = size = 0
    flags = []
    for o in range(bs.N_OBJ):
        s = bs.sift3d_answer(o)
        inner = s["undecided"][:, 1:-1]
        assert not inner[s["count"] != 1].any(), o                        # only an isolated point's 0 = 0 comparisons
        und += int(inner.sum()); size += inner.size
        flags.append(int((s["flags"] > 0).sum()))
    print("SIFT3D: extrema per object %s, undecided share %.5f" % (flags, und / size))
    assert und / size <= 0.02 and und == 3 and flags[bs.obj("longest")] > 0

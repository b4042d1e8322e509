"""Codebook training (train.hip: Codebook::activate after the activation step) and vote casting (k_cast_votes in codebook.hip)
against the float64 references of codebook_ref.py on the scenes of codebook_scenes.py (-m gpu). test_codebook_cpu.py proves the
references, the tolerances and the scenes first.

Integer outputs are equal. vote_weight, vote_xyz, cast positions and class sigma^2 lie within TOL_W, TOL_XYZ, TOL_POS, TOL_SIGMA of
float64 (4 x what the float32 oracle measures), while a median rank off by one moves a weight of `ranks` by >= 175 TOL_W and a
sampled one of `hub` by >= 10 TOL_W. The class weights are bit-equal to the numpy float32 restatement, sigma^2 to the oracle's
sequential float32 sums; -0.0 and NaN are compared by sign and kind; frames with a dyadic quaternion give exact votes; boundary
votes are kept or dropped as the reference says; the bbox quaternion of a live vote under every signed permutation pins the SIGN of
rot_quaternion (strict `trace > 0`, diagonal ties to i = 0); refusals raise and leave the context usable.

Measured on the MI355X (largest |device - float64| per scene, as a share of the tolerance):
  scene            weights            votes              sigma^2 (relative)
  ranks            1.09e-07 (0.19)    7.45e-09 (0.01)    0                   6601 medians, all compared
  ties             6.64e-09 (0.01)    0                  2.14e-06 (0.02)     the tied values, 0.0f and 1.0f exactly
  hub              1.10e-07 (0.20)    7.45e-09 (0.01)    0                   257 of 32768 medians compared
  frames           7.99e-08 (0.14)    2.12e-07 (0.23)    3.08e-06 (0.03)     12 exact frames give exact votes, no undecided frame
  term3, cleanup   1.41e-08 (0.03)    3.73e-09 (0.00)    3.67e-08 (0.00)
  sigma-* (13)     1.39e-07 (0.25)    1.19e-07 (0.13)    2.93e-05 (0.24, l2-352; chi2-352 1.06e-05, l2-1344 6.48e-06)
  csr-* (4)        9.33e-08 (0.17)    2.30e-07 (0.25)    1.67e-07 (0.00)
  votes_edges      positions 1.16e-07 (0.25 TOL_POS) at each of the 16 flag values; 79 to 81 live of 168 slots; weights: the same bytes
These are the figures test_codebook_cpu.py measures for the CPU oracle: the device evaluates the oracle's float32 sequence.
The hub scene is the longest device call, 0.07 s; its test takes 0.8 s with the reference of its 257 sampled medians, the test
of ranks 0.9 s with the reference of all 6601, every other test below 0.1 s. The suite found no defect in train.hip or codebook.hip.

Scratch builds of the library, each run against this module (41 tests):
  `m >= TR_MAXM` in k_tr_weights alone            fails ranks (the word of 2048 votes is left to neither kernel) and the refusal test,
                                                  which trains ranks again. Moved in both kernels the change cannot be seen: they
                                                  compute the same median.
  `select(m / 2 - 1)` for odd m                   fails 22: ranks, ties, term3, every sigma and csr scene (not hub and frames: even m)
  `(uint32_t)c < rank` in select                  fails 24: every training scene but cleanup (words of one vote)
  `atomicMin` in k_tr_stats2                      fails 25: every training scene (the class weights)
  `variance /= num`                               fails 24: every training scene but hub (sigma^2 = 0 there)
  `words <= max_elements`                         fails 22: every training scene but ranks and hub (sigma^2 = 0 on any sample there)
  `>=` on the 2 sigma test                        fails votes_edges at all 16 flag values
  `<=` on the epsilon test                        fails votes_edges at flags 2 and 3 (where the weight is exactly FLT_EPSILON)
  the matching weight evaluated in float          fails votes_edges at the 8 flag values with the matching term
  `trace >= 0.0f`                                 fails votes_edges at all 16 flag values: the rotation is the same, but four of the
                                                  eight 120-degree turns (trace exactly 0) get the negated quaternion, which the bbox
                                                  quaternion b * q of their live votes shows. No training output depends on the sign.
  `>=` on both diagonal comparisons (a 13th build) fails votes_edges at all 16 flag values in the same way (9 frames of trace 0 or -1)
Two changes are NOT observable and pass:
  the bisection started at bit 29                 every weight is exp(-x) <= 1.0f = 0x3f800000, so bit 30 is never set
  `c <= 1` in the clean-up                        the flag reads `c > 0 && (!clean_up || c <= 1)`: with c > 0 in front it is c == 1
"""
import time

import numpy as np
import pytest

import codebook_scenes as sc
from test_codebook_cpu import (NEAR_TIE, TOL_POS, TOL_SIGMA, TOL_W, TOL_XYZ, exact_frames, same_kind, sigma32, sigma_error, weight_close)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def train_on(pkg, gpu, s):
    """the scene through capi.train_activate_lists (through capi.train_activate where the scene gives k: the kNN hand-over and the
    clean-up are then the point)"""
    ctx, dev = gpu
    kp = s["kp"]
    args = (ctx, s["metric"], T(s["desc"], dev), T(s["lrf"], dev), T(kp[:, 0], dev), T(kp[:, 1], dev), T(kp[:, 2], dev), s["cls"], s["model"], s["centre"])
    cw = None if s["codewords"] is None else T(s["codewords"], dev)
    if "k" in s:
        return pkg.capi.train_activate(*args, k=s["k"], clean_up=s["clean_up"], n_classes=s["n_classes"], codewords=cw)
    return pkg.capi.train_activate_lists(*args, s["act_off"], T(s["act_idx"].astype(np.int32), dev), n_classes=s["n_classes"], codewords=cw)


def check_training(name, s, ref, got, ora):
    for key in ("word_src", "vote_offsets", "vote_feature"):
        assert np.array_equal(got[key], ref[key]), key
    ev = ref["evaluated"]
    ew = np.abs(got["vote_weight"][ev] - ref["vote_weight"][ev]).max(initial=0.0)
    ex = np.abs(got["vote_xyz"] - ref["vote_xyz"]).max(initial=0.0)
    es = sigma_error(got["class_sigma"], ref["class_sigma"])
    print(f"{name}: weights {ew:.3g} ({ew / TOL_W:.2f} TOL_W), votes {ex:.3g} ({ex / TOL_XYZ:.2f} TOL_XYZ), sigma {es:.3g} ({es / TOL_SIGMA:.2f} TOL_SIGMA), "
          f"{int(ev.sum())} of {len(ev)} weights compared")
    assert not np.isnan(got["vote_weight"]).any()
    assert ew <= TOL_W, np.argwhere(np.abs(got["vote_weight"] - ref["vote_weight"]) > TOL_W)[:10]
    assert ex <= TOL_XYZ
    assert same_kind(got["class_sigma"], ref["class_sigma"]) and es <= TOL_SIGMA, (got["class_sigma"], ref["class_sigma"])
    assert np.array_equal(got["vote_class_weight"].view(np.uint32), ref["vote_class_weight32"].view(np.uint32))
    want = sigma32(ora, s)                                        # the sequential float32 sums of the oracle
    ok = ~np.isnan(want)
    assert np.array_equal(got["class_sigma"].view(np.uint32)[ok], want.view(np.uint32)[ok])


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_training_scene_against_float64(pkg, gpu, ora, name):
    s, ref = sc.scene(name), sc.reference(name)
    t0 = time.perf_counter()
    got = train_on(pkg, gpu, s)
    print(f"{name}: device call {time.perf_counter() - t0:.2f} s")
    check_training(name, s, ref, got, ora)
    if name == "frames":
        exact = exact_frames(ref)[ref["vote_feature"]]
        assert exact.sum() == 12
        assert np.array_equal(got["vote_xyz"][exact].astype(f64), ref["vote_xyz"][exact])
        near = ref["near_tie"][ref["vote_feature"]]
        undecided = (near > 0) & (near < NEAR_TIE)
        print(f"frames: {int(undecided.sum())} undecided frames of {len(near)}")
    if name == "ties":
        w = got["vote_weight"]; vo = ref["vote_offsets"].astype(np.int64)
        assert np.all(w[vo[0]:vo[2]] == 1) and np.all(w[vo[7]:vo[9]] == 1)                   # exactly 1.0f
        assert np.array_equal(w[vo[4]:vo[7]], np.array([0.5] * 4 + [1, 1, 1, 0, 0] + [0, 1, 1], f32))      # exactly 0.0f
        assert len(np.unique(w[vo[3]:vo[4]])) == 1                                            # the tetrahedron: the tied value itself


def test_hub_twin_is_refused_and_the_context_stays_usable(pkg, gpu, ora):
    """32769 votes of one word: ISMHIP_ERR_UNSUPPORTED (-4), an ordinary refusal; the same context then trains `ranks` correctly"""
    with pytest.raises(pkg.capi.IsmHipError, match=r"\(-4\).*32768"):
        train_on(pkg, gpu, sc.hub(sc.HUB_M + 1))
    check_training("ranks", sc.scene("ranks"), sc.reference("ranks"), train_on(pkg, gpu, sc.scene("ranks")), ora)


def test_descriptor_of_1345_is_refused_and_the_context_stays_usable(pkg, gpu, ora):
    with pytest.raises(pkg.capi.IsmHipError, match=r"\(-4\).*1344"):
        train_on(pkg, gpu, sc.sigma(0, 1345))
    name = "sigma-l2-33"
    check_training(name, sc.scene(name), sc.reference(name), train_on(pkg, gpu, sc.scene(name)), ora)


# ----------------------------------------------------------------------------------------------------------- vote casting
def device_codebook(pkg, ctx, cb):
    return pkg.capi.Codebook(ctx, cb["words"], cb["vote_offsets"], cb["vote_xyz"], cb["vote_class"], cb["vote_instance"], cb["n_classes"],
                             cb["class_sigma"], word_weight=cb["word_weight"], vote_weight=cb["vote_weight"], vote_class_weight=cb["vote_class_weight"],
                             vote_bbox_quat=cb["vote_bbox_quat"], vote_bbox_size=cb["vote_bbox_size"])


def check_votes(ref, got, want_bbox):
    g = {k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}
    live = ref["live"]
    assert np.array_equal(g["cls"] >= 0, live), np.argwhere((g["cls"] >= 0) != live)[:10]
    for key in ("cls", "inst", "codeword"):
        assert np.array_equal(g[key], ref[key]), key
    assert weight_close(g["weight"], ref["weight"])                        # the same bytes: float32 products, the matching term rounded once
    ep = np.abs(g["pos"] - ref["pos"]).max()
    assert ep <= TOL_POS and np.all(g["pos"][~live] == 0)
    if want_bbox:
        assert np.abs(g["bbox_quat"] - ref["bbox_quat"]).max() <= TOL_POS and np.array_equal(g["bbox_size"], ref["bbox_size"])
    else:
        assert g["bbox_quat"] is None and g["bbox_size"] is None
    return ep


@pytest.mark.parametrize("flags", range(16))
def test_votes_edges_csr_and_dense(pkg, gpu, flags):
    ctx, dev = gpu
    s, ref = sc.votes_scene(), sc.votes_reference(flags)
    cb = device_codebook(pkg, ctx, s["cb"])
    try:
        assert cb.max_votes == 4
        frame = (T(s["lrf"], dev), T(s["kp"][:, 0], dev), T(s["kp"][:, 1], dev), T(s["kp"][:, 2], dev))
        worst = 0.0
        for want_bbox in (True, False):
            got = pkg.capi.cast_votes_csr(ctx, cb, flags, *frame, s["act_off"], T(s["idx"], dev), T(s["dist"], dev), want_bbox=want_bbox)
            worst = max(worst, check_votes(ref, got, want_bbox))
            dense = pkg.capi.cast_votes(ctx, cb, flags, *frame, T(s["dense_idx"], dev), T(s["dense_dist"], dev), want_bbox=want_bbox)
            slots = sc.dense_slots(s)
            for key, v in dense.items():                                       # the same slots for the same activations, byte for byte
                if v is not None:
                    a, b = v.cpu().numpy()[slots], got[key].cpu().numpy()
                    assert np.array_equal(a.view(np.uint32) if a.dtype == f32 else a, b.view(np.uint32) if b.dtype == f32 else b), key
            pad = np.setdiff1d(np.arange(dense["cls"].shape[0]), slots)
            assert np.all(dense["cls"].cpu().numpy()[pad] == -1) and np.all(dense["weight"].cpu().numpy()[pad] == 0)
        print(f"votes_edges flags {flags}: positions {worst:.3g} ({worst / TOL_POS:.2f} TOL_POS), {int(ref['live'].sum())} live of {len(ref['live'])} slots")
    finally:
        ctx.sync(); cb.close()

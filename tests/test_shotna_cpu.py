"""The SHOTNA reference frame on the host (no GPU): known answers of the restatement shotna_ref.py, proof that every scene of
shotna_scenes.py reaches the branch test_gpu_shotna.py asserts on it and keeps clear of votes that could fall either way, the host
config (ReferenceFrameType "SHOTNA" accepted and round-tripped, "BOARD" refused, anything else a bad parameter), and the C ABI's name."""
import json
import os

import numpy as np
import pytest

import host_binding as hb
import shotna_ref as ref
import shotna_scenes as sc
from test_host_layer import _cfg

f32 = np.float32


# ------------------------------------------------------------------------------------------------ known answers
def _patch(up):
    """planar anisotropic patch z = 0 around the origin: 60 points at x < 0 and 140 at x > 0, each with its mirror image in y (the
    covariance is diagonal: the axes are the coordinate axes), normals (0, 0, up)"""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(0.02, 0.25, 70), rng.uniform(-0.25, -0.02, 30)])
    y = rng.uniform(0.01, 0.1, 100)
    p = np.concatenate([np.stack([x, y, np.zeros(100)], 1), np.stack([x, -y, np.zeros(100)], 1)]).astype(f32)
    return p, np.tile(f32([0, 0, up]), (200, 1))


@pytest.mark.parametrize("up", [1, -1])
def test_planar_patch_has_the_closed_form_frame(up):
    p, n = _patch(up)
    r = ref.frame_of_keypoint(p, n, f32([0, 0, 0]), 0.3)
    assert r["valid"] == 200 and r["plusT"] in (80, -80) and abs(r["plusN"]) == 200 and r["decided_x"] and r["decided_z"] and r["gap"] > 0.1
    np.testing.assert_allclose(r["frame"], [1, 0, 0, 0, up, 0, 0, 0, up], atol=1e-6)
    # the position rule cannot tell the two sides of a plane apart: every vij . v3 is 0 and counts as plus; x is the same
    shot = ref.frame_of_keypoint(p, n, f32([0, 0, 0]), 0.3, normal_votes=False)
    assert shot["plusN"] == 200 and shot["small_z"] == 200 and not shot["decided_z"] and np.array_equal(shot["frame"][:3], r["frame"][:3])


def _ten_plus_one(coincident_up):
    """10 neighbours (z spread the smallest, five normals up and five down) + one point ON the keypoint with its normal up or down"""
    rng = np.random.default_rng(6)
    p = (rng.normal(size=(10, 3)) * [0.12, 0.07, 0.03]).astype(f32)
    n = np.tile(f32([0, 0, 1]), (10, 1)); n[5:] = -n[5:]
    return np.concatenate([p, np.zeros((1, 3), f32)]), np.concatenate([n, f32([[0, 0, 1 if coincident_up else -1]])])


def test_the_coincident_point_votes_with_its_normal():
    """v3 oriented upwards: six of eleven normals up give 2 * 6 - 10 = +2; five of eleven give 0 and the five medians decide by position"""
    up = ref.frame_of_keypoint(*_ten_plus_one(True), f32([0, 0, 0]), 0.5, v3_hint=[0, 0, 1])
    dn = ref.frame_of_keypoint(*_ten_plus_one(False), f32([0, 0, 0]), 0.5, v3_hint=[0, 0, 1])
    for r in (up, dn):
        assert r["valid"] == 10 and r["in_ball"] == 11 and r["gap"] > 0.1 and r["decided_x"] and r["small_z"] == 0
    assert up["plusN"] == 2 and not up["tie_z"] and up["frame"][8] > 0.9
    assert dn["plusN"] == 0 and dn["tie_z"]
    p, _ = _ten_plus_one(False)
    d2 = (p[:10].astype(np.float64) ** 2).sum(1)
    med = p[np.argsort(d2, kind="stable")[3:8]].astype(np.float64)          # ranks valid / 2 - 2 .. valid / 2 + 2
    assert ((med @ dn["frame"][6:9].astype(np.float64)) > 0).sum() >= 3 and abs(dn["frame"][8]) > 0.9
    # the reference's sum is not antisymmetric when a point lies on the keypoint: for -v3 it is 2 c - plusN, so sums of 0 .. 2 c depend
    # on the sign the eigen-solver happens to give v3. The restatement reports such a keypoint as not decided.
    assert not up["decided_z"] and not dn["decided_z"]
    flipped = ref.frame_of_keypoint(*_ten_plus_one(True), f32([0, 0, 0]), 0.5, v3_hint=[0, 0, -1])
    assert flipped["plusN"] == 0 and flipped["tie_z"]


def test_four_neighbours_and_a_coincident_point_give_nan():
    p, n = _ten_plus_one(True)
    r = ref.frame_of_keypoint(np.concatenate([p[:4], p[10:]]), np.concatenate([n[:4], n[10:]]), f32([0, 0, 0]), 0.5)
    assert r["valid"] == 4 and r["in_ball"] == 5 and np.isnan(r["frame"]).all()


def test_a_nan_normal_never_counts_as_plus():
    p, n = _patch(1)
    n = n.copy(); n[:3, 2] = np.nan; n[3, 0] = np.nan
    for hint in ([0, 0, 1], [0, 0, -1]):
        r = ref.frame_of_keypoint(p, n, f32([0, 0, 0]), 0.3, v3_hint=hint)
        assert r["plusN"] == (2 * 196 - 200 if hint[2] > 0 else -200) and r["frame"][8] == 1


# ------------------------------------------------------------------------------------------------ the GPU scenes reach their branches
@pytest.mark.parametrize("s", sc.gpu_scenes(), ids=lambda s: s.name)
def test_scene_is_clear_of_undecidable_votes(s):
    r = s.reference()
    fin = np.isfinite(r["frame"][:, 0])
    assert fin.any() and np.nanmin(r["gap"]) >= 1e-3
    undecided = int((~r["decided"][fin]).sum())
    print(f"{s.name}: {fin.sum()} valid keypoints, smallest gap {np.nanmin(r['gap']):.3g}, undecided {undecided}, z ties {int(r['tie_z'].sum())}")
    assert undecided <= 0.01 * fin.sum()
    if s.name.startswith(("mirror", "dense-")):
        assert undecided == 0


@pytest.mark.parametrize("negated", [False, True])
def test_generic_scene_turns_z_with_the_normals(negated):
    """inside a convex surface the position rule turns z inward at every keypoint, the normal rule along the normals"""
    s = sc.get(sc.generic, negated)
    na, shot = s.reference(True), s.reference(False)
    assert np.isfinite(na["frame"]).all() and na["in_ball"][0] == na["valid"][0] + 1 and (na["in_ball"][1:] == na["valid"][1:]).all()
    assert np.array_equal(na["frame"][:, :3], shot["frame"][:, :3])
    sgn = -1.0 if not negated else 1.0
    assert np.array_equal(na["frame"][:, 6:9], f32(sgn) * shot["frame"][:, 6:9])
    pt_off, p, n, kp_off, kp = s.soa()
    for k in range(len(kp)):
        ball = ((p.astype(np.float64) - kp[k]) ** 2).sum(1) < s.radius ** 2
        mean_n = n[ball].astype(np.float64).mean(0)
        assert na["frame"][k, 6:9] @ (mean_n / np.linalg.norm(mean_n)) >= 0.70
    assert not na["tie_z"].any() and (np.abs(na["plusN"]) > 2).all()


def test_ragged_scene_holds_its_edge_cases():
    s = sc.get(sc.ragged)
    r = s.reference()
    pt_off, p, n, kp_off, kp = s.soa()
    assert len(pt_off) == 12 and pt_off[3] == pt_off[2] and pt_off[5] - pt_off[4] == 4 and np.isnan(p).any()
    nan = np.isnan(r["frame"][:, 0])
    want = np.zeros(len(kp), bool)
    want[kp_off[2]] = True; want[kp_off[4]:kp_off[5]] = True; want[kp_off[1] - 2:kp_off[1]] = True      # empty, 4 points, far away, NaN
    assert np.array_equal(nan, want) and np.array_equal(np.isnan(r["frame"]).all(1), nan)
    o, j = sc.RAGGED_NAN_BALL
    k = kp_off[o] + j
    bad = np.nonzero(np.isnan(n).any(1))[0]
    assert len(bad) == 3 and (bad >= pt_off[o]).all() and (bad < pt_off[o + 1]).all() and r["in_ball"][k] > 50
    assert (((p[bad].astype(np.float64) - kp[k]) ** 2).sum(1) < 0.25 * s.radius ** 2).all()               # well inside that ball
    firsts = [kp_off[i] for i in (0, 1, 3, 5, 6)]                          # first keypoints sit on surface points
    assert ((r["in_ball"] - r["valid"])[firsts] == 1).all() and r["decided"][~nan].all()


@pytest.mark.parametrize("m", sc.MIRROR_M)
def test_mirror_scenes_reach_every_count(m):
    r = {kind: sc.get(sc.mirror, m, kind).reference() for kind in sc.MIRROR_SETS}
    u = sc.MIRROR_U
    for kind, q in r.items():
        assert q["valid"][0] == 2 * m and q["plusT"][0] == 0 and q["tie_x"][0] and q["decided"][0], kind
    assert abs(r["one-way"]["plusN"][0]) == 2 * m and not r["one-way"]["tie_z"][0]
    assert r["mirrored"]["plusN"][0] == 0 and r["half"]["plusN"][0] == 0 and r["mirrored"]["tie_z"][0] and r["half"]["tie_z"][0]
    assert abs(r["half-minus"]["plusN"][0]) == 2 and abs(r["half-plus"]["plusN"][0]) == 2
    z = {kind: q["frame"][0, 6:9].astype(np.float64) for kind, q in r.items()}
    assert z["half-minus"] @ u < -0.5 and z["half-plus"] @ u > 0.5 and z["one-way"] @ u > 0.5
    # the two one-vote outcomes are opposite, so the tie's outcome is opposite to one of them: a count off by one vote shows
    assert np.array_equal(z["half-minus"], -z["half-plus"])
    assert np.array_equal(z["half"], z["half-plus"]) != np.array_equal(z["half"], z["half-minus"])
    assert np.array_equal(z["half"], z["mirrored"])                         # both ties are decided by the same five positions


def test_dense_scene_deals_zero_and_two():
    base = sc.get(sc.dense, None).reference()
    assert base["valid"].min() > 4000 and base["valid"].max() > 20000 and len(base["valid"]) == 40
    z = {}
    for deal, want in sc.DENSE_DEALS.items():
        r = sc.get(sc.dense, deal).reference()
        assert abs(r["plusN"][0]) == abs(want) and r["tie_z"][0] == (want == 0) and r["decided"].all() and r["valid"][0] % 2 == 0
        z[deal] = r["frame"][0, 6:9]
    u = np.zeros(3); u[np.argmax(np.abs(base["frame"][0, 6:9]))] = 1
    assert abs(base["frame"][0, 6:9] @ u) > 0.5
    assert z["plus"] @ u > 0.5 and z["minus"] @ u < -0.5 and np.array_equal(z["plus"], -z["minus"])


# ------------------------------------------------------------------------------------------------ host config and C ABI
def _features(frame_type):
    return _cfg(**{"Children/Features/Parameters/ReferenceFrameType": frame_type})


def test_host_accepts_shotna_and_round_trips_it():
    m = hb.Model()
    m.config_from_json(_features("SHOTNA"))
    out = json.loads(m.config_to_json())
    assert out["Children"]["Features"]["Parameters"]["ReferenceFrameType"] == "SHOTNA"
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())
    assert json.loads(m2.config_to_json())["Children"]["Features"] == out["Children"]["Features"]
    m.close(); m2.close()
    m = hb.Model()
    m.config_from_json(_cfg())
    assert json.loads(m.config_to_json())["Children"]["Features"]["Parameters"]["ReferenceFrameType"] == "SHOT"     # the default stays
    m.close()


def test_host_refuses_board_and_flare_and_rejects_nonsense():
    for name in ("BOARD", "FLARE"):
        m = hb.Model()
        with pytest.raises(hb.HostError, match=r'not built.*"SHOT", "SHOTNA"'):
            m.config_from_json(_features(name))
        m.close()
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"invalid reference frame type \(Value: nonsense\)"):
        m.config_from_json(_features("nonsense"))
    m.close()


def test_driver_config_takes_the_two_frame_types(pkg):
    assert pkg.pipeline.IsmConfig().lrf_type == "SHOT" and pkg.pipeline.IsmConfig(lrf_type="SHOTNA").lrf_type == "SHOTNA"
    for bad in ("BOARD", "FLARE", "shotna", ""):
        with pytest.raises(ValueError, match="lrf_type"):
            pkg.pipeline.IsmConfig(lrf_type=bad)


def test_shotna_entry_is_declared_and_listed(pkg):
    header = open(os.path.join(hb.ROOT, "include", "ismhip.h")).read()
    assert "ismhip_shotna_lrf(" in header and "ismhip_shotna_lrf" in pkg.capi.EXPORTS

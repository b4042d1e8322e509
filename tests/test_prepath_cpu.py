"""Host-side proofs for the normals and voxel-keypoint tests (no GPU): the float64 references of normals_ref.py / voxel_ref.py
agree with the oracle as far as the oracle's own float arithmetic goes, and every scene of prepath_scenes.py reaches the case it
was built for. Only then do the references judge a kernel (test_gpu_normals.py, test_gpu_voxel.py)."""
import numpy as np
import pytest

import frontend_scenes as fs
import normals_ref as nr
import prepath_scenes as ps
import voxel_ref as vr

f32 = np.float32
QS = [0.5, 0.99, 0.995, 1.0]


# ------------------------------------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("orientation", [0, 1])
def test_normals_ref_matches_oracle_on_generic(ora, orientation):
    """NaN pattern equal, sign equal outside the |cos| exemption, q99.5 of the angle below the 2e-3 of test_estimate_normals_pca:
    that is all PCL's float covariance allows. Orientation 1: the oracle searches in centroid-shifted float coordinates, the
    reference (as the device) in the original ones; the count of points whose angle exceeds 1e-3 (about one neighbour) is printed."""
    s = ps.normal_scene("generic")
    want, cos = nr.orient(s["off"], s["P"], s["ref"], orientation)
    got = ora.pca_normals(s["off"], *fs.cols(s["P"]), s["radius"], orientation).astype(np.float64)
    assert np.array_equal(np.isnan(got).any(1), np.isnan(want).any(1))
    ok = s["ref"].valid
    ang = nr.angle(got[ok], want[ok])
    q = np.quantile(ang, QS)
    print(f"generic, orientation {orientation}: oracle vs float64 reference, angle quantiles {QS} = {q}, above 1e-3: {(ang > 1e-3).sum()}"
          f" of {ok.sum()}, neighbours {s['ref'].count[ok].min()}..{s['ref'].count[ok].max()}")
    assert q[2] < 2e-3, q
    decided = ok & (cos >= nr.COS_MIN)
    assert ((got[decided] * want[decided]).sum(1) > 0).all()
    assert s["ref"].gap[ok].min() > 1e-2 and cos[ok].min() > 0, (s["ref"].gap[ok].min(), cos[ok].min())


def test_raw_sign_matches_oracle(ora):
    """the closed form of pcl::eigen33's sign against the oracle's unflipped normals, wherever the component margin allows"""
    s = ps.normal_scene("generic")
    raw = ora.pca_normals(s["off"], *fs.cols(s["P"]), s["radius"], 2).astype(np.float64)
    want = nr.raw_sign(s["ref"].n)
    clear = s["ref"].valid & (s["ref"].margin > nr.MARGIN_MIN)
    k = np.argmax(np.abs(want[clear]), axis=1)
    print("raw_sign: clear points", int(clear.sum()), "of", int(s["ref"].valid.sum()), "largest component on x / y / z", np.bincount(k, minlength=3))
    assert clear.sum() > 6000 and np.bincount(k, minlength=3).min() > 500
    assert ((raw[clear] * want[clear]).sum(1) > 0).all()


def _oracle_voxels(ora, s, o):
    p, c = s["objs"][o], s["rgba"][o]
    return ora.voxel_grid(p[:, 0], p[:, 1], p[:, 2], s["leaf"], c)


@pytest.mark.parametrize("name", [n for n in ps.VOXEL_SCENES if n != "crowded"])
def test_voxel_ref_matches_oracle(ora, name):
    s = ps.voxel_scene(name)
    for o, ref in enumerate(s["ref"]):
        wx, wy, wz, wc = _oracle_voxels(ora, s, o)
        assert len(wx) == len(ref["key"]), (o, len(wx), len(ref["key"]))
        if len(wx):
            np.testing.assert_allclose(np.stack([wx, wy, wz], 1), ref["xyz"], rtol=2e-6, atol=2e-6)
            assert np.array_equal(wc, ref["rgba"])
    print(name, "voxels per object", [len(r["key"]) for r in s["ref"]], "table entries", [r["n_table"] for r in s["ref"]])


def test_voxel_ref_on_the_crowded_voxel(ora):
    """counts, order and colours equal; at 30 000 points per voxel the oracle's float running sum is the less accurate side"""
    s = ps.voxel_scene("crowded")
    ref = s["ref"][0]
    wx, wy, wz, wc = _oracle_voxels(ora, s, 0)
    assert len(wx) == len(ref["key"]) and np.array_equal(wc, ref["rgba"])
    assert ref["count"].max() >= 30000 and ref["count"].max() < 65000
    got = np.stack([wx, wy, wz], 1).astype(np.float64)
    big = int(np.argmax(ref["count"]))
    err = np.abs(got - ref["xyz"])
    print("crowded: oracle float sum vs exact mean, crowded voxel", err[big], "in units of the device bound", (err / vr.bound(ref["xyz"], ref["maxabs"]))[big])
    others = np.arange(len(wx)) != big
    np.testing.assert_allclose(got[others], ref["xyz"][others], rtol=2e-6, atol=2e-6)    # same voxels in the same order


# ------------------------------------------------------------------------------------------------ scenes reach their cases
def test_exact_radius_scene_sits_on_the_decision():
    s = ps.normal_scene("exact_radius")
    P, r2 = s["P"], nr.r2_of(s["radius"])
    assert len(s["probes"]) >= 8 and float(r2) == 81.0 / 4096.0
    flipped = nr.unoriented(s["off"], P, s["radius"], flip_equal=True)
    moved = []
    for pr in s["probes"]:
        d_on, d_in = nr.sqdist3(P[pr["on"]], P[pr["q"]]), nr.sqdist3(P[pr["inside"]], P[pr["q"]])
        assert (d_on == r2).all() and (d_in < r2).all(), (d_on, d_in, r2)
        assert flipped.count[pr["q"]] == s["ref"].count[pr["q"]] + len(pr["on"])
        moved.append(float(nr.angle(flipped.n[pr["q"]], s["ref"].n[pr["q"]])))
    # ... and dropping the points just inside moves it as far
    print("exact radius: normal at the probes moves by", np.round(moved, 4), "rad when d2 <= r2 decides; neighbours at the probes",
          s["ref"].count[[pr["q"] for pr in s["probes"]]])
    assert min(moved) > 1e-2, moved


def test_inexact_radius_scene_is_decided_in_float32():
    s = ps.normal_scene("inexact_radius")
    P, r2 = s["P"], nr.r2_of(s["radius"])
    d_on = np.concatenate([nr.sqdist3(P[pr["on"]], P[pr["q"]]) for pr in s["probes"]])
    print("inexact radius (h = 0.05, r = 0.15): points meant to be on the radius fall below / on / above r2 in float32:",
          int((d_on < r2).sum()), int((d_on == r2).sum()), int((d_on > r2).sum()))
    # coordinates up to 8 carry 2^-21 steps against differences of ~0.1: d2 lands within 2 * 2^-21 / 0.1 ~ 1e-5 of r2, on both sides
    assert np.abs(d_on.astype(np.float64) / float(r2) - 1).max() < 2e-5 and (d_on < r2).sum() >= 3 and (d_on >= r2).sum() >= 3


def test_minimal_scene_counts():
    s = ps.normal_scene("minimal")
    for (start, n), want in zip(s["groups"], ps.MINIMAL_COUNTS):
        assert n == want and (s["ref"].count[start:start + n] == want).all()
    assert np.isnan(s["ref"].n[:2]).all() and s["ref"].valid[2:].all()


def test_method2_scene_crosses_a_chunk(ora):
    s = ps.normal_scene("method2")
    off, P = s["off"], s["P"]
    frames = ora.shot_lrf(off, *fs.cols(P), off, *fs.cols(P), s["radius"])
    fin = np.isfinite(P).all(1)
    bad = fin & ~np.isfinite(frames[:, 0])
    k = [int(bad[off[o]:off[o + 1]].sum()) for o in range(3)]
    kth = int(np.nonzero(fin[:off[1]])[0][k[0] - 1])
    print("method 2: invalid frames per object", k, "; the k-th finite point of object 0 has index", kth, "; NaN points at", s["nan_at"])
    assert k[0] >= 300 and kth >= 256 and kth > k[0] - 1 and k[1] == 0 and k[2] == 3
    assert len(s["nan_at"]) == 3 and max(s["nan_at"]) < 40
    assert bad[s["group_at"]].all() and (s["ref"].count[s["group_at"]] == 4).all()


@pytest.mark.parametrize("leaf", [0.25, 0.1])
def test_faces_scene_has_points_on_faces(leaf):
    s = ps.voxel_scene(f"faces-{leaf}")
    n = sum(int(vr.on_face(p, leaf).any(1).sum()) for p in s["objs"])
    neg = sum(int((vr.on_face(p, leaf) & (p < 0)).any(1).sum()) for p in s["objs"])
    print(f"faces, leaf {leaf}: points with a coordinate on a voxel face {n}, of them on a negative face {neg}")
    assert n >= 100 and neg >= 100


@pytest.mark.parametrize("name", list(ps.NORMAL_SCENES) + ["method2"])
def test_exemptions_are_few(name):
    """a point leaves the angle check when its eigenvalue gap is below 1e-3 and the sign check when |cos| is below 1e-5: at most
    1 % of any scene (the minimal scene's coincident and collinear groups are exempt by construction)"""
    s = ps.normal_scene(name)
    ok = s["ref"].valid
    shares = [float((s["ref"].gap[ok] < nr.GAP_MIN).mean())]
    for orientation in (0, 1):
        shares.append(float((nr.orient(s["off"], s["P"], s["ref"], orientation)[1][ok] < nr.COS_MIN).mean()))
    print(f"{name}: {ok.sum()} normals; exempt share: gap {shares[0]:.4f}, |cos| orientation 0 {shares[1]:.4f}, orientation 1 {shares[2]:.4f}; "
          f"min gap {s['ref'].gap[ok].min():.3g}")
    if name != "minimal":
        assert max(shares) <= 0.01, shares

"""CGF on the host (no GPU): the float64 restatement cgf_ref.py against answers worked out by hand, the cap on what the GPU tests may
leave undecided on the scenes of cgf_scenes.py, the perceptron's derived error bound against a float32 forward pass, the weights
container (tool, library loader, every refusal by name) and the host layer (header, binding, config, factory message)."""
import ctypes as C
import importlib.util
import json
import os
import re
import struct

import numpy as np
import pytest

import cgf_ref as ref
import cgf_scenes as scenes
import host_binding as hb
from test_host_layer import _cfg

F = np.float32
R, RMIN = 0.625, 0.03125             # rmin = 0.05 R, both exact


def _tool():
    spec = importlib.util.spec_from_file_location("cgf_weights", os.path.join(hb.ROOT, "tools", "cgf_weights.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ hand-derived answers
def test_radii_take_the_trip_through_to_string():
    assert ref.radii(0.625) == (0.625, 0.03125, 0.46875)
    # float32(0.4371234567) = 0.437123447...: "%f" keeps six decimals of R, 0.05 R and 0.75 R
    assert ref.radii(0.4371234567) == (0.437123, 0.021856, 0.327843)
    assert ref.radii(0.1) == (0.1, 0.005, 0.075)


def test_one_neighbour_on_each_axis():
    """r = 0.25: 16 ln(8) / ln(20) + 1 = 12.1 -> radial bin 12. +x: theta 90 (bin 5), phi 0 -> 12 * 180 / 360 = 6. +y: phi 90.0000008 -> 9.
    -y: phi -90.0000008 -> 12 * 89.9999992 / 360 = 2.99999997 -> 2, not 3: pcl::rad2deg multiplies by 57.29578, 8.5e-9 above 180 / pi.
    +z: theta 0 (bin 0), phi = atan2(0, 0) = 0 -> 6. -z: theta 180.0000015 -> 11.0000001 -> clamped to 10. -x (y = +0): phi 180.0000015
    -> 12.00000005 -> clamped to 11."""
    pts = np.array([[0.25, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.25], [0, 0, -0.25], [-0.25, 0.0, 0]])
    br, bt, bp = ref.bins(pts[:, 0], pts[:, 1], pts[:, 2], R, RMIN)
    assert br.tolist() == [12] * 6
    assert bt.tolist() == [5, 5, 5, 0, 10, 5]
    assert bp.tolist() == [6, 9, 2, 6, 6, 11]
    assert ref.index(12, 5, 6) == 12 + 17 * 5 + 187 * 6 and ref.DIM == 2244


def test_radial_edges():
    """r = rmin: 16 * 0 / ln(20) + 1 = 1 exactly -> bin 1. Just below: the sum is below 1 and the cast truncates -> 0, as for every smaller r
    (at r = rmin / 20 the sum is -15, clamped). r = R: 16 + 1 = 17 up to rounding -> clamped to 16. Bin k begins at rmin 20^((k - 1) / 16)."""
    below = RMIN * (1 - 2.0 ** -23)
    r = np.array([RMIN, below, RMIN / 20, 1e-300, R, RMIN * 20 ** (0.5 / 16), RMIN * 20 ** (1.5 / 16), RMIN * 20 ** (15.5 / 16)])
    br, _, _ = ref.bins(r, np.zeros_like(r), np.zeros_like(r), R, RMIN)
    assert br.tolist() == [1, 0, 0, 0, 16, 1, 2, 16]


def test_polar_edges():
    """theta = 0, 90, 180 and the first interior edge 180 / 11 degrees from either side"""
    e = np.deg2rad(180.0 / 11) * (180 / np.pi) / ref.RAD2DEG          # the angle whose rad2deg is 180 / 11
    th = np.array([0.0, np.pi / 2, np.pi, e * (1 - 1e-9), e * (1 + 1e-9)])
    _, bt, _ = ref.bins(0.25 * np.sin(th), np.zeros_like(th), 0.25 * np.cos(th), R, RMIN)
    assert bt.tolist() == [0, 5, 10, 0, 1]


def test_azimuth_seam_plus_and_minus_180():
    """x < 0 with y = +0: atan2 = +pi -> phi + 180 = 360.0000015 -> bin 12 -> clamped to 11. y = -0: atan2 = -pi -> phi + 180 = -1.5e-6 -> the
    cast truncates towards zero -> bin 0. The two zeros land at opposite ends of the histogram, as in the reference."""
    _, _, bp = ref.bins([-0.25, -0.25, -0.25, -0.25], [0.0, -0.0, 2.0 ** -100, -(2.0 ** -100)], [0.0] * 4, R, RMIN)
    assert bp.tolist() == [11, 0, 11, 0]


def test_nan_goes_to_bin_zero():
    """r = 0 gives ln r = -inf (radial bin 0) and acos(0 / 0) = NaN: polar bin 0 by the named deviation"""
    br, bt, bp = ref.bins([0.0, np.nan], [0.0, 0.1], [0.0, 0.1], R, RMIN)
    assert (br.tolist(), bt.tolist(), bp.tolist()) == ([0, 0], [0, 0], [6, 0])


NANF = np.full(9, np.nan, F)


def test_the_edge_island_by_the_restatement():
    """the island of cgf_scenes.EDGE_POINTS under an identity frame: the nearest point is skipped, every other point lands in the bin
    written next to it, none is undecided (the identity's dot products are exact)"""
    pts = np.asarray([p for p, _ in scenes.EDGE_POINTS], np.float64).astype(F)
    out = ref.raw(pts, np.zeros((1, 3), F), NANF[None], np.full((1, 3), np.nan, F), R)
    want = np.zeros(ref.DIM, np.int64)
    for _p, b in scenes.EDGE_POINTS[1:]:
        want[ref.index(*b)] += 1
    assert out["kind"] == ["identity"] and out["ball"][0] == len(pts) and out["skipped"][0] == 0 and out["sum"][0] == len(pts) - 1
    assert np.array_equal(out["counts"][0], want) and not out["undecided"][0]
    assert np.array_equal(out["rows"][0], (want / float(len(pts) - 1)).astype(F))


def test_skip_rule_duplicates_and_coincident_points():
    """the nearest point goes, by index among equals; a point with d2 <= 1e-15 goes too; no deposit left: a row of zeros, not NaN"""
    kp = np.zeros((1, 3), F); nn = np.full((1, 3), np.nan, F)
    dup = ref.raw(F([[0.0625, 0, 0], [0.0625, 0, 0], [0, 0.25, 0.125]]), kp, NANF[None], nn, R)
    assert dup["skipped"][0] == 0 and dup["sum"][0] == 2 and dup["counts"][0][ref.index(*ref.bins(0.0625, 0, 0, R, RMIN))] == 1
    co = ref.raw(F([[0, 0, 0], [1e-8, 0, 0], [0.25, 0.125, 0]]), kp, NANF[None], nn, R)
    assert co["ball"][0] == 3 and co["skipped"][0] == 0 and co["sum"][0] == 1
    far = ref.raw(F([[0.25, 0, 0]]), kp, NANF[None], nn, R)                # the one ball point is the nearest: skipped although it is 0.25 away
    assert far["ball"][0] == 1 and far["sum"][0] == 0 and not far["rows"].any() and np.isfinite(far["rows"]).all()
    none = ref.raw(F([[5, 5, 5]]), kp, NANF[None], nn, R)
    assert none["ball"][0] == 0 and none["skipped"][0] == -1 and not none["rows"].any()


def test_frame_rule():
    lrf = F([1, 0, 0, 0, 1, 0, 0, 0, 1])
    assert ref.frame(lrf, F([0, 0, 1]))[3] == "kept" and ref.frame(lrf, F([0, 0, -1]))[3] == "flipped"
    assert ref.frame(lrf, F([np.nan] * 3))[3] == "kept"                     # a NaN normal negates nothing
    ax, ay, az, kind, _ = ref.frame(lrf, F([0.6, 0, -0.8]))
    assert kind == "flipped" and np.array_equal(np.stack([ax, ay, az]), -lrf.reshape(3, 3))
    bad = lrf.copy(); bad[1] = np.nan
    assert ref.frame(bad, F([0, 0, -1]))[3] == "identity"


# ------------------------------------------------------------------------------------------------ the scenes
@pytest.mark.parametrize("k", range(scenes.N_SCENES))
def test_scene_caps_with_the_restatement_alone(k, ora):
    """frames by the CPU oracle's SHOT frames, normals by the float64 PCA: at most 5 % of a scene's keypoints are left undecided, and scene 0
    holds every case the GPU test is there for"""
    s = scenes.scene(k)
    _, _, rl = ref.radii(s["radius"])
    lrf = ora.shot_lrf(s["pt_off"], s["xyz"][:, 0], s["xyz"][:, 1], s["xyz"][:, 2], s["kp_off"], s["kp"][:, 0], s["kp"][:, 1], s["kp"][:, 2], rl)
    nrm, cnt, _gap = scenes.keypoint_normals(s)
    ans = scenes.answer(s, lrf, nrm.astype(F))
    nkp = len(s["kp"])
    print("scene %d: %d keypoints, %d undecided; balls %s" % (k, nkp, ans["undecided"].sum(), sorted(set(ans["ball"].tolist()))))
    assert ans["undecided"].sum() <= scenes.MAX_UNDECIDED * nkp
    assert np.isfinite(ans["rows"]).all() and np.allclose(ans["rows"].sum(1)[ans["sum"] > 0], 1.0, atol=1e-5)
    if k == 0:
        for n in (0, 1, 2, 63, 64, 65):
            assert n in ans["ball"].tolist()
        assert ans["ball"].max() >= 250
        kinds = ans["kind"]
        assert {"identity", "flipped", "kept"} <= set(kinds)
        a, b = scenes.object_of(s, "edges")
        assert kinds[a] == "identity" and ans["sum"][a] == len(scenes.EDGE_POINTS) - 1
        # a valid frame whose normal ball holds fewer than three points: nothing to flip against
        a, b = scenes.object_of(s, "ball 64")
        assert kinds[a] == "kept" and cnt[a] < 3 and np.isnan(nrm[a]).all()
        # both patches: normals exist; the one above the origin is flipped, the one below kept
        a, b = scenes.object_of(s, "patch above the origin")
        assert (cnt[a:b] >= 3).all() and set(kinds[a:b]) == {"flipped"}
        a, b = scenes.object_of(s, "patch below the origin")
        assert (cnt[a:b] >= 3).all() and set(kinds[a:b]) == {"kept"}
        # keypoints that are cloud points (d2 = 0 for the nearest) and keypoints that are not
        a, b = scenes.object_of(s, "patch above the origin")
        p = s["xyz"][s["pt_off"][9]:s["pt_off"][10]]
        on = [(p == q).all(1).any() for q in s["kp"][a:b]]
        assert any(on) and not all(on)
    else:
        assert ref.radii(s["radius"])[0] == 0.437123 != float(F(s["radius"]))


# ------------------------------------------------------------------------------------------------ the perceptron's bound
def _f32_forward(x, layers):
    x = np.asarray(x, F)
    for W, b, relu in layers:
        x = (x @ W + b).astype(F)
        if relu:
            x = np.maximum(x, F(0))
    return x


@pytest.mark.parametrize("nnz", [0, scenes.MLP_NNZ])
def test_mlp_bound_holds_for_a_float32_pass(nnz):
    """a float32 numpy pass (whatever order its BLAS sums in) lies inside the derived bound on the real shape; with the sparse weights the
    bound is a small share of what the outputs owe to the input, with the dense ones it is not (cgf_scenes.random_layers says why)"""
    rng = np.random.default_rng(5)
    layers = scenes.random_layers(rng, [2244, 512, 512, 512, 512, 40], nnz)
    x = rng.normal(size=(9, 2244)).astype(F)
    x[0] = 0
    y, e = ref.mlp(x, layers)
    assert np.allclose(y[0], ref.mlp(np.zeros((1, 2244)), layers)[0][0], rtol=1e-12, atol=0)   # an all-zero row: the bias path
    got = _f32_forward(x, layers)
    spread = np.abs(y[1:] - y[1:].mean(0)).max()
    print("nnz %d: largest bound %.3g, largest float32 error %.3g, outputs vary by %.3g over the rows" % (nnz, e.max(), np.abs(got - y).max(), spread))
    assert (np.abs(got - y) <= e).all() and (e > 0).all()
    if nnz:
        assert e.max() < 0.05 * spread
    hidden = np.maximum(x.astype(np.float64) @ layers[0][0] + layers[0][1], 0)
    assert 0.3 < (hidden == 0).mean() < 0.7                                 # weights of both signs: ReLU cuts about half
    assert ref.gamma(3) == pytest.approx(3 * 2.0 ** -24, rel=1e-6)


# ------------------------------------------------------------------------------------------------ the weights container
def _small_layers(seed=3, first=ref.DIM):
    return scenes.random_layers(np.random.default_rng(seed), [first, 48, 7])


def test_weights_round_trip_tool_and_library(pkg, tmp_path):
    tool = _tool()
    layers = _small_layers()
    npz = str(tmp_path / "w.npz"); cg = str(tmp_path / "w.cgfw"); back = str(tmp_path / "back.npz")
    np.savez(npz, w1=layers[0][0], b1=layers[0][1], w2=layers[1][0], b2=layers[1][1])
    assert tool.main(["to-cgfw", npz, cg]) == 0 and tool.main(["to-npz", cg, back]) == 0 and tool.main(["info", cg]) == 0
    z = np.load(back)
    assert z["relu"].tolist() == [1, 0]
    got = pkg.capi.cgfw_read(cg, ref.DIM)                                   # the library's loader
    for l, (W, b, relu) in enumerate(layers):
        assert np.array_equal(z["w%d" % (l + 1)], W) and np.array_equal(z["b%d" % (l + 1)], b)
        assert np.array_equal(got[l][0], W) and np.array_equal(got[l][1], b) and got[l][2] == relu
    raw = open(cg, "rb").read()
    assert raw[:4] == b"CGFW" and struct.unpack_from("<IIIII", raw, 4) == (1, 2, ref.DIM, 48, 1)
    assert len(raw) == 12 + 2 * 12 + 4 * (ref.DIM * 48 + 48 + 48 * 7 + 7)
    other = str(tmp_path / "lib.cgfw")
    pkg.capi.cgfw_write(other, layers)                                      # the binding's writer gives the same bytes
    assert open(other, "rb").read() == raw
    assert pkg.pipeline.IsmConfig(n_classes=3, feature="CGF", cgf_model=cg).dim == 7


def _refusals(tmp_path):
    """(file, the loader's word for it)"""
    layers = _small_layers()
    tool = _tool()
    good = str(tmp_path / "good.cgfw")
    tool.write_cgfw(good, layers)
    raw = open(good, "rb").read()
    cases = []

    def put(name, data, word):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        cases.append((p, word))
    put("magic.cgfw", b"CGFX" + raw[4:], "wrong magic")
    put("version.cgfw", raw[:4] + struct.pack("<I", 2) + raw[8:], "unsupported version")
    put("count.cgfw", raw[:8] + struct.pack("<I", 9) + raw[12:], "layer count")
    put("trunc_header.cgfw", raw[:10], "truncated file")
    put("trunc_weights.cgfw", raw[:-5], "truncated file")
    put("trailing.cgfw", raw + b"\0", "trailing bytes")
    w2_at = 12 + 12 + 4 * (ref.DIM * 48 + 48)
    put("widths.cgfw", raw[:w2_at] + struct.pack("<I", 47) + raw[w2_at + 4:], "inconsistent widths")
    put("activation.cgfw", raw[:20] + struct.pack("<I", 5) + raw[24:], "unknown activation")
    put("range.cgfw", raw[:16] + struct.pack("<I", 513) + raw[20:], "width out of range")
    bad = bytearray(raw); bad[24:28] = struct.pack("<f", float("inf"))
    put("inf.cgfw", bytes(bad), "non-finite weight")
    bad = bytearray(raw); bad[-4:] = struct.pack("<f", float("nan"))
    put("nan_bias.cgfw", bytes(bad), "non-finite weight")
    first = str(tmp_path / "first.cgfw")
    tool.write_cgfw(first, _small_layers(first=100))
    cases.append((first, "first layer width"))
    cases.append((str(tmp_path / "missing.cgfw"), "cannot open"))
    return good, cases


def test_loader_refuses_by_name(pkg, tmp_path):
    tool = _tool()
    good, cases = _refusals(tmp_path)
    assert len(pkg.capi.cgfw_read(good, ref.DIM)) == 2 and len(tool.read_cgfw(good, ref.DIM)) == 2
    for path, word in cases:
        with pytest.raises(pkg.capi.IsmHipError, match=word):
            pkg.capi.cgfw_read(path, ref.DIM)
        if word != "cannot open":
            with pytest.raises(tool.CgfwError, match=word):
                tool.read_cgfw(path, ref.DIM)
    assert len(pkg.capi.cgfw_read(cases[-2][0], 0)) == 2                    # without an expected width the 100-wide net is a valid file


# ------------------------------------------------------------------------------------------------ host layer
NEW_SYMBOLS = ["ismhip_keypoint_normals_pca", "ismhip_cgf_raw", "ismhip_mlp_create", "ismhip_mlp_destroy", "ismhip_mlp_forward", "ismhip_mlp_in",
               "ismhip_mlp_out", "ismhip_cgfw_open", "ismhip_cgfw_close", "ismhip_cgfw_layers", "ismhip_cgfw_layer", "ismhip_mlp_from_cgfw"]


def test_library_exports_the_new_symbols(pkg):
    """fails on the parent commit: none of them exists there"""
    L = C.CDLL(pkg.capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None and name in pkg.capi.EXPORTS
    h = open(os.path.join(hb.ROOT, "include", "ismhip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, h)
    for name, v in (("RAW_DIM", 2244), ("RADIAL_BINS", 17), ("POLAR_BINS", 11), ("AZIMUTH_BINS", 12)):
        assert re.search(rf"#define ISMHIP_CGF_{name}\s+{v}\b", h)
    assert re.search(r"#define ISMHIP_ABI_VERSION\s+4\b", h)                 # additions only
    assert pkg.capi.CGF_RAW_DIM == 2244 and pkg.capi.cgf_radii(0.625) == ref.radii(0.625) and pkg.capi.cgf_radii(0.4371234567) == ref.radii(0.4371234567)


def _cgf_cfg(model, **params):
    p = {"ReferenceFrameRadius": 0.3, "ReferenceFrameType": "SHOT", "CgfModelFile": model}
    p.update(params)
    return _cfg(**{"Children/Features": {"Type": "CGF", "Parameters": p}})


def test_host_configures_cgf_and_reads_the_length_from_the_file(tmp_path):
    """on the parent commit the factory refuses the type"""
    good, _ = _refusals(tmp_path)
    m = hb.Model()
    m.config_from_json(_cgf_cfg(good, Radius=0.25))
    out = json.loads(m.config_to_json())["Children"]["Features"]
    assert out["Type"] == "CGF" and out["Parameters"]["Radius"] == pytest.approx(0.25) and out["Parameters"]["CgfModelFile"] == good
    assert m.L.ism3d_descriptor_length(m.h) == 7
    m2 = hb.Model()
    m2.config_from_json(m.config_to_json())                        # what we write, we read
    assert json.loads(m2.config_to_json())["Children"]["Features"] == out
    m.close(); m2.close()
    tool = _tool()
    d40 = str(tmp_path / "d40.cgfw")
    tool.write_cgfw(d40, scenes.random_layers(np.random.default_rng(1), [ref.DIM, 16, 40]))
    m = hb.Model()
    m.config_from_json(_cgf_cfg(d40))                              # Radius not given: the reference's default 0.1
    assert json.loads(m.config_to_json())["Children"]["Features"]["Parameters"]["Radius"] == pytest.approx(0.1)
    assert m.L.ism3d_descriptor_length(m.h) == 40
    m.close()


def test_host_refuses_bad_weights_files_by_name(tmp_path):
    _, cases = _refusals(tmp_path)
    for path, word in cases:
        m = hb.Model()
        with pytest.raises(hb.HostError, match="CGF: CgfModelFile: .*" + word):
            m.config_from_json(_cgf_cfg(path))
        m.close()


def test_host_reads_the_example_config(tmp_path, monkeypatch):
    """config/modelnet10_cgf.ism names the default file in the working directory, as the reference's hard-coded checkpoint name does"""
    src = json.load(open(os.path.join(hb.ROOT, "config", "modelnet10_cgf.ism")))["ObjectConfig"]
    assert src["Children"]["Features"]["Parameters"]["CgfModelFile"] == "embed_model_910000.cgfw"
    m = hb.Model()
    monkeypatch.chdir(tmp_path)
    with pytest.raises(hb.HostError, match="cannot open"):
        m.config_from_json(json.dumps(src))
    _tool().write_cgfw("embed_model_910000.cgfw", scenes.random_layers(np.random.default_rng(2), [ref.DIM, 8, 32]))
    m.config_from_json(json.dumps(src))
    out = json.loads(m.config_to_json())
    assert out["Children"]["Features"]["Type"] == "CGF" and out["Children"]["Features"]["Parameters"]["Radius"] == pytest.approx(0.4)
    assert m.L.ism3d_descriptor_length(m.h) == 32
    m.close()
    other = json.load(open(os.path.join(hb.ROOT, "config", "modelnet10_rsd.ism")))["ObjectConfig"]
    del src["Children"]["Features"]["Parameters"]["CgfModelFile"], other["Children"]["Features"]["Parameters"]["UseFullRSDHistogram"]
    for j in (src, other):                                         # the value set of modelnet10_rsd.ism, the feature apart
        del j["Children"]["Features"]["Type"]
    assert src == other


def test_pfh_is_still_refused_with_cgf_in_the_built_list():
    m = hb.Model()
    with pytest.raises(hb.HostError, match=r"outside the MI355X hot path \(built: .*CGF, RIFT, SpinImage, RSD, CoSPAIR\)"):
        m.config_from_json(_cfg(**{"Children/Features/Type": "PFH"}))
    m.close()

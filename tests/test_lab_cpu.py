"""CIELab without a GPU: the float CPU oracle over the WHOLE 24-bit colour cube against the float64 restatement lab_ref.py, which is
written from the reference's color_conversion.cpp and shares nothing with the oracle. Every colour reference in tests/ that borrows
ora.rgb2lab (short_cshot_ref, cospair_ref, culling_ref, frontend_scenes.edge_colors) rests on what is asserted here; the device is held
to the same rule, and to the oracle bit for bit, in test_gpu_lab.py.

Rule: where lab_ref calls a colour decided, every channel within lab_ref's derived float32 bound; elsewhere, on one of the candidate
table entries within the bound. Measured on the cube (printed by the test): 105 888 colours undecided (0.63 %; the cap is 2 %), largest
|oracle - lab_ref| / bound 0.46 / 0.51 / 0.51 (L, a, b), largest differences on decided colours 8.3e-6 / 4.6e-5 / 1.9e-5."""
import numpy as np
import pytest

import lab_ref
import shot_ref_scenes as srs

CHUNK = 1 << 20
_cube = {}


def cube(ora):
    """one pass over the 2^24 colours in 16 chunks -> the figures every test below reads"""
    if _cube:
        return _cube
    und, lo, hi = 0, np.full(3, np.inf), np.full(3, -np.inf)
    ratio = {False: np.zeros(3), True: np.zeros(3)}
    err = np.zeros(3)
    top = {srs.WHITE: 0, srs.BLACK: 0}
    for base in range(0, 1 << 24, CHUNK):
        c = np.arange(base, base + CHUNK, dtype=np.uint32)
        lab = lab_ref.convert(c)
        und += int((~lab.decided).sum())
        lo, hi = np.minimum(lo, lab.raw.min(0)), np.maximum(hi, lab.raw.max(0))
        for normalised in (False, True):
            got = ora.rgb2lab_n(c, normalised)
            ratio[normalised] = np.maximum(ratio[normalised], lab_ref.excess(got, lab, normalised).max(0))
            if not normalised:
                err = np.maximum(err, np.abs(got - lab.raw)[lab.decided].max(0))
        for k in top:                                            # the farthest colour step of CSHOT from white and from black
            ref = lab_ref.convert(np.uint32([k])).norm[0]
            cd = (np.abs(lab.norm[:, 0] - ref[0]) + (np.abs(lab.norm[:, 1] - ref[1]) + np.abs(lab.norm[:, 2] - ref[2])) / 2) / 3
            top[k] = max(top[k], int(np.floor(cd.max() * 30 + 0.5)))
    _cube.update(undecided=und, lo=lo, hi=hi, ratio=ratio, err=err, top=top)
    return _cube


def test_oracle_over_the_whole_cube_lies_within_the_float64_bound(ora):
    c = cube(ora)
    print("cube: undecided %d (%.3f %%), largest |oracle - lab_ref| / bound raw %s normalised %s, largest difference on decided colours %s"
          % (c["undecided"], 100.0 * c["undecided"] / (1 << 24), c["ratio"][False], c["ratio"][True], c["err"]))
    assert c["undecided"] <= 0.02 * (1 << 24)                    # a condition on the margin's derivation, not a measurement
    assert (c["ratio"][False] <= 1).all() and (c["ratio"][True] <= 1).all()


def test_the_clamps_are_dead_code_for_srgb_input(ora):
    """L > 100 and |a|, |b| > 120 cannot happen for any of the 2^24 colours: the three clamps of the text never act"""
    c = cube(ora)
    print("cube: L %.4f .. %.4f, a %.4f .. %.4f, b %.4f .. %.4f" % (c["lo"][0], c["hi"][0], c["lo"][1], c["hi"][1], c["lo"][2], c["hi"][2]))
    slack = lab_ref.convert(np.uint32([0xffffff])).e_raw.max() * 10
    assert c["lo"][0] >= 0 and c["hi"][0] < 100 - slack
    assert -120 + slack < c["lo"][1] and c["hi"][1] < 120 - slack and -120 + slack < c["lo"][2] and c["hi"][2] < 120 - slack
    assert abs(c["hi"][0] - 99.99) < 0.01 and abs(c["lo"][1] + 86.2) < 0.05 and abs(c["hi"][1] - 98.3) < 0.05
    assert abs(c["lo"][2] + 107.9) < 0.05 and abs(c["hi"][2] - 94.5) < 0.05


def test_the_palette_scenes_reach_the_farthest_colour_step_of_the_cube(ora):
    c = cube(ora)
    for k in (srs.WHITE, srs.BLACK):
        assert srs.palette_max_step(k) == c["top"][k], (hex(k), srs.palette_max_step(k), c["top"][k])


def test_bits_24_to_31_are_ignored(ora):
    rng = np.random.default_rng(5)
    c = rng.integers(0, 1 << 24, size=4096).astype(np.uint32)
    hi = (rng.integers(1, 256, size=4096).astype(np.uint32) << 24) | c
    assert np.array_equal(lab_ref.convert(c).raw, lab_ref.convert(hi).raw)
    for normalised in (False, True):
        assert ora.rgb2lab_n(c, normalised).tobytes() == ora.rgb2lab_n(hi, normalised).tobytes()
    assert ora.rgb2lab(int(hi[0])) == ora.rgb2lab(int(c[0])) == tuple(ora.rgb2lab_n(c[:1])[0].tolist())   # the batch is the single call


# textbook CIELab (D65) of the cube's corners; the text's 0.3333 exponent and 4000-entry table move them by < 0.15
CORNERS = {"black": (0x000000, (0.0, 0.0, 0.0)), "white": (0xffffff, (100.0, 0.0, 0.0)), "red": (0xff0000, (53.24, 80.09, 67.20)),
           "green": (0x00ff00, (87.73, -86.18, 83.18)), "blue": (0x0000ff, (32.30, 79.19, -107.86)), "yellow": (0xffff00, (97.14, -21.55, 94.48)),
           "cyan": (0x00ffff, (91.11, -48.09, -14.13)), "magenta": (0xff00ff, (60.32, 98.23, -60.82))}


@pytest.mark.parametrize("name", list(CORNERS))
def test_cube_corners(ora, name):
    rgba, want = CORNERS[name]
    lab = lab_ref.convert(np.uint32([rgba]))
    assert np.abs(lab.raw[0] - want).max() < 0.15, (name, lab.raw[0])
    assert bool(lab.decided[0]), name                            # white too: both candidates of its three channels clamp to entry 3999
    for normalised in (False, True):
        assert (lab_ref.excess(ora.rgb2lab_n(np.uint32([rgba]), normalised), lab, normalised) <= 1).all(), name
    if name == "white":
        assert lab.index[0].tolist() == [3999, 3999, 3999] and lab_ref.table_arguments(np.uint32([rgba]))[0, 1] >= 4000     # the one deviation (vy: its matrix row sums to 1)
        assert lab.raw[0, 1] == 0 and lab.raw[0, 2] == 0 and ora.rgb2lab(rgba)[1:] == (0.0, 0.0)
    if name == "black":
        assert lab.index[0].tolist() == [0, 0, 0] and abs(lab.raw[0]).max() < 1e-12 and max(abs(v) for v in ora.rgb2lab(rgba)) < 2e-6


def test_greys(ora):
    """the 256 greys: L rises strictly, a and b stay within one table step of 0 (the matrix rows sum to the white point only to
    5 digits, so the three indices of a grey may differ by one), and the oracle obeys the rule on each"""
    g = np.arange(256, dtype=np.uint32) * 0x010101
    lab = lab_ref.convert(g)
    assert (np.diff(lab.raw[:, 0]) > 0).all() and abs(lab.raw[0, 0]) < 1e-12 and 99.98 < lab.raw[255, 0] < 100
    assert (np.abs(np.diff(lab.index, axis=1)) <= 1).all()
    step = np.abs(np.diff(lab_ref.SXYZ_LUT)).max()
    assert np.abs(lab.raw[:, 1]).max() <= 500 * step and np.abs(lab.raw[:, 2]).max() <= 200 * step
    for normalised in (False, True):
        assert (lab_ref.excess(ora.rgb2lab_n(g, normalised), lab, normalised) <= 1).all()
    print("greys: undecided", int((~lab.decided).sum()), "of 256")


def test_undecided_colours_name_two_neighbouring_entries():
    rng = np.random.default_rng(6)
    c = rng.integers(0, 1 << 24, size=1 << 16).astype(np.uint32)
    lab = lab_ref.convert(c)
    und = ~lab.decided
    assert 0 < und.sum() < 0.02 * len(c)
    assert (np.abs(lab.alt - lab.index) <= 1).all() and (np.abs(lab.alt - lab.index)[und].max(1) == 1).all()
    assert (lab.alt[~und] == lab.index[~und]).all()
    raw, norm, e_raw, e_norm = lab_ref.candidates(lab_ref.Lab(*(f[und] for f in lab)))
    assert raw.shape == (und.sum(), 8, 3) and np.array_equal(raw[:, 0], lab.raw[und])           # combination 0 is the primary reading
    assert (np.abs(raw - raw[:, :1]).max((1, 2)) > 50 * e_raw.max()).all()                      # the other entry is far outside the bound


def test_the_probe_is_exported_and_the_abi_version_stays(pkg):
    import os
    import re
    L = pkg.capi.lib()
    assert "ismhip_rgb2lab" in pkg.capi.EXPORTS and L.ismhip_rgb2lab is not None and callable(pkg.capi.rgb2lab)
    assert L.ismhip_abi_version() == 4
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ismhip.h")).read()
    assert "int  ismhip_rgb2lab(" in h and re.search(r"#define ISMHIP_ABI_VERSION\s+4\b", h)

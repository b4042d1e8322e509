"""CIELab of packed 0x00RRGGBB colours in numpy float64, restated from third_party/pcl_color_conversion/color_conversion.cpp:19-83
of the reference (the two look-up tables of its constructor and RgbToCieLabNormalized), sharing no code with oracle/ or csrc/.

What is kept of the text: its constants ARE the float32 literals it names (0.412453f, 0.95047f, 2.4f, 0.3333f ...; 0.04045, 0.008856,
7.787 and 16.0 / 116.0 are doubles there and here), the table sizes 256 and 4000, the truncating index int(v * 4000), the clamps
L <= 100, |a|, |b| <= 120 and the normalisation (100, 120, 120). Every operation on them runs in float64 here. One deviation, which the
oracle and the device name too: the index is clamped to 0..3999 (white gives vx * 4000 = 4000.0005, one past the table in the text).

A float32 evaluation of the same text (the oracle's, the device's) differs from this one in two ways, both bounded below with
u = 2^-24 and first-order sums of relative errors (every intermediate is a sum of non-negative terms, so relative errors add and
never amplify; the few second-order terms are covered by the factor 1 + 2^-10 on every bound):

 1. THE TABLE INDEX. t = v * 4000 with
        f = i / 255                          1 rounding                                         u
        (f + 0.055f) / 1.055f                2 more                                             3 u
        powf(., 2.4f)                        the exponent multiplies the relative error, and powf is within 1 ulp <= 2 u of the true
                                             power (glibc documents < 1 ulp; an assumption about the platform's libm)
                                                                                                2.4 * 3 u + 2 u = 9.2 u
        (linear branch f / 12.92f: 2 u, smaller)
        fr * c1 + fg * c2 + fb * c3          a product each (u), two additions (u each)         12.2 u
        / 0.95047f, / 1.08883f               (y is not divided)                                 13.2 u
        * 4000                                                                                   14.2 u
    so |t32 - t64| <= INDEX_REL * t64, INDEX_REL = 14.2 u (1 + 2^-10): at most 3.4e-3 index units at the top of the table, 0 at
    black. Where t64 lies farther than that from every integer, int(t32) == int(t64): the colour is DECIDED. Elsewhere the float32
    evaluation may take either of the two neighbouring entries (k - 1 or k, k = the integer nearby), per channel; candidates() lists
    all of them. A colour whose two candidate indices coincide after the clamp (white) is decided.
 2. THE VALUE, given the index. A table entry powf(i / 4000, 0.3333f) carries 0.3333 * u + 2 u <= 2.34 u relative (the linear branch:
    one cast, u), on values v <= 1:
        L = 116 v - 16                       116 (2.34 u v) + u (116 v) [product] + u |L| [difference]
        a = 500 (vx - vy)                    500 (2.34 u (vx + vy)) + u |a| [difference, scaled] + u |a| [product]
        b = 200 (vy - vz)                    200 (2.34 u (vy + vz)) + 2 u |b|
        normalised: the bound divided by (100, 120, 120), plus u |value| for the division.
    At white this gives 2.9e-5 / 1.4e-4 / 5.6e-5 (measured, float32 oracle against this file on the whole cube: see test_lab_cpu.py).
"""
from collections import namedtuple

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
INDEX_REL = 14.2 * U * SLACK
ENTRY_REL = 2.34 * U
SCALE = np.array([100.0, 120.0, 120.0])


def _c(x):
    """the value of a float32 literal of the text"""
    return float(f32(x))


def _tables():
    i = np.arange(256, dtype=f64)
    f = i / 255.0
    srgb = np.where(f32(f).astype(f64) > 0.04045, ((f + _c(0.055)) / _c(1.055)) ** _c(2.4), f / _c(12.92))   # the test is on the float f (:25)
    j = np.arange(4000, dtype=f64)
    g = j / 4000.0
    sxyz = np.where(f32(g).astype(f64) > 0.008856, g ** _c(0.3333), 7.787 * g + 16.0 / 116.0)
    return srgb, sxyz


SRGB_LUT, SXYZ_LUT = _tables()
_M = np.array([[_c(0.412453), _c(0.357580), _c(0.180423)],
               [_c(0.212671), _c(0.715160), _c(0.072169)],
               [_c(0.019334), _c(0.119193), _c(0.950227)]])
_WHITE = np.array([_c(0.95047), 1.0, _c(1.08883)])

Lab = namedtuple("Lab", "raw norm e_raw e_norm decided index alt")


def channels(rgba):
    """(R, G, B) of packed colours; bits 24..31 are ignored"""
    c = np.asarray(rgba).astype(np.uint32).reshape(-1)
    return np.stack([(c >> 16) & 0xff, (c >> 8) & 0xff, c & 0xff], -1).astype(np.int64)


def table_arguments(rgba):
    """t = (vx, vy, vz) * 4000 in float64 [n, 3]: what int() truncates to the table index (:55-61)"""
    lin = SRGB_LUT[channels(rgba)]
    return (lin @ _M.T) / _WHITE * 4000.0


def _from_entries(idx):
    """Lab and its float32 error bounds from table indices [..., 3] (:63-82) -> raw, norm, e_raw, e_norm"""
    v = SXYZ_LUT[idx]
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    L = np.minimum(116.0 * vy - 16.0, 100.0)
    a = np.clip(500.0 * (vx - vy), -120.0, 120.0)
    b = np.clip(200.0 * (vy - vz), -120.0, 120.0)
    raw = np.stack([L, a, b], -1)
    e = np.stack([116.0 * vy * (ENTRY_REL + U) + U * np.abs(L),
                  500.0 * ENTRY_REL * (vx + vy) + 2 * U * np.abs(a),
                  200.0 * ENTRY_REL * (vy + vz) + 2 * U * np.abs(b)], -1) * SLACK
    norm = raw / SCALE
    return raw, norm, e, (e / SCALE + U * np.abs(norm)) * SLACK


def convert(rgba):
    """Lab of packed colours [n]:
    raw, norm [n, 3]     (L, a, b) as the text has them before / after its last three lines
    e_raw, e_norm [n, 3] what a float32 evaluation that took the SAME table entries may differ by, per channel
    decided [n]          True where every float32 evaluation takes these entries
    index [n, 3]         the entries taken here: int(t) clamped to 0..3999
    alt [n, 3]           the other entry a float32 evaluation may take (== index where that channel is decided)"""
    t = table_arguments(rgba)
    k = np.rint(t)
    near = np.abs(t - k) <= INDEX_REL * t
    index = np.clip(np.floor(t).astype(np.int64), 0, 3999)
    other = np.where(t >= k, k - 1, k)                        # t in [k, k + margin]: float32 may fall to k - 1; t in [k - margin, k): may reach k
    alt = np.where(near, np.clip(other.astype(np.int64), 0, 3999), index)
    raw, norm, e_raw, e_norm = _from_entries(index)
    return Lab(raw, norm, e_raw, e_norm, (alt == index).all(1), index, alt)


def candidates(lab):
    """every combination of entries a float32 evaluation may take -> raw, norm, e_raw, e_norm, each [n, 8, 3]"""
    pick = np.array([[(m >> c) & 1 for c in range(3)] for m in range(8)], bool)                 # [8, 3]
    idx = np.where(pick[None], lab.alt[:, None, :], lab.index[:, None, :])
    return _from_entries(idx)


def excess(got, lab, normalised):
    """|got - reference| / bound per colour and channel [n, 3] for float32 results `got`: on decided colours against the one reference,
    on undecided ones against the best of the candidate combinations (the combination must fit all three channels at once). A
    result is acceptable iff its three ratios are <= 1."""
    got = np.asarray(got, f64).reshape(-1, 3)
    ref, e = (lab.norm, lab.e_norm) if normalised else (lab.raw, lab.e_raw)
    ratio = np.abs(got - ref) / e
    und = np.nonzero(~lab.decided)[0]
    if len(und):
        sub = Lab(*(f[und] for f in lab))
        raw, norm, e_raw, e_norm = candidates(sub)
        cref, ce = (norm, e_norm) if normalised else (raw, e_raw)
        r = np.abs(got[und, None, :] - cref) / ce                                                # [m, 8, 3]
        best = r.max(2).argmin(1)
        ratio[und] = r[np.arange(len(und)), best]
    return ratio

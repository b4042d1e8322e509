"""FPFH-33 of fpfh.hip (k_fpfh_mark, k_spfh, k_fpfh_sum) against the float64 intervals of fpfh_ref.py (-m gpu) on the scenes of
fpfh_scenes.py. test_fpfh_cpu.py proves the reference, the margins and the scenes first.

The reference takes the neighbourhoods in float32 exactly as the library does, so counts and NaN rows are exact. Every deposit that
float64 can decide must be in its bin: a finite value lies in [lo - TOL, hi + TOL], TOL = 3.7e-4 (float32 sums; test_fpfh_cpu.py),
while one pair in a wrong bin, one dropped or one extra neighbour moves a value by at least min_move >= 4 TOL in the generic and the
count scenes. Where float64 cannot decide (the seam of f1, role ties, the signed zero) the device is held to the CPU oracle's row,
the one float32 evaluation order both restate. The fast pair arithmetic must give the bytes of the exact arithmetic.

Measured on the MI355X (largest excess over [lo, hi], undecided deposits of all deposits, smallest min_move of the scene):
  generic              8.61e-06, 31 of 127485, min_move 0.0166      f1_edges             6.33e-06, 150 of 990, min_move 0.0217
  f2_edges             2.74e-06, 150 of 990, min_move 0.0217        seam                 2.74e-06, 42 of 324, min_move 0.0217
  swap_tie             7.63e-06, 20 of 79326, min_move 0.00115      pole_and_degenerate  9.13e-06, 18 of 3570, min_move 0.0124 (2 exempt)
  queue_counts         4.25e-06, 0 of 2313, min_move 0.521          sum_counts           8.55e-06, 10 of 46317, min_move 0.00861
  exact_radius         2.8e-06, 0 of 252, min_move 0.0955           inexact_radius       2.46e-06, 0 of 252, min_move 0.0637
Largest difference from the oracle's row: seam 1.53e-05, swap_tie 3.81e-05, f2_edges 1.53e-05. Fast and exact arithmetic: equal bytes
on every scene and on the wide batch.
The seam scene caught a defect: pair_bins_fast called t1 near 0 and near 11 "sure", but for x < 0 the sign of y alone separates
bin 0 from bin 10 there -- the fast arithmetic read y = -0.0f as +pi (the signed-zero probe: 99.5 in bin 10 instead of bin 0) and
took the other sign than the exact arithmetic for a y at rounding-noise level (one of the turned objects). Such pairs now go to
the exact arithmetic.
Scratch builds of fpfh.hip that these tests fail, as they must: `d2 != 0` dropped from k_fpfh_sum (7 tests), FPFH_GUARD 0
(fast == exact on f1_edges), the queue drained at `qn_ >= 128` (queue_counts, swap_tie), the last partial batch taken with
`lane <= qn_` (all), `<=` instead of `<` on the radius in k_fpfh_mark, k_spfh or k_fpfh_sum (exact_radius and inexact_radius each).
Two changes are NOT observable and pass: draining at `qn_ > 64` (a block adds at most 64 entries, so the 128 slots still hold them
and the last batch is still <= 64) and queueing the point itself (`t != p` dropped: its pair has d = 0 and is skipped anyway)."""
import numpy as np
import pytest

import fpfh_scenes as sc
import frontend_scenes as fs
from test_fpfh_cpu import TOL, excess, oracle_rows

pytestmark = pytest.mark.gpu
_device = {}


def T(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def fpfh_on(pkg, gpu, objs, kps, cell, radius):
    """capi.fpfh33 of a ragged batch on the shared context -> (descriptors [K, 33] float32, counts [K])"""
    ctx, dev = gpu
    po, P, N, ko, KP = fs.soa(objs, kps)
    cloud = pkg.capi.Cloud(ctx, po, *[T(c, dev) for c in fs.cols(P)], *[T(c, dev) for c in fs.cols(N)], cell)
    try:
        d, c = pkg.capi.fpfh33(ctx, cloud, ko, *[T(c, dev) for c in fs.cols(KP)], radius, want_counts=True)
        return d.cpu().numpy(), c.cpu().numpy().astype(np.int64)
    finally:
        ctx.sync(); cloud.close()


def run(pkg, gpu, name):
    s = sc.scene(name)
    return fpfh_on(pkg, gpu, s["objs"], s["kps"], s["cell"], s["radius"])


def device_rows(pkg, gpu, name):
    """the scene by the default (fast + exact) arithmetic, once per process"""
    if name not in _device:
        _device[name] = run(pkg, gpu, name)
    return _device[name]


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_rows(ref, got, cnt):
    """device rows and counts against the intervals of fpfh_ref.Result: NaN rows as a whole, exact counts, every value of a keypoint that is
    not exempt inside [lo, hi] within TOL, block sums 0 or 100 -> the excesses"""
    assert np.array_equal(np.isnan(got).any(1), ref.nan) and np.array_equal(np.isnan(got).all(1), ref.nan)
    assert np.array_equal(cnt, ref.count)
    ex = excess(ref, got)
    assert ex.max(initial=0.0) <= TOL, np.argwhere(ex > TOL)[:10]
    sums = got[~ref.nan].reshape(-1, 3, 11).sum(2)
    zero = (ref.hi[~ref.nan].reshape(-1, 3, 11).sum(2) == 0) & ~ref.exempt[~ref.nan][:, None]
    assert (sums[zero] == 0).all()
    nonzero = ~zero & ~ref.exempt[~ref.nan][:, None]
    assert (np.abs(sums - 100) <= 1e-3)[nonzero].all()
    return ex


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_fpfh33_inside_the_float64_intervals(pkg, gpu, ora, name):
    ref = sc.reference(name)
    got, cnt = device_rows(pkg, gpu, name)
    ex = check_rows(ref, got, cnt)
    ok = ~ref.nan & ~ref.exempt
    print(f"{name}: largest excess {ex.max(initial=0.0):.3g}, undecided {int(ref.undecided.sum())} of {int(ref.deposits.sum())} deposits, "
          f"min_move {ref.min_move[ok].min(initial=np.inf):.3g}, exempt keypoints {int(ref.exempt.sum())}")
    # only the degenerate pairs exempt a keypoint from the intervals; there the oracle's row decides
    assert int(ref.exempt.sum()) == (len(sc.scene(name)["degenerate"]) if name == "pole_and_degenerate" else 0)
    if ref.exempt.any():
        want, _ = oracle_rows(ora, name)
        assert np.abs(got[ref.exempt] - want[ref.exempt]).max() <= TOL


@pytest.mark.parametrize("name", list(sc.SCENES) + ["wide-fused"])
def test_fast_bins_are_the_exact_bins(pkg, gpu, monkeypatch, name):
    """pair_bins_fast (v_rsq, v_rcp, a degree-13 arctangent) claims the reference's bins wherever it does not hand the pair to the
    exact arithmetic. ISMHIP_FPFH_DBG=2 sends EVERY pair through the exact arithmetic: the bytes must not change."""
    if name == "wide-fused":
        b = fs.wide_batch(fs.FUSED_SURFACE, with_color=False)
        args = (b["objs"], b["fpfh_kps"], fs.DENSE_CELL, fs.FPFH_RADIUS)
        fast = fpfh_on(pkg, gpu, *args)
    else:
        s = sc.scene(name)
        args = (s["objs"], s["kps"], s["cell"], s["radius"])
        fast = device_rows(pkg, gpu, name)
    monkeypatch.setenv("ISMHIP_FPFH_DBG", "2")
    exact = fpfh_on(pkg, gpu, *args)
    assert np.array_equal(fast[1], exact[1])
    diff = fast[0].view(np.uint32) != exact[0].view(np.uint32)
    assert not diff.any(), (int(diff.any(1).sum()), np.argwhere(diff)[:10], np.nanmax(np.abs(fast[0] - exact[0])))


@pytest.mark.parametrize("name", ["seam", "swap_tie", "f2_edges"])
def test_signed_zero_and_seam_follow_the_oracle(pkg, gpu, ora, name):
    """Where the float64 reference cannot decide, the oracle's float32 operation order does: y at rounding-noise level or -0.0f on
    the seam of f1 (bin 0 or bin 10), role ties (PCL's acos comparison does not swap on a tie), and f2 EXACTLY on its bin edges
    (the double-precision bin formula decides for the float32 below, at and above the edge)."""
    got, cnt = device_rows(pkg, gpu, name)
    want, wcnt = oracle_rows(ora, name)
    assert np.array_equal(cnt, wcnt) and np.array_equal(np.isnan(got), np.isnan(want))
    err = np.abs(got - want)
    print(f"{name}: largest difference from the oracle {np.nanmax(err):.3g}")
    assert np.nanmax(err) <= TOL, np.argwhere(err > TOL)[:10]
    if name == "seam":                                        # the signed-zero probe: y = -0.0f, x < 0 belongs to bin 0
        k = sc.arrays(name)[3][sc.scene(name)["zero_probe"]]
        assert want[k, 0] > 50 and got[k, 0] > 50


def test_copy_of_an_object_gives_the_same_bytes(pkg, gpu):
    """the flags and the SPFH rows live in the batch's index space base + t: a later copy of an object must not see the original's"""
    got, cnt = device_rows(pkg, gpu, "generic")
    ko = sc.arrays("generic")[3]
    a, b = sc.scene("generic")["copy"]
    assert ko[a + 1] - ko[a] == ko[b + 1] - ko[b] == 16
    assert same_bytes(got[ko[a]:ko[a + 1]], got[ko[b]:ko[b + 1]]) and np.array_equal(cnt[ko[a]:ko[a + 1]], cnt[ko[b]:ko[b + 1]])


def test_two_calls_give_the_same_bytes(pkg, gpu):
    first = device_rows(pkg, gpu, "generic")
    again = run(pkg, gpu, "generic")
    assert same_bytes(first[0], again[0]) and np.array_equal(first[1], again[1])

"""The perceptron on the MI355X (ismhip_mlp_create / ismhip_mlp_forward, csrc/mlp.hip) against the float64 pass of tests/cgf_ref.py: every
output within the bound derived there (any summation order, u = 2^-24, nothing measured), on dense weights and on the sparse ones for
which that bound is a small share of the outputs (cgf_scenes.random_layers says why both). Identical bytes from run to run, for any row
count around a row's place in its tile, and through capi.cgf's chunking."""
import numpy as np
import pytest

import cgf_ref as ref
import cgf_scenes as scenes

pytestmark = pytest.mark.gpu
F = np.float32

REAL = [2244, 512, 512, 512, 512, 40]
NETS = {                                            # name -> (widths, non-zeros per output or 0 for dense)
    "real dense": (REAL, 0),
    "real sparse": (REAL, scenes.MLP_NNZ),
    "D = 32": ([2244, 512, 512, 512, 512, 32], scenes.MLP_NNZ),
    "D = 1": ([2244, 512, 512, 512, 512, 1], scenes.MLP_NNZ),
    "ragged": ([2244, 48, 7], scenes.MLP_NNZ),
    "one layer, widest input": ([4096, 5], 0),
    "odd everywhere": ([13, 511, 3], 0),
}
ROWS = (1, 31, 33, 257)


@pytest.fixture(scope="module")
def nets(pkg, gpu):
    """name -> (layers, Mlp, x [257, in] with an all-zero row 0, float64 answer, bound), built once"""
    ctx, _dev = gpu
    out = {}
    for i, (name, (widths, nnz)) in enumerate(NETS.items()):
        rng = np.random.default_rng(900 + i)
        layers = scenes.random_layers(rng, widths, nnz)
        x = rng.normal(size=(max(ROWS), widths[0])).astype(F)
        x[0] = 0
        y, e = ref.mlp(x, layers)
        out[name] = (layers, pkg.capi.Mlp(ctx, layers), x, y, e)
    yield out
    for _l, m, _x, _y, _e in out.values():
        m.close()


def _forward(gpu, mlp, x):
    import torch
    ctx, dev = gpu
    y = mlp.forward(torch.as_tensor(np.ascontiguousarray(x)).to(dev))
    ctx.sync()
    return y.cpu().numpy()


@pytest.mark.parametrize("name", list(NETS))
def test_outputs_lie_within_the_derived_bound(gpu, nets, name):
    layers, mlp, x, y, e = nets[name]
    assert (mlp.n_in, mlp.n_out) == (layers[0][0].shape[0], layers[-1][0].shape[1])
    full = _forward(gpu, mlp, x)
    assert full.shape == y.shape and full.dtype == np.float32
    err = np.abs(full.astype(np.float64) - y)
    spread = np.abs(y[1:] - y[1:].mean(0)).max()
    print("%s: largest error %.3g, %.3g of its bound; largest bound %.3g; the outputs vary by %.3g over the rows" % (name, err.max(), (err / e).max(), e.max(), spread))
    assert (err <= e).all()
    # an all-zero input row: the bias path, the same for every net input
    zero = ref.mlp(np.zeros((1, x.shape[1])), layers)[0][0]
    assert (np.abs(full[0] - zero) <= e[0]).all()
    for n in ROWS:                                  # a row's bytes do not depend on how many rows follow it
        part = _forward(gpu, mlp, x[:n])
        assert part.shape == (n, y.shape[1]) and np.array_equal(part.view(np.uint32), full[:n].view(np.uint32)), n
    assert np.array_equal(_forward(gpu, mlp, x).view(np.uint32), full.view(np.uint32))            # two runs
    shifted = _forward(gpu, mlp, x[5:70])           # nor on where the row sits in its tile
    assert np.array_equal(shifted.view(np.uint32), full[5:70].view(np.uint32))


def test_relu_cuts_about_half_on_the_real_shape(nets):
    layers, _m, x, _y, _e = nets["real dense"]
    hidden = x[1:].astype(np.float64) @ layers[0][0] + layers[0][1]
    assert 0.4 < (hidden < 0).mean() < 0.6


def test_nan_rows_stay_nan_and_alone(gpu, nets):
    _layers, mlp, x, _y, _e = nets["ragged"]
    x = x[:70].copy()
    x[33, 100] = np.nan
    got = _forward(gpu, mlp, x)
    assert np.isnan(got[33]).all() and np.isfinite(np.delete(got, 33, axis=0)).all()


def test_create_refusals(pkg, gpu):
    ctx, _dev = gpu
    z = lambda a, b: (np.zeros((a, b), F), np.zeros(b, F), True)
    for layers, word in (([z(4097, 4)], "width out of range"), ([z(4, 513)], "width out of range"), ([z(8, 4), z(5, 3)], "inconsistent widths"),
                         ([z(4, 4)] * 9, "layer count")):
        with pytest.raises(pkg.capi.IsmHipError, match="mlp_create: " + word):
            pkg.capi.Mlp(ctx, layers)


def test_cgf_rows_do_not_depend_on_the_chunk_size(pkg, gpu, tmp_path):
    """capi.cgf end to end on scene 1 with a file-loaded net: three chunk sizes, the same bytes; the rows within the bound of the
    device's own raw rows"""
    import torch
    ctx, dev = gpu
    s = scenes.scene(1)
    layers = scenes.random_layers(np.random.default_rng(77), [ref.DIM, 48, 32], scenes.MLP_NNZ)
    path = str(tmp_path / "net.cgfw")
    pkg.capi.cgfw_write(path, layers)
    mlp = pkg.capi.Mlp.from_file(ctx, path, ref.DIM)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    x, y, z = (t(s["xyz"][:, i]) for i in range(3))
    kx, ky, kz = (t(s["kp"][:, i]) for i in range(3))
    R, rmin, rl = pkg.capi.cgf_radii(s["radius"])
    cloud = pkg.capi.Cloud(ctx, s["pt_off"], x, y, z, x, y, z, 0.4 * R)
    rows = [pkg.capi.cgf(ctx, cloud, s["kp_off"], kx, ky, kz, s["radius"], mlp, chunk_rows=c, want_counts=True) for c in (32768, 7, 20)]
    got = [(r.cpu().numpy(), c.cpu().numpy()) for r, c in rows]
    for r, c in got[1:]:
        assert np.array_equal(r.view(np.uint32), got[0][0].view(np.uint32)) and np.array_equal(c, got[0][1])
    lrf = pkg.capi.shot_lrf(ctx, cloud, s["kp_off"], kx, ky, kz, rl)
    n = pkg.capi.keypoint_normals_pca(ctx, cloud, s["kp_off"], kx, ky, kz, 0.1 * R)
    raw = pkg.capi.cgf_raw(ctx, cloud, s["kp_off"], kx, ky, kz, lrf, *n, R, rmin).cpu().numpy()
    want, e = ref.mlp(raw, layers)
    assert got[0][0].shape == (len(s["kp"]), 32) and (np.abs(got[0][0] - want) <= e).all()
    cloud.close(); mlp.close()

#!/usr/bin/env python3
"""Converts the weights of a CGF embedding between an .npz with arrays w1..wL, b1..bL and the .cgfw container that the library and the
C++ host read (include/ismhip.h: "CGFW", version 1, layer count; per layer in, out, activation, float32 W[in][out], float32 b[out]; little
endian).

    python tools/cgf_weights.py to-cgfw weights.npz embed_model_910000.cgfw [--linear-last | --relu-all]
    python tools/cgf_weights.py to-npz embed_model_910000.cgfw weights.npz
    python tools/cgf_weights.py info embed_model_910000.cgfw

w{l} is [in, out] as TensorFlow stores a dense layer's kernel, b{l} is [out]. The embedding of third_party/cgf/embedding.py:103-108 applies
ReLU after every layer but the last, which is the default here (--linear-last); an optional int array `relu` [L] in the .npz overrides it.
INTEGRATION.md says how the arrays are dumped from the reference's embed_model_910000.ckpt. The reader below refuses what the library's
loader refuses, with the same names; numpy only, no device."""
import argparse
import struct
import sys

import numpy as np

MAGIC, VERSION, MAX_LAYERS, MAX_IN, MAX_OUT = b"CGFW", 1, 8, 4096, 512


class CgfwError(ValueError):
    pass


def write_cgfw(path, layers):
    """layers: [(W [in, out], b [out], relu), ...]"""
    check_layers(layers)
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<II", VERSION, len(layers)))
        for W, b, relu in layers:
            W = np.ascontiguousarray(W, "<f4"); b = np.ascontiguousarray(b, "<f4")
            f.write(struct.pack("<III", W.shape[0], W.shape[1], 1 if relu else 0))
            f.write(W.tobytes()); f.write(b.tobytes())


def check_layers(layers, expect_in=0):
    if not 1 <= len(layers) <= MAX_LAYERS:
        raise CgfwError("layer count %d outside 1 .. 8" % len(layers))
    prev = None
    for l, (W, b, _relu) in enumerate(layers):
        W = np.asarray(W); b = np.asarray(b)
        if W.ndim != 2 or b.shape != (W.shape[1],):
            raise CgfwError("layer %d: inconsistent widths (W must be [in, out], b [out])" % (l + 1))
        if not (1 <= W.shape[0] <= MAX_IN and 1 <= W.shape[1] <= MAX_OUT):
            raise CgfwError("layer %d: width out of range (in 1 .. 4096, out 1 .. 512)" % (l + 1))
        if l == 0 and expect_in and W.shape[0] != expect_in:
            raise CgfwError("first layer width %d, not %d" % (W.shape[0], expect_in))
        if prev is not None and W.shape[0] != prev:
            raise CgfwError("layer %d: inconsistent widths" % (l + 1))
        if not (np.isfinite(W).all() and np.isfinite(b).all()):
            raise CgfwError("layer %d: non-finite weight" % (l + 1))
        prev = W.shape[1]


def read_cgfw(path, expect_in=0):
    data = open(path, "rb").read()
    if len(data) < 4:
        raise CgfwError("truncated file")
    if data[:4] != MAGIC:
        raise CgfwError("wrong magic")
    if len(data) < 12:
        raise CgfwError("truncated file")
    version, n = struct.unpack_from("<II", data, 4)
    if version != VERSION:
        raise CgfwError("unsupported version %d" % version)
    if not 1 <= n <= MAX_LAYERS:
        raise CgfwError("layer count %d outside 1 .. 8" % n)
    at, layers = 12, []
    for l in range(n):
        if len(data) < at + 12:
            raise CgfwError("truncated file")
        n_in, n_out, act = struct.unpack_from("<III", data, at); at += 12
        if not (1 <= n_in <= MAX_IN and 1 <= n_out <= MAX_OUT):
            raise CgfwError("layer %d: width out of range (in 1 .. 4096, out 1 .. 512)" % (l + 1))
        if l == 0 and expect_in and n_in != expect_in:
            raise CgfwError("first layer width %d, not %d" % (n_in, expect_in))
        if layers and n_in != layers[-1][0].shape[1]:
            raise CgfwError("layer %d: inconsistent widths" % (l + 1))
        if act > 1:
            raise CgfwError("layer %d: unknown activation" % (l + 1))
        nb = 4 * (n_in * n_out + n_out)
        if len(data) < at + nb:
            raise CgfwError("layer %d: truncated file" % (l + 1))
        W = np.frombuffer(data, "<f4", n_in * n_out, at).reshape(n_in, n_out).astype(np.float32); at += 4 * n_in * n_out
        b = np.frombuffer(data, "<f4", n_out, at).astype(np.float32); at += 4 * n_out
        if not (np.isfinite(W).all() and np.isfinite(b).all()):
            raise CgfwError("layer %d: non-finite weight" % (l + 1))
        layers.append((W, b, bool(act)))
    if at != len(data):
        raise CgfwError("trailing bytes")
    return layers


def layers_from_npz(path, relu_all=False):
    z = np.load(path)
    n = 0
    while "w%d" % (n + 1) in z.files:
        n += 1
    if n == 0 or any("b%d" % (l + 1) not in z.files for l in range(n)):
        raise CgfwError("the .npz needs arrays w1..wL and b1..bL")
    relu = [bool(v) for v in z["relu"]] if "relu" in z.files else [relu_all or l + 1 < n for l in range(n)]
    if len(relu) != n:
        raise CgfwError("relu must hold one flag per layer")
    return [(np.asarray(z["w%d" % (l + 1)], np.float32), np.asarray(z["b%d" % (l + 1)], np.float32).reshape(-1), relu[l]) for l in range(n)]


def layers_to_npz(path, layers):
    arrays = {"relu": np.asarray([1 if r else 0 for _w, _b, r in layers], np.int32)}
    for l, (W, b, _r) in enumerate(layers):
        arrays["w%d" % (l + 1)] = W; arrays["b%d" % (l + 1)] = b
    np.savez(path, **arrays)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("to-cgfw"); a.add_argument("npz"); a.add_argument("cgfw")
    g = a.add_mutually_exclusive_group()
    g.add_argument("--linear-last", action="store_true", help="ReLU on every layer but the last (default)")
    g.add_argument("--relu-all", action="store_true", help="ReLU on every layer")
    b = sub.add_parser("to-npz"); b.add_argument("cgfw"); b.add_argument("npz")
    c = sub.add_parser("info"); c.add_argument("cgfw")
    args = ap.parse_args(argv)
    try:
        if args.cmd == "to-cgfw":
            write_cgfw(args.cgfw, layers_from_npz(args.npz, relu_all=args.relu_all))
        elif args.cmd == "to-npz":
            layers_to_npz(args.npz, read_cgfw(args.cgfw))
        else:
            for l, (W, _b, r) in enumerate(read_cgfw(args.cgfw)):
                print("layer %d: %d -> %d, %s" % (l + 1, W.shape[0], W.shape[1], "ReLU" if r else "identity"))
    except CgfwError as e:
        print("cgf_weights: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""ctypes access to the host library's global-verification exports (capi_host.cpp: ism3d_global_features_get / _set, ism3d_last_global,
ism3d_classify_knn, ism3d_merge_sequence) on a host_binding.Model, and the translation of their arrays into global_ref's objects."""
import ctypes as C

import numpy as np

import global_ref as gr
import host_binding as hb

EXPORTS = ["ism3d_global_features_get", "ism3d_global_features_set", "ism3d_last_global", "ism3d_classify_knn", "ism3d_merge_sequence"]
_p = hb._p


def global_features(m):
    """the stored global features of a model -> dict(cls, cloud, inst [n], rf [n, 9], desc [n, dim], radius [n], n_clouds)"""
    dim, clouds = C.c_int(), C.c_int()
    n = m.L.ism3d_global_features_get(m.h, C.byref(dim), C.byref(clouds), *([None] * 6))
    m._ck(min(n, 0), "global_features_get")
    out = dict(cls=np.zeros(n, np.uint32), cloud=np.zeros(n, np.uint32), inst=np.zeros(n, np.uint32), rf=np.zeros((n, 9), np.float32),
               desc=np.zeros((n, dim.value), np.float32), radius=np.zeros(n, np.float32))
    m.L.ism3d_global_features_get(m.h, None, None, *[_p(out[k]) for k in ("cls", "cloud", "inst", "rf", "desc", "radius")])
    out["n_clouds"] = clouds.value
    return out


def set_global_features(m, cls, inst, rf, desc, radius):
    desc, rf, radius = hb._f(desc), hb._f(rf), hb._f(radius)                       # named: the arrays must outlive the call
    cls, inst = np.ascontiguousarray(cls, np.uint32), np.ascontiguousarray(inst, np.uint32)
    m._ck(m.L.ism3d_global_features_set(m.h, desc.shape[0], desc.shape[1], _p(cls), _p(inst), _p(rf), _p(desc), _p(radius)), "global_features_set")


def last_global(m):
    """the global step of the last detect_batch -> dict (see ism3d_last_global)"""
    k, dim, n_obj, n_max = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    n = m.L.ism3d_last_global(m.h, C.byref(k), C.byref(dim), C.byref(n_obj), C.byref(n_max), *([None] * 16))
    m._ck(min(n, 0), "last_global")
    K, D, O, M = k.value, dim.value, max(n_obj.value, 0), n_max.value
    out = dict(region_obj=np.zeros(n, np.int32), region_max=np.zeros(n, np.int32), n_sel=np.zeros(n, np.uint32), centroid=np.zeros((n, 3), np.float32),
               radius=np.zeros(n, np.float32), desc=np.zeros((n, D), np.float32), knn_idx=np.zeros((n, K), np.int32), knn_dist=np.zeros((n, K), np.float32),
               hyp_id=np.zeros((n, 2), np.uint32), hyp_w=np.zeros((n, 2), np.float32), max_off=np.zeros(O + 1, np.uint32), max_cls=np.zeros(M, np.int32),
               max_inst=np.zeros(M, np.int32), max_w=np.zeros(M, np.float32), max_iw=np.zeros(M, np.float32), max_pos=np.zeros((M, 3), np.float32))
    keys = ["region_obj", "region_max", "n_sel", "centroid", "radius", "desc", "knn_idx", "knn_dist", "hyp_id", "hyp_w", "max_off", "max_cls", "max_inst",
            "max_w", "max_iw", "max_pos"]
    m.L.ism3d_last_global(m.h, None, None, None, None, *[_p(out[k]) for k in keys])
    out["k"], out["dim"] = K, D
    return out


def classify_knn(n_class, n_inst, n_dist, max_class, single_object_mode):
    L = hb.lib()
    ids, w = np.zeros(2, np.uint32), np.zeros(2, np.float32)
    nc, ni, nd = np.ascontiguousarray(n_class, np.uint32), np.ascontiguousarray(n_inst, np.uint32), hb._f(n_dist)
    rc = L.ism3d_classify_knn(len(nc), _p(nc), _p(ni), _p(nd), C.c_uint32(max_class), int(single_object_mode), _p(ids), _p(w))
    assert rc == 0, L.ism3d_last_error()
    return int(ids[0]), float(w[0]), int(ids[1]), float(w[1])


def merge_sequence(fn, maxima, radius, min_threshold=0.0, best_k=-1, min_svm_score=0.70, rate_limit=0.60, weight_factor=1.5):
    """the host library's merge sequence on a list of global_ref.Maximum -> a new list"""
    L = hb.lib()
    n = len(maxima)
    ids = np.array([[m.cls, m.inst] for m in maxima], np.uint32).reshape(n, 2)
    w = np.array([[m.weight, m.inst_weight] for m in maxima], np.float32).reshape(n, 2)
    pos = np.array([m.pos for m in maxima], np.float32).reshape(n, 3)
    hid = np.array([[m.g_cls, m.g_inst] for m in maxima], np.uint32).reshape(n, 2)
    hw = np.array([[m.g_weight, m.g_inst_weight] for m in maxima], np.float32).reshape(n, 2)
    roi = np.array([m.roi for m in maxima], np.float32).reshape(n, 3)
    params = np.asarray([radius, min_threshold, best_k, min_svm_score, rate_limit, weight_factor], np.float32)
    k = L.ism3d_merge_sequence(int(fn), n, _p(ids), _p(w), _p(pos), _p(hid), _p(hw), _p(roi), _p(params))
    assert k >= 0, L.ism3d_last_error()
    return [gr.Maximum(ids[i, 0], w[i, 0], ids[i, 1], w[i, 1], pos[i], (hid[i, 0], hw[i, 0], hid[i, 1], hw[i, 1]), roi[i]) for i in range(k)]

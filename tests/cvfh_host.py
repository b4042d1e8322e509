"""ctypes access to the host exports that several rows per region need (capi_host.cpp: ism3d_global_features_set_clouds,
ism3d_last_global_rows) on a host_binding.Model; global_host.py covers the one-row exports."""
import ctypes as C

import numpy as np

import host_binding as hb

_p = hb._p
CVFH = {"Type": "CVFH", "Parameters": {"CvfhClusterTolerance": 0.08, "CvfhNormalRadius": 0.12, "CvfhMinPoints": 50}}


def set_global_features(m, cls, cloud, inst, rf, desc, radius):
    """rows with their training cloud: rows of one cloud are consecutive"""
    desc, rf, radius = hb._f(desc), hb._f(rf), hb._f(radius)
    cls, cloud, inst = (np.ascontiguousarray(a, np.uint32) for a in (cls, cloud, inst))
    m._ck(m.L.ism3d_global_features_set_clouds(m.h, desc.shape[0], desc.shape[1], _p(cls), _p(cloud), _p(inst), _p(rf), _p(desc), _p(radius)),
          "global_features_set_clouds")


def last_global(m):
    """the global step of the last detect_batch with per-ROW desc, knn_idx, knn_dist and row_off [regions + 1]"""
    k, dim, n_obj, n_max = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    n = m.L.ism3d_last_global(m.h, C.byref(k), C.byref(dim), C.byref(n_obj), C.byref(n_max), *([None] * 16))
    m._ck(min(n, 0), "last_global")
    row_off = np.zeros(n + 1, np.uint32)
    T = m.L.ism3d_last_global_rows(m.h, _p(row_off))
    m._ck(min(T, 0), "last_global_rows")
    K, D, O, M = k.value, dim.value, max(n_obj.value, 0), n_max.value
    out = dict(region_obj=np.zeros(n, np.int32), region_max=np.zeros(n, np.int32), n_sel=np.zeros(n, np.uint32), centroid=np.zeros((n, 3), np.float32),
               radius=np.zeros(n, np.float32), desc=np.zeros((T, D), np.float32), knn_idx=np.zeros((T, K), np.int32), knn_dist=np.zeros((T, K), np.float32),
               hyp_id=np.zeros((n, 2), np.uint32), hyp_w=np.zeros((n, 2), np.float32), max_off=np.zeros(O + 1, np.uint32), max_cls=np.zeros(M, np.int32),
               max_inst=np.zeros(M, np.int32), max_w=np.zeros(M, np.float32), max_iw=np.zeros(M, np.float32), max_pos=np.zeros((M, 3), np.float32))
    keys = ["region_obj", "region_max", "n_sel", "centroid", "radius", "desc", "knn_idx", "knn_dist", "hyp_id", "hyp_w", "max_off", "max_cls", "max_inst",
            "max_w", "max_iw", "max_pos"]
    m.L.ism3d_last_global(m.h, None, None, None, None, *[_p(out[k]) for k in keys])
    out["k"], out["dim"], out["row_off"] = K, D, row_off
    return out


def classify_rows(stored_cls, stored_inst, knn_idx, knn_dist, max_class, single):
    """GlobalClassifier::classifyWithKNN (global_classifier.cpp:242-347) restated directly: the loop over the query rows feeds ONE
    accumulator (float32 score sums in arrival order), then the decision -> (class, class weight, instance, instance weight)"""
    f32 = np.float32
    votes = {}
    for idx_row, dist_row in zip(knn_idx, knn_dist):
        for i, d in zip(idx_row, dist_row):
            score = f32(np.exp(-np.sqrt(f32(d), dtype=f32), dtype=f32))
            acc = votes.setdefault(int(stored_cls[i]), dict(n=0, score=f32(0), inst={}))
            acc["n"] += 1
            acc["score"] = f32(acc["score"] + score)
            e = acc["inst"].setdefault(int(stored_inst[i]), [0, f32(0)])
            e[0] += 1
            e[1] = f32(e[1] + score)
    cls, cw, inst, iw = max_class, f32(0), 0xffffffff, f32(0)

    def best_instance(acc):
        best, who = 0, None
        for k in sorted(acc["inst"]):
            if acc["inst"][k][0] > best:
                best, who = acc["inst"][k][0], k
        return who, f32(acc["inst"][who][1] / f32(acc["inst"][who][0]))

    if single:
        best = 0
        for c in sorted(votes):
            if votes[c]["n"] > best:
                best, cls = votes[c]["n"], c
        cw = f32(votes[cls]["score"] / f32(votes[cls]["n"]))
        inst, iw = best_instance(votes[cls])
    elif max_class in votes:
        cw = f32(votes[max_class]["score"] / f32(votes[max_class]["n"]))
        inst, iw = best_instance(votes[max_class])
    return cls, float(cw), inst, float(iw)

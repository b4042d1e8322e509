// vfh_deposit.h -- what k_vfh (global.hip) and k_cvfh_rows (cvfh.hip) share: the span sweep, the bin rule and the per-point deposit of the
// viewpoint-feature histogram (include/ismhip.h states the arithmetic under ismhip_global_vfh). Included at file scope.
#pragma once
#include "common.h"
#include "pair_features.h"

namespace {

#define VFH_COPIES 8
#define VFH_SHAPE_BINS 45
#define VFH_VP_BINS 128

// floor(v) clamped to [0, last] as a bin index; -1 for a NaN (no deposit). The clamp is taken in double: no int conversion of a
// value outside int.
__device__ __forceinline__ int vfh_bin(double v, int last) {
    if (!(v == v)) return -1;
    v = floor(v);
    return v < 0.0 ? 0 : (v > (double)last ? last : (int)v);
}

// One sweep of a region's span, position and (with NORMALS) normal of each record, in the order i = tid, tid + 256, ... per thread (the
// order of the double sums). The loop of k_global issues one load and waits for it, ~64 dependent round trips per sweep of a
// 16 384-point object with one wave per SIMD; here four records' loads (eight with normals) are issued before the first is used.
// Without NORMALS sn is not read and f gets a zero normal. k_vfh, k_gasd and the kernels of cvfh.hip sweep with it.
template <bool NORMALS, class F>
__device__ __forceinline__ void span_sweep(const float4* __restrict__ sp, const float4* __restrict__ sn, uint32_t n, int tid, F&& f) {
    for (uint32_t i0 = tid; i0 < n; i0 += 4 * 256) {
        float4 p[4], nr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t i = (uint64_t)i0 + 256u * j;                          // past the end: a record that is there, not used
            p[j] = sp[i < n ? i : i0];
            if constexpr (NORMALS) nr[j] = sn[i < n ? i : i0]; else nr[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) if ((uint64_t)i0 + 256u * j < n) f(p[j], nr[j]);
    }
}

// The deposits of ONE selected point p with normal nr into a 308-bin integer histogram, against the centroid c, the normal nc and the
// unit view direction vd: the viewpoint block for every finite normal, the four shape blocks from pcl::computePairFeatures(c, nc, p, n).
// bin4(f4) gives the bin of the distance block (-1: no deposit): the one place where VFH and CVFH differ.
template <class B4>
__device__ __forceinline__ void vfh_deposit(uint32_t* hist, float cx, float cy, float cz, float ncx, float ncy, float ncz,
                                            float vdx, float vdy, float vdz, const float4& p, const float4& nr, B4&& bin4) {
    if (!(isfinite(nr.x) && isfinite(nr.y) && isfinite(nr.z))) return;
    const double dpi = (double)(1.0f / (2.0f * (float)M_PI));
    // viewpoint block: every such point, whatever becomes of its pair
    const float dv = (nr.x * vdx + nr.y * vdy) + nr.z * vdz;
    const int bv = vfh_bin((((double)dv + 1.0) * 0.5) * (double)VFH_VP_BINS, VFH_VP_BINS - 1);
    if (bv >= 0) atomicAdd(&hist[4 * VFH_SHAPE_BINS + bv], 1u);
    // shape blocks: computePairFeatures(centroid, normal centroid, p, n); f4 is its own first expression
    float f1, f2, f3;
    if (!pair_features(cx, cy, cz, ncx, ncy, ncz, p.x, p.y, p.z, nr.x, nr.y, nr.z, f1, f2, f3)) return;
    const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
    const float f4 = sqrtf((dx * dx + dy * dy) + dz * dz);
    const int b1 = vfh_bin((double)VFH_SHAPE_BINS * (((double)f1 + M_PI) * dpi), VFH_SHAPE_BINS - 1);
    const int b2 = vfh_bin((double)VFH_SHAPE_BINS * (((double)f2 + 1.0) * 0.5), VFH_SHAPE_BINS - 1);
    const int b3 = vfh_bin((double)VFH_SHAPE_BINS * (((double)f3 + 1.0) * 0.5), VFH_SHAPE_BINS - 1);
    const int b4 = bin4(f4);
    if (b1 >= 0) atomicAdd(&hist[b1], 1u);
    if (b2 >= 0) atomicAdd(&hist[VFH_SHAPE_BINS + b2], 1u);
    if (b3 >= 0) atomicAdd(&hist[2 * VFH_SHAPE_BINS + b3], 1u);
    if (b4 >= 0) atomicAdd(&hist[3 * VFH_SHAPE_BINS + b4], 1u);
}

// the view direction: (viewpoint - centroid) / |.| in float; a zero norm leaves 0
__device__ __forceinline__ void vfh_view_direction(float vpx, float vpy, float vpz, float cx, float cy, float cz, float& vdx, float& vdy, float& vdz) {
    vdx = vpx - cx; vdy = vpy - cy; vdz = vpz - cz;
    const float vn = sqrtf((vdx * vdx + vdy * vdy) + vdz * vdz);
    if (vn != 0.0f) { vdx /= vn; vdy /= vn; vdz /= vn; }
}

}  // namespace

// pair_features.h — pcl::computePairFeatures (PCL 1.10) in float, written once for the two descriptors built on
// it: FPFH-33 (fpfh.hip: k_spfh) and CoSPAIR (cospair.hip: k_cospair). Two evaluations of the same three Darboux features of a pair
// (source p with normal pn, target q with normal qn): the reference's own float sequence, and a fast one that says when it cannot be
// trusted. Each descriptor keeps its own bin formulas and its own guard against its own bin edges.
#pragma once
#include "common.h"

#ifdef __HIPCC__
// pcl::computePairFeatures in float; returns false when the pair is degenerate (PCL then zeroes its outputs; here f1..f3 are left
// as they are and the caller decides: FPFH skips the pair, CoSPAIR deposits f = 0). A caller that holds the difference d = q - p
// already passes p = 0 and q = d: d - 0 is d, bit for bit.
__device__ __forceinline__ bool pair_features(float px, float py, float pz, float pnx, float pny, float pnz,
                                              float qx, float qy, float qz, float qnx, float qny, float qnz,
                                              float& f1, float& f2, float& f3) {
    float dx = qx - px, dy = qy - py, dz = qz - pz;
    const float f4 = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (f4 == 0.0f) return false;
    float ax = pnx, ay = pny, az = pnz, bx = qnx, by = qny, bz = qnz;
    const float angle1 = ((ax * dx + ay * dy) + az * dz) / f4;
    const float angle2 = ((bx * dx + by * dy) + bz * dz) / f4;
    // PCL swaps the roles when acos|a1| > acos|a2|. acos is decreasing with |slope| >= 1, so when the two absolute cosines differ
    // by more than 1e-5 (hundreds of float acosf errors) the order of the acos values is the reverse order of the cosines and no
    // acosf is needed; inside that band (and only there) the reference's own comparison of the two acosf values decides.
    const float c1 = fabsf(angle1), c2 = fabsf(angle2);
    const float gap = c2 - c1;
    const bool swap_roles = fabsf(gap) > 1e-5f ? gap > 0.f : acosf(c1) > acosf(c2);
    if (swap_roles) {
        float t;
        t = ax; ax = bx; bx = t; t = ay; ay = by; by = t; t = az; az = bz; bz = t;
        dx = -dx; dy = -dy; dz = -dz;
        f3 = -angle2;
    } else f3 = angle1;
    float vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;
    const float vn = sqrtf((vx * vx + vy * vy) + vz * vz);
    if (vn == 0.0f) return false;
    vx /= vn; vy /= vn; vz /= vn;
    const float wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;
    f2 = (vx * bx + vy * by) + vz * bz;
    f1 = atan2f((wx * bx + wy * by) + wz * bz, (ax * bx + ay * by) + az * bz);
    return true;
}

// arctangent by a degree-13 odd polynomial: max error 6.6e-7 rad over [0, 1], fitted and checked in tests/test_host_cpu.py
__device__ __forceinline__ float fast_atan2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float a = mn * __builtin_amdgcn_rcpf(mx);                     // 0/0 -> NaN: the caller's guard test fails and the exact path runs
    const float z = a * a;
    float p = 0.008097294718027115f;
    p = fmaf(p, z, -0.037751708179712296f); p = fmaf(p, z, 0.08475969731807709f); p = fmaf(p, z, -0.13537675142288208f);
    p = fmaf(p, z, 0.19895026087760925f); p = fmaf(p, z, -0.3332797586917877f); p = fmaf(p, z, 0.9999997019767761f);
    float r = a * p;
    r = ay > ax ? 1.57079632679489662f - r : r;
    r = x < 0.f ? 3.14159265358979323846f - r : r;
    return y < 0.f ? -r : r;
}

// The same three features by FAST arithmetic (v_rsq_f32 / v_rcp_f32 instead of sqrt + IEEE divisions, fast_atan2);
// x = the cosine argument of the arctangent (the callers need its sign at the +-pi seam of f1). The features differ from the exact
// ones by a few 1e-6. False -- the caller takes the exact path -- for coincident points, a near tie of the two cosines (or NaN:
// the exact path decides the roles), a degenerate cross product and near the pole of the arctangent. The role swap (which decides
// everything downstream) is otherwise taken exactly as in pair_features.
__device__ __forceinline__ bool pair_features_fast(float px, float py, float pz, float pnx, float pny, float pnz,
                                                   float qx, float qy, float qz, float qnx, float qny, float qnz,
                                                   float& f1, float& f2, float& f3, float& x) {
    float dx = qx - px, dy = qy - py, dz = qz - pz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 == 0.0f) return false;                                       // coincident points: the exact path's business
    const float inv_f4 = __builtin_amdgcn_rsqf(d2);
    float ax = pnx, ay = pny, az = pnz, bx = qnx, by = qny, bz = qnz;
    // the swap test needs the reference's own angle values near a tie: exact division there, reciprocal elsewhere
    const float dot1 = (ax * dx + ay * dy) + az * dz, dot2 = (bx * dx + by * dy) + bz * dz;
    float angle1 = dot1 * inv_f4, angle2 = dot2 * inv_f4;
    const float gapf = fabsf(angle2) - fabsf(angle1);
    if (!(fabsf(gapf) > 1e-4f)) return false;                           // near tie of the two cosines (or NaN): exact path decides the roles
    float f3_;
    if (gapf > 0.f) {
        float t;
        t = ax; ax = bx; bx = t; t = ay; ay = by; by = t; t = az; az = bz; bz = t;
        dx = -dx; dy = -dy; dz = -dz;
        f3_ = -angle2;
    } else f3_ = angle1;
    float vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;
    const float vn2 = (vx * vx + vy * vy) + vz * vz;
    if (!(vn2 > 1e-30f)) return false;                                  // degenerate (or denormal): exact path
    const float inv_vn = __builtin_amdgcn_rsqf(vn2);
    vx *= inv_vn; vy *= inv_vn; vz *= inv_vn;
    const float wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;
    const float f2_ = (vx * bx + vy * by) + vz * bz;
    const float ay_ = (wx * bx + wy * by) + wz * bz, ax_ = (ax * bx + ay * by) + az * bz;
    // the arctangent is only as well conditioned as |(x, y)| is large: the two arguments carry ~3e-7 of fast-arithmetic error, which
    // is 1.5e-5 rad = 2.6e-5 of an FPFH bin at |(x, y)| = 0.02 (unit normals: |(x, y)|^2 = 1 - f2^2); closer to the pole the exact path runs
    if (!((ax_ * ax_ + ay_ * ay_) > 4e-4f)) return false;
    f1 = fast_atan2(ay_, ax_); f2 = f2_; f3 = f3_; x = ax_;
    return true;
}
#endif

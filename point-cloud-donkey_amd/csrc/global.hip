// global.hip — region descriptors: the global features of the reference's "extended pipeline" (UseGlobalFeatures), one 256-thread
// workgroup per REGION = (object, selection centre, selection radius). Reference seams: FeaturesSHORTSHOTGlobal::iComputeDescriptors /
// compute_descriptor (features/features_short_shot_global.cpp:36-165) and FeaturesSHOTGlobal::iComputeDescriptors
// (features/features_shot_global.cpp:27-99), both on the cloud Voting hands them: the whole object (training, single-object mode) or the
// points inside a ball round a maximum (voting.cpp:217-239).
//
// The shape is not that of the per-keypoint kernels (one wave per keypoint, one radius per call): there is ONE keypoint per region, the
// centroid of the selected points; its support is every selected point; the radius is the region's own (the largest distance from that
// centroid). So the workgroup STREAMS the object's cell-sorted span sp4 (coalesced float4 loads, the selection predicate evaluated on
// the fly; the grid is not used) once per step, all steps in one kernel:
//   1. count + coordinate sums (double)          -> n_sel, centroid      (a whole-object region takes both from the cloud's GridMeta:
//                                                                          bit-equal to ismhip_cloud_centroids by construction)
//   2. max |p - centroid| (k_cloud_radii's float arithmetic; max is order-free: bit-equal to ismhip_cloud_radii for a whole object)
//   3. k_lrf_cov's weighted covariance in double -> eigen3.h on one thread -> axis candidates
//   4. the two sign votes (integers); on a tie the five median neighbours by (d^2, original index) decide, found by bitwise bisection
//      over the 64-bit keys with one more sweep of the span per bit -- no key store, so the region may hold any number of points
//   5. the histogram: per-wave LDS copies of INTEGER bins (counts, or SHOT's 2^-28 fixed point), merged as integers, then the norm
// Every reduction is a fixed-order tree in double (per thread in index order, DPP wave sum, the four waves in order: block_sum_d_left, common.h) or an integer sum;
// there is no float atomic: two calls give the same bits in every output.
//
// Byte model per region: 5 sweeps x 16 B x n_obj_points (6 for SHOT-352: + 16 B per descriptor neighbour for its normal), the first
// from HBM, the later ones from L2 when the object's span fits (a 16 384-point object: 256 KiB); a tie adds ~50 sweeps from L2.
// One region per workgroup: a region of a very large object is not split over several workgroups.
// k_vfh (further down) is the frame-free third descriptor on the same regions: ismhip_global_vfh.
// k_gasd (after it) is the fourth, in the region's own covariance frame and with colour: ismhip_global_gasd.
// The clustered fifth, ismhip_global_cvfh, is cvfh.hip; it shares vfh_deposit.h with k_vfh.
#include "shot_deposit.h"
#include "lrf_common.h"
#include "eigen3.h"
#include "pair_features.h"
#include "vfh_deposit.h"

namespace {

#define GLOBAL_SSHOT_RAD2DEG 57.29578     /* pcl::rad2deg(double) of PCL 1.10 multiplies by this truncated constant (external) */

struct GlobalArgs {
    const uint32_t* pt_off; const GridMeta* meta;
    const float4 *sp4, *sn4, *slab4;          // slab4: never read (shot_neighbour<false>)
    const float *x, *y, *z;                   // original order: the tie's five points
    int n_obj;
    const int32_t* reg_obj; const float* reg_center; const float* reg_radius;
    uint32_t* n_sel; float* centroid; float* radius; float* lrf; float* desc; uint32_t* counts;
    int r_bins, e_bins, a_bins, log_radius;   // SHORT_SHOT_GLOBAL only
    double ln_rmin, min_radius;
};

template <bool SHOT>
struct GlobalSmem {
    double red_d[4];
    unsigned long long red_k[4];
    uint32_t red_u[4];
    float red_f[4];
    double axes[6];
    float lrf[9];
    int bad;
    shot_bin_t hist[SHOT ? 4 * 352 : 1];
    uint32_t cnt[SHOT ? 1 : 4 * ISMHIP_SHORT_SHOT_MAX_DIM];
};

// int(double) as the reference's x86-64 build takes it (cvttsd2si): NaN and values outside int give INT_MIN, which the clamps that
// follow turn into bin 0 (r) or drop (theta, phi: the bin index is checked against the row)
__device__ __forceinline__ int ref_int(double v) {
    return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (int)0x80000000;
}

template <bool SHOT>
__global__ __launch_bounds__(256) void k_global(GlobalArgs a) {
    __shared__ GlobalSmem<SHOT> sm;
    const int D = SHOT ? 352 : a.r_bins * a.e_bins * a.a_bins;
    const int tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const uint32_t reg = blockIdx.x;
    const float qnan = __builtin_nanf("");
    float* row = a.desc + (size_t)reg * D;
    uint32_t* crow = (!SHOT && a.counts) ? a.counts + (size_t)reg * D : nullptr;
    auto nan_row = [&](bool frame) {
        for (int i = tid; i < D; i += 256) { row[i] = qnan; if (crow) crow[i] = 0u; }
        if (frame && tid < 9) a.lrf[(size_t)reg * 9 + tid] = qnan;
    };

    // ---- the region -------------------------------------------------------------------------------------------------------------
    const int o = a.reg_obj[reg];
    const bool obj_ok = o >= 0 && o < a.n_obj;
    uint32_t base = 0, n = 0, npts = 0;
    GridMeta m{};
    if (obj_ok) {
        m = a.meta[o];
        base = a.pt_off[o]; npts = a.pt_off[o + 1] - base;
        n = m.n_finite < npts ? m.n_finite : npts;            // the sorted span holds the finite points first
    }
    const float qx = a.reg_center[reg * 3], qy = a.reg_center[reg * 3 + 1], qz = a.reg_center[reg * 3 + 2];
    const float rs = a.reg_radius[reg];
    const bool whole = rs < 0.f;
    const float r2s = (float)((double)rs * (double)rs);       // the ball sweeps' rule (shot_wave.h): d2 < (float)((double)r * r)
    const float4* sp = a.sp4 + base;
    auto selected = [&](const float4& p) { return whole || sqdist3(p.x, p.y, p.z, qx, qy, qz) < r2s; };

    // ---- 1. count and centroid ----------------------------------------------------------------------------------------------------
    uint32_t nsel; float cx, cy, cz;
    if (whole) {
        nsel = n; cx = m.centroid[0]; cy = m.centroid[1]; cz = m.centroid[2];
    } else {
        uint32_t c = 0; double sx = 0, sy = 0, sz = 0;
        for (uint32_t i = tid; i < n; i += 256) {
            const float4 p = sp[i];
            if (selected(p)) { sx += (double)p.x; sy += (double)p.y; sz += (double)p.z; c++; }
        }
        nsel = block_sum_i(c, sm.red_u);
        sx = block_sum_d_left(sx, sm.red_d); sy = block_sum_d_left(sy, sm.red_d); sz = block_sum_d_left(sz, sm.red_d);
        cx = (float)(sx / (double)nsel); cy = (float)(sy / (double)nsel); cz = (float)(sz / (double)nsel);   // pcl::compute3DCentroid
    }
    if (tid == 0) a.n_sel[reg] = nsel;
    if (nsel == 0) {                                          // workgroup-uniform
        if (tid < 3) a.centroid[reg * 3 + tid] = qnan;
        if (tid == 0) a.radius[reg] = 0.f;
        nan_row(true);
        return;
    }
    if (tid == 0) { a.centroid[reg * 3] = cx; a.centroid[reg * 3 + 1] = cy; a.centroid[reg * 3 + 2] = cz; }

    // ---- 2. radius: k_cloud_radii's arithmetic -----------------------------------------------------------------------------------------
    float R = 0.f;
    for (uint32_t i = tid; i < n; i += 256) {
        const float4 p = sp[i];
        if (!selected(p)) continue;
        const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        const float d = sqrtf(dx * dx + dy * dy + dz * dz);
        if (d > R) R = d;
    }
    R = block_max_f(R, sm.red_f);
    if (tid == 0) a.radius[reg] = R;
    const float r2 = (float)((double)R * (double)R);          // PCL: static_cast<float>(radius * radius) with a double radius
    // a descriptor neighbour: selected and inside the ball (centroid, R); a frame neighbour: also not the centroid itself (k_lrf_cov)
    auto neighbour = [&](const float4& p, float& d2) { d2 = sqdist3(p.x, p.y, p.z, cx, cy, cz); return d2 < r2 && selected(p); };
    auto frame_nb = [&](const float4& p) { return !(p.x == cx && p.y == cy && p.z == cz); };

    // ---- 3. covariance, eigenvectors ----------------------------------------------------------------------------------------------
    {
        double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0, sum = 0;
        uint32_t valid = 0;
        const double rd = (double)R;
        for (uint32_t i = tid; i < n; i += 256) {
            const float4 p = sp[i];
            float d2;
            if (!neighbour(p, d2) || !frame_nb(p)) continue;
            const double vx = (double)(p.x - cx), vy = (double)(p.y - cy), vz = (double)(p.z - cz);
            const double w = rd - sqrt_f32_as_f64(d2);
            const double wx = w * vx, wy = w * vy, wz = w * vz;
            c00 = fma(wx, vx, c00); c01 = fma(wx, vy, c01); c02 = fma(wx, vz, c02);
            c11 = fma(wy, vy, c11); c12 = fma(wy, vz, c12); c22 = fma(wz, vz, c22);
            sum += w; valid++;
        }
        c00 = block_sum_d_left(c00, sm.red_d); c01 = block_sum_d_left(c01, sm.red_d); c02 = block_sum_d_left(c02, sm.red_d);
        c11 = block_sum_d_left(c11, sm.red_d); c12 = block_sum_d_left(c12, sm.red_d); c22 = block_sum_d_left(c22, sm.red_d);
        sum = block_sum_d_left(sum, sm.red_d);
        const uint32_t nvalid = block_sum_i(valid, sm.red_u);
        if (tid == 0) {
            bool bad = nvalid < 5u;                                                // shot_na_lrf.hpp:80-86
            double w[3], V[3][3];
            if (!bad) {
                double A[3][3] = {{c00 / sum, c01 / sum, c02 / sum}, {c01 / sum, c11 / sum, c12 / sum}, {c02 / sum, c12 / sum, c22 / sum}};
                eigen_sym3(A, w, V);
                bad = !(isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]));
            }
            sm.bad = bad ? 1 : 0;
            if (!bad) {
                sm.axes[0] = V[0][2]; sm.axes[1] = V[1][2]; sm.axes[2] = V[2][2];     // x candidate: largest eigenvalue
                sm.axes[3] = V[0][0]; sm.axes[4] = V[1][0]; sm.axes[5] = V[2][0];     // z candidate: smallest
            }
        }
        __syncthreads();
        if (sm.bad) { nan_row(true); return; }

        // ---- 4. sign votes ------------------------------------------------------------------------------------------------------------
        double v1[3] = {sm.axes[0], sm.axes[1], sm.axes[2]}, v3[3] = {sm.axes[3], sm.axes[4], sm.axes[5]};
        uint32_t pt = 0, pn = 0;
        for (uint32_t i = tid; i < n; i += 256) {
            const float4 p = sp[i];
            float d2;
            if (!neighbour(p, d2) || !frame_nb(p)) continue;
            const double vx = (double)(p.x - cx), vy = (double)(p.y - cy), vz = (double)(p.z - cz);
            if (vx * v1[0] + vy * v1[1] + vz * v1[2] >= 0) pt++;
            if (vx * v3[0] + vy * v3[1] + vz * v3[2] >= 0) pn++;
        }
        const int plusT = 2 * (int)block_sum_i(pt, sm.red_u) - (int)nvalid;
        const int plusN = 2 * (int)block_sum_i(pn, sm.red_u) - (int)nvalid;
        if (plusT < 0) { v1[0] = -v1[0]; v1[1] = -v1[1]; v1[2] = -v1[2]; }
        if (plusN < 0) { v3[0] = -v3[0]; v3[1] = -v3[1]; v3[2] = -v3[2]; }
        if (plusT == 0 || plusN == 0) {                                            // workgroup-uniform
            // the five median neighbours by distance decide (shot_na_lrf.hpp:139-151): ranks n/2 - 2 .. n/2 + 2 of the keys
            // (bits of d^2, original index). The key of rank t is the largest v with #(key < v) <= t: one sweep per bit.
            auto key_of = [&](const float4& p, float d2) { return ((unsigned long long)__float_as_uint(d2) << 32) | __float_as_uint(p.w); };
            int idx_bits = 1; while (idx_bits < 32 && (1u << idx_bits) < npts) ++idx_bits;
            const uint32_t tsel = nvalid / 2 - 2;
            unsigned long long five[5], sel = 0ull;
            for (int bit = 62; bit >= 0; --bit) {
                if (bit < 32 && bit >= idx_bits) continue;
                const unsigned long long cand = sel | (1ull << bit);
                uint32_t c = 0;
                for (uint32_t i = tid; i < n; i += 256) {
                    const float4 p = sp[i];
                    float d2;
                    if (neighbour(p, d2) && frame_nb(p)) c += key_of(p, d2) < cand;
                }
                if (block_sum_i(c, sm.red_u) <= tsel) sel = cand;
            }
            five[0] = sel;
            for (int j = 1; j < 5; ++j) {
                unsigned long long mn = ~0ull;
                for (uint32_t i = tid; i < n; i += 256) {
                    const float4 p = sp[i];
                    float d2;
                    if (!neighbour(p, d2) || !frame_nb(p)) continue;
                    const unsigned long long kk = key_of(p, d2);
                    if (kk > five[j - 1] && kk < mn) mn = kk;
                }
                five[j] = block_min_u64(mn, sm.red_k);
            }
            int cntx = 0, cntz = 0;
            for (int j = 0; j < 5; ++j) {
                const uint32_t orig = (uint32_t)(five[j] & 0xffffffffull);
                if (orig >= npts) continue;                                        // cannot happen: every key is a neighbour's
                const double vx = (double)(a.x[base + orig] - cx), vy = (double)(a.y[base + orig] - cy), vz = (double)(a.z[base + orig] - cz);
                if (vx * v1[0] + vy * v1[1] + vz * v1[2] > 0) cntx++;
                if (vx * v3[0] + vy * v3[1] + vz * v3[2] > 0) cntz++;
            }
            if (plusT == 0 && cntx < 3) { v1[0] = -v1[0]; v1[1] = -v1[1]; v1[2] = -v1[2]; }
            if (plusN == 0 && cntz < 3) { v3[0] = -v3[0]; v3[1] = -v3[1]; v3[2] = -v3[2]; }
        }
        if (tid == 0) write_lrf(sm.lrf, v1, v3);
        __syncthreads();
        if (tid < 9) a.lrf[(size_t)reg * 9 + tid] = sm.lrf[tid];
    }
    const float fx[3] = {sm.lrf[0], sm.lrf[1], sm.lrf[2]}, fy[3] = {sm.lrf[3], sm.lrf[4], sm.lrf[5]}, fz[3] = {sm.lrf[6], sm.lrf[7], sm.lrf[8]};

    // ---- 5. the histogram and its norm ----------------------------------------------------------------------------------------------
    if constexpr (SHOT) {
        for (int i = tid; i < 4 * 352; i += 256) sm.hist[i] = 0ull;
        __syncthreads();
        shot_bin_t* hist = sm.hist + wv * 352;
        const float r12 = R * 0.5f, r14 = R * 0.25f, r34 = (R * 3.0f) * 0.25f, inv_r12 = 1.0f / r12;
        const float r12sq_f = shot_r12sq_f(R);
        uint32_t total = 0;
        for (uint32_t i = tid; i < n; i += 256) {
            const float4 p = sp[i];
            float d2;
            if (!neighbour(p, d2)) continue;
            total++;
            shot_neighbour<false>(a, hist, true, base + i, p.x - cx, p.y - cy, p.z - cz, d2, fx, fy, fz, r12, r14, r34, inv_r12, r12sq_f, 0.f, 0.f, 0.f);
        }
        total = block_sum_i(total, sm.red_u);                                      // its barriers also publish the deposits
        if (total < 5u) { nan_row(false); return; }                               // computePointSHOT: fewer than 5 neighbours
        // normalizeHistogram: double accumulate of float squares, divide by float(norm)
        float v[2] = {0.f, 0.f};
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + 256 * j;
            if (i < 352) {
                const shot_bin_t h = sm.hist[i] + sm.hist[352 + i] + sm.hist[704 + i] + sm.hist[1056 + i];
                v[j] = (float)((double)h * SHOT_FIX_INV);
                acc += (double)(v[j] * v[j]);
            }
        }
        const float fn = (float)sqrt(block_sum_d_left(acc, sm.red_d));
#pragma unroll
        for (int j = 0; j < 2; ++j) { const int i = tid + 256 * j; if (i < 352) row[i] = v[j] / fn; }
    } else {
        // A short histogram draws many lanes onto the same address, and same-address LDS atomics of a wave instruction serialise: the
        // 256 slots a wave owns hold 256 / D copies of the D bins, lane l counts in copy l % copies (integers: the merge is exact)
        const int copies = ISMHIP_SHORT_SHOT_MAX_DIM / D;
        for (int i = tid; i < 4 * ISMHIP_SHORT_SHOT_MAX_DIM; i += 256) sm.cnt[i] = 0u;
        __syncthreads();
        uint32_t* hist = sm.cnt + wv * ISMHIP_SHORT_SHOT_MAX_DIM + (lane % copies) * D;
        const int rb = a.r_bins, eb = a.e_bins, ab = a.a_bins;
        const double radius_d = (double)R;
        const double ln_rmax_rmin = a.log_radius ? log(radius_d / a.min_radius) : 1.0;
        for (uint32_t i = tid; i < n; i += 256) {
            const float4 p = sp[i];
            float d2;
            if (!neighbour(p, d2)) continue;
            if (!((double)d2 > 1e-15)) continue;                                   // distances[j] > 1E-15 on the SQUARED distance (:124)
            const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
            const double xl = (double)((dx * fx[0] + dy * fx[1]) + dz * fx[2]);    // float products, unfused, in short_shot.hip's order
            const double yl = (double)((dx * fy[0] + dy * fy[1]) + dz * fy[2]);
            const double zl = (double)((dx * fz[0] + dy * fz[1]) + dz * fz[2]);
            const double r = sqrt((xl * xl + yl * yl) + zl * zl);
            const double theta = acos(zl / r) * GLOBAL_SSHOT_RAD2DEG;
            const double phi = atan2(yl, xl) * GLOBAL_SSHOT_RAD2DEG;
            int bin_r = a.log_radius ? ref_int(((double)(rb - 1) * (log(r) - a.ln_rmin)) / ln_rmax_rmin + 1.0)
                                     : ref_int(((double)rb * r) / radius_d);
            int bin_theta = ref_int(((double)eb * theta) / 180.0);
            int bin_phi = ref_int(((double)ab * (phi + 180.0)) / 360.0);
            bin_r = bin_r >= 0 ? bin_r : 0;
            bin_r = bin_r < rb ? bin_r : rb - 1;
            bin_theta = bin_theta < eb ? bin_theta : eb - 1;
            bin_phi = bin_phi < ab ? bin_phi : ab - 1;
            if (bin_theta < 0 || bin_phi < 0) continue;                            // a NaN angle: outside the row in the reference (undefined there)
            atomicAdd(&hist[bin_r + bin_theta * rb + bin_phi * rb * eb], 1u);
        }
        __syncthreads();
        uint32_t c = 0;
        if (tid < D) for (int k = 0; k < 4; ++k) for (int j = 0; j < copies; ++j) c += sm.cnt[k * ISMHIP_SHORT_SHOT_MAX_DIM + j * D + tid];
        if (crow && tid < D) crow[tid] = c;
        // the L2 norm (:151-161): double sum of squares (integers below 2^53: exact in any order), sqrt, double division, cast to float;
        // no contributing point gives 0 / 0: a NaN row
        const double cd = (double)c;
        const double norm = sqrt(block_sum_d_left(cd * cd, sm.red_d));
        if (tid < D) row[tid] = (float)(cd / norm);
    }
}

// ---- VFH (features/features_vfh.cpp:27-70 -> pcl::VFHEstimation, PCL 1.10 vfh.hpp restated in include/ismhip.h) ----------------------
// The same region, count, centroid and radius as k_global (steps 1 and 2, the same arithmetic: bit-equal outputs), but NO frame: the
// pair (centroid, normal centroid) against every selected point with a finite normal, pair_features.h's exact evaluation, four 45-bin
// blocks and a 128-bin viewpoint block of INTEGER counts. Sweeps: count + centroid (skipped for a whole object), radius fused with the
// normal sums (32 B per point: position and normal), histogram (32 B per point). Byte model per whole-object region: 64 B x n.
// A 45-bin block -- and a viewpoint block that a planar patch drives into ONE bin -- is the same-address case of the short histogram
// above: each wave owns VFH_COPIES copies of the 308 bins, lane l counts in copy l % VFH_COPIES; integers, so the merge is exact.
struct VfhArgs {
    const uint32_t* pt_off; const GridMeta* meta;
    const float4 *sp4, *sn4;
    int n_obj;
    const int32_t* reg_obj; const float* reg_center; const float* reg_radius;
    float vpx, vpy, vpz; int fill_size;
    uint32_t* n_sel; float* centroid; float* radius; float* ncen; float* desc; uint32_t* counts;
};

struct VfhSmem {
    double red_d[4];
    uint32_t red_u[4];
    float red_f[4];
    uint32_t cnt[4 * VFH_COPIES * ISMHIP_VFH_DIM];
};

// vfh_bin, span_sweep and the per-point deposit vfh_deposit: vfh_deposit.h (shared with cvfh.hip)
__global__ __launch_bounds__(256) void k_vfh(VfhArgs a) {
    __shared__ VfhSmem sm;
    constexpr int D = ISMHIP_VFH_DIM;
    const int tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const uint32_t reg = blockIdx.x;
    const float qnan = __builtin_nanf("");
    float* row = a.desc + (size_t)reg * D;
    uint32_t* crow = a.counts ? a.counts + (size_t)reg * D : nullptr;
    auto nan_row = [&]() { for (int i = tid; i < D; i += 256) { row[i] = qnan; if (crow) crow[i] = 0u; } };

    // ---- the region: as k_global ---------------------------------------------------------------------------------------------------
    const int o = a.reg_obj[reg];
    const bool obj_ok = o >= 0 && o < a.n_obj;
    uint32_t base = 0, n = 0;
    GridMeta m{};
    if (obj_ok) {
        m = a.meta[o];
        base = a.pt_off[o];
        const uint32_t npts = a.pt_off[o + 1] - base;
        n = m.n_finite < npts ? m.n_finite : npts;            // the sorted span holds the finite points first
    }
    const float qx = a.reg_center[reg * 3], qy = a.reg_center[reg * 3 + 1], qz = a.reg_center[reg * 3 + 2];
    const float rs = a.reg_radius[reg];
    const bool whole = rs < 0.f;
    const float r2s = (float)((double)rs * (double)rs);
    const float4* sp = a.sp4 + base;
    const float4* sn = a.sn4 + base;
    auto selected = [&](const float4& p) { return whole || sqdist3(p.x, p.y, p.z, qx, qy, qz) < r2s; };

    // ---- 1. count and centroid: k_global's step 1 ---------------------------------------------------------------------------------
    uint32_t nsel; float cx, cy, cz;
    if (whole) {
        nsel = n; cx = m.centroid[0]; cy = m.centroid[1]; cz = m.centroid[2];
    } else {
        uint32_t c = 0; double sx = 0, sy = 0, sz = 0;
        for (uint32_t i = tid; i < n; i += 256) {
            const float4 p = sp[i];
            if (selected(p)) { sx += (double)p.x; sy += (double)p.y; sz += (double)p.z; c++; }
        }
        nsel = block_sum_i(c, sm.red_u);
        sx = block_sum_d_left(sx, sm.red_d); sy = block_sum_d_left(sy, sm.red_d); sz = block_sum_d_left(sz, sm.red_d);
        cx = (float)(sx / (double)nsel); cy = (float)(sy / (double)nsel); cz = (float)(sz / (double)nsel);
    }
    if (tid == 0) a.n_sel[reg] = nsel;
    if (nsel == 0) {                                          // workgroup-uniform
        if (tid < 3) { a.centroid[reg * 3 + tid] = qnan; a.ncen[reg * 3 + tid] = qnan; }
        if (tid == 0) a.radius[reg] = 0.f;
        nan_row();
        return;
    }
    if (tid == 0) { a.centroid[reg * 3] = cx; a.centroid[reg * 3 + 1] = cy; a.centroid[reg * 3 + 2] = cz; }

    // ---- 2. radius (k_global's step 2) and the normal centroid: double sums over the finite normals, fixed order ------------------------
    float R = 0.f;
    uint32_t mt = 0; double snx = 0, sny = 0, snz = 0;
    span_sweep<true>(sp, sn, n, tid, [&](const float4& p, const float4& nr) {
        if (!selected(p)) return;
        const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        const float d = sqrtf(dx * dx + dy * dy + dz * dz);
        if (d > R) R = d;
        if (isfinite(nr.x) && isfinite(nr.y) && isfinite(nr.z)) { snx += (double)nr.x; sny += (double)nr.y; snz += (double)nr.z; mt++; }
    });
    R = block_max_f(R, sm.red_f);
    const uint32_t mfin = block_sum_i(mt, sm.red_u);
    snx = block_sum_d_left(snx, sm.red_d); sny = block_sum_d_left(sny, sm.red_d); snz = block_sum_d_left(snz, sm.red_d);
    const float ncx = (float)(snx / (double)mfin), ncy = (float)(sny / (double)mfin), ncz = (float)(snz / (double)mfin);   // m = 0: NaN
    if (tid == 0) {
        a.radius[reg] = R;
        a.ncen[reg * 3] = ncx; a.ncen[reg * 3 + 1] = ncy; a.ncen[reg * 3 + 2] = ncz;
    }
    if (mfin < 2u) { nan_row(); return; }                     // workgroup-uniform

    // ---- the view direction: (viewpoint - centroid) / |.| in float; a zero norm leaves 0 ----------------------------------------------
    float vdx, vdy, vdz;
    vfh_view_direction(a.vpx, a.vpy, a.vpz, cx, cy, cz, vdx, vdy, vdz);

    // ---- 3. the histogram ----------------------------------------------------------------------------------------------------------------
    for (int i = tid; i < 4 * VFH_COPIES * D; i += 256) sm.cnt[i] = 0u;
    __syncthreads();
    uint32_t* hist = sm.cnt + (wv * VFH_COPIES + (lane % VFH_COPIES)) * D;
    span_sweep<true>(sp, sn, n, tid, [&](const float4& p, const float4& nr) {
        if (!selected(p)) return;
        // b4: hundredths of a unit, not normalised
        vfh_deposit(hist, cx, cy, cz, ncx, ncy, ncz, vdx, vdy, vdz, p, nr,
                    [](float f4) { return vfh_bin((double)(f4 * 100.0f) + 0.5, VFH_SHAPE_BINS - 1); });
    });
    __syncthreads();
    // counts -> row: one product per bin (order-free); the distance block stays zero unless the size component is asked for
    const float incr = 100.0f / (float)(mfin - 1u);
    const double incr_shape = (double)incr, incr_vp = (double)(float)(100.0 / (double)mfin);
    for (int b = tid; b < D; b += 256) {
        uint32_t c = 0;
        for (int k = 0; k < 4 * VFH_COPIES; ++k) c += sm.cnt[k * D + b];
        if (crow) crow[b] = c;
        const bool size_block = b >= 3 * VFH_SHAPE_BINS && b < 4 * VFH_SHAPE_BINS;
        row[b] = (size_block && !a.fill_size) ? 0.f : (float)((double)c * (b < 4 * VFH_SHAPE_BINS ? incr_shape : incr_vp));
    }
}

// ---- GASD (features/features_gasd.cpp:25-91 -> pcl::GASDColorEstimation, PCL 1.10 gasd.hpp restated in include/ismhip.h) -------------
// The same region, count, centroid and radius as k_global (steps 1 and 2, the same arithmetic: bit-equal outputs); the frame is the
// region's own covariance frame (eigen3.h on one thread), the histograms two regular grids in that frame: 6^3 cells of positions and
// 4^3 cells x 12 hue bins, INTEGER counts. Sweeps, 16 B per point each: count + centroid (skipped for a whole object), radius fused
// with the six covariance sums, max_coord fused with the sign counts of x, histogram (+ 4 B per point for its colour).
// Byte model per whole-object region: 48 B x n, 52 B x n with colour.
// A planar region drives every point into one z layer of cells, the same-address case of the short histogram above. Each wave owns
// GASD_COPIES copies of the 984 bins, lane l counts in copy l % GASD_COPIES; integers, so the merge is exact. ONE copy per wave is
// kept: measured against two on planes and on blobs, the times are equal within their spread, and one copy
// is half the LDS. Static LDS 15 848 bytes, below k_vfh's 39 488.
#ifndef GASD_COPIES
#define GASD_COPIES 1
#endif
#define GASD_SHAPE_BINS 216
#define GASD_HUE_BINS 12

struct GasdArgs {
    const uint32_t* pt_off; const GridMeta* meta;
    const float4* sp4; const uint32_t* rgba;  // rgba: the caller's colours in original order (with_color), read at the index sp4.w carries
    int n_obj;
    const int32_t* reg_obj; const float* reg_center; const float* reg_radius;
    float vdx, vdy, vdz; int with_color;
    uint32_t* n_sel; float* centroid; float* radius; float* frame; float* max_coord; float* desc; uint32_t* counts;
};

struct GasdSmem {
    double red_d[4];
    uint32_t red_u[4];
    float red_f[4];
    float frame[9];
    int bad;
    uint32_t cnt[4 * GASD_COPIES * ISMHIP_GASD_DIM];
};

// the hue bin of a packed colour by GASDColorEstimation::computeFeature's float arithmetic (include/ismhip.h); -1: no deposit
__device__ __forceinline__ int gasd_hue_bin(uint32_t c4) {
    const int r = (int)((c4 >> 16) & 0xffu), g = (int)((c4 >> 8) & 0xffu), b = (int)(c4 & 0xffu);
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    const float diff_inv = 1.f / (float)(mx - mn);
    float hue;
    if (!isfinite(diff_inv)) hue = 0.f;
    else if (mx == r) hue = 60.f * ((float)(g - b) * diff_inv);
    else if (mx == g) hue = 60.f * (2.f + (float)(b - r) * diff_inv);
    else hue = 60.f * (4.f + (float)(r - g) * diff_inv);
    if (hue < 0.f) hue += 360.f;
    const float hb = floorf((hue / 360.f) * (float)GASD_HUE_BINS);
    return (hb >= 0.f && hb < (float)GASD_HUE_BINS) ? (int)hb : -1;
}

// floor((q * half) + half) as a cell index; -1 outside 0 .. 2 * half - 1 and for a NaN (PCL's padding cell: no deposit)
__device__ __forceinline__ int gasd_cell(float q, float half) {
    const float coord = floorf(q * half + half);               // unfused (-ffp-contract=off)
    return (coord >= 0.f && coord < 2.f * half) ? (int)coord : -1;
}

__global__ __launch_bounds__(256) void k_gasd(GasdArgs a) {
    __shared__ GasdSmem sm;
    const int D = a.with_color ? ISMHIP_GASD_DIM : ISMHIP_GASD_SHAPE_DIM;
    const int tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const uint32_t reg = blockIdx.x;
    const float qnan = __builtin_nanf("");
    float* row = a.desc + (size_t)reg * D;
    uint32_t* crow = a.counts ? a.counts + (size_t)reg * D : nullptr;
    auto nan_row = [&](bool frame) {
        for (int i = tid; i < D; i += 256) { row[i] = qnan; if (crow) crow[i] = 0u; }
        if (frame && tid < 9) a.frame[(size_t)reg * 9 + tid] = qnan;
        if (frame && tid == 0) a.max_coord[reg] = qnan;
    };

    // ---- the region: as k_global ---------------------------------------------------------------------------------------------------
    const int o = a.reg_obj[reg];
    const bool obj_ok = o >= 0 && o < a.n_obj;
    uint32_t base = 0, n = 0;
    GridMeta m{};
    if (obj_ok) {
        m = a.meta[o];
        base = a.pt_off[o];
        const uint32_t npts = a.pt_off[o + 1] - base;
        n = m.n_finite < npts ? m.n_finite : npts;            // the sorted span holds the finite points first
    }
    const float qx = a.reg_center[reg * 3], qy = a.reg_center[reg * 3 + 1], qz = a.reg_center[reg * 3 + 2];
    const float rs = a.reg_radius[reg];
    const bool whole = rs < 0.f;
    const float r2s = (float)((double)rs * (double)rs);
    const float4* sp = a.sp4 + base;
    auto selected = [&](const float4& p) { return whole || sqdist3(p.x, p.y, p.z, qx, qy, qz) < r2s; };

    // ---- 1. count and centroid: k_global's step 1 ---------------------------------------------------------------------------------
    uint32_t nsel; float cx, cy, cz;
    if (whole) {
        nsel = n; cx = m.centroid[0]; cy = m.centroid[1]; cz = m.centroid[2];
    } else {
        uint32_t c = 0; double sx = 0, sy = 0, sz = 0;
        span_sweep<false>(sp, sp, n, tid, [&](const float4& p, const float4&) {
            if (selected(p)) { sx += (double)p.x; sy += (double)p.y; sz += (double)p.z; c++; }
        });
        nsel = block_sum_i(c, sm.red_u);
        sx = block_sum_d_left(sx, sm.red_d); sy = block_sum_d_left(sy, sm.red_d); sz = block_sum_d_left(sz, sm.red_d);
        cx = (float)(sx / (double)nsel); cy = (float)(sy / (double)nsel); cz = (float)(sz / (double)nsel);
    }
    if (tid == 0) a.n_sel[reg] = nsel;
    if (nsel == 0) {                                          // workgroup-uniform
        if (tid < 3) a.centroid[reg * 3 + tid] = qnan;
        if (tid == 0) a.radius[reg] = 0.f;
        nan_row(true);
        return;
    }
    if (tid == 0) { a.centroid[reg * 3] = cx; a.centroid[reg * 3 + 1] = cy; a.centroid[reg * 3 + 2] = cz; }

    // ---- 2. radius (k_global's step 2) and the covariance sums: products of the float differences in double (exact), fixed order ------
    float R = 0.f;
    double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
    span_sweep<false>(sp, sp, n, tid, [&](const float4& p, const float4&) {
        if (!selected(p)) return;
        const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        const float d = sqrtf(dx * dx + dy * dy + dz * dz);
        if (d > R) R = d;
        const double vx = (double)dx, vy = (double)dy, vz = (double)dz;
        c00 += vx * vx; c01 += vx * vy; c02 += vx * vz; c11 += vy * vy; c12 += vy * vz; c22 += vz * vz;
    });
    R = block_max_f(R, sm.red_f);
    if (tid == 0) a.radius[reg] = R;
    if (nsel < 2u) { nan_row(true); return; }                 // workgroup-uniform: PCL's increment 100 / (n - 1) is infinite
    c00 = block_sum_d_left(c00, sm.red_d); c01 = block_sum_d_left(c01, sm.red_d); c02 = block_sum_d_left(c02, sm.red_d);
    c11 = block_sum_d_left(c11, sm.red_d); c12 = block_sum_d_left(c12, sm.red_d); c22 = block_sum_d_left(c22, sm.red_d);

    // ---- 3. the frame, up to the sign of x: z the smallest eigenvalue's vector, turned away from the view direction; x the largest's -----
    if (tid == 0) {
        double A[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}}, w[3], V[3][3];
        eigen_sym3(A, w, V);
        double z[3] = {V[0][0], V[1][0], V[2][0]};
        const double x[3] = {V[0][2], V[1][2], V[2][2]};
        if ((z[0] * (double)a.vdx + z[1] * (double)a.vdy) + z[2] * (double)a.vdz > 0.0) { z[0] = -z[0]; z[1] = -z[1]; z[2] = -z[2]; }
        const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            sm.frame[k] = (float)x[k]; sm.frame[3 + k] = (float)y[k]; sm.frame[6 + k] = (float)z[k];
            ok = ok && isfinite(x[k]) && isfinite(y[k]) && isfinite(z[k]);
        }
        sm.bad = ok ? 0 : 1;
    }
    __syncthreads();
    if (sm.bad) { nan_row(true); return; }                    // a covariance that overflowed: no frame
    float fx[3] = {sm.frame[0], sm.frame[1], sm.frame[2]}, fy[3] = {sm.frame[3], sm.frame[4], sm.frame[5]};
    const float fz[3] = {sm.frame[6], sm.frame[7], sm.frame[8]};
    auto rotate = [&](const float4& p, float& tx, float& ty, float& tz) {       // float products, unfused, in this order
        const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        tx = (fx[0] * dx + fx[1] * dy) + fx[2] * dz;
        ty = (fy[0] * dx + fy[1] * dy) + fy[2] * dz;
        tz = (fz[0] * dx + fz[1] * dy) + fz[2] * dz;
    };

    // ---- 4. max_coord and the sign of x: neither |t| nor the two counts' roles depend on the sign the sweep runs with -------------------
    float mc = 0.f;
    uint32_t pos = 0, neg = 0;
    span_sweep<false>(sp, sp, n, tid, [&](const float4& p, const float4&) {
        if (!selected(p)) return;
        float tx, ty, tz;
        rotate(p, tx, ty, tz);
        mc = fmaxf(mc, fmaxf(fabsf(tx), fmaxf(fabsf(ty), fabsf(tz))));
        pos += tx > 0.f; neg += tx < 0.f;
    });
    mc = block_max_f(mc, sm.red_f);
    const uint32_t npos = block_sum_i(pos, sm.red_u), nneg = block_sum_i(neg, sm.red_u);
    bool flip = nneg > npos;
    if (nneg == npos) {                                       // a tie: the component of largest magnitude (lowest index) becomes positive
        int k = 0;
        if (fabsf(fx[1]) > fabsf(fx[k])) k = 1;
        if (fabsf(fx[2]) > fabsf(fx[k])) k = 2;
        flip = fx[k] < 0.f;
    }
    if (flip) for (int k = 0; k < 3; ++k) { fx[k] = -fx[k]; fy[k] = -fy[k]; }   // y = z cross x changes sign with x, exactly
    if (tid < 3) { a.frame[(size_t)reg * 9 + tid] = fx[tid]; a.frame[(size_t)reg * 9 + 3 + tid] = fy[tid]; a.frame[(size_t)reg * 9 + 6 + tid] = fz[tid]; }
    if (tid == 0) a.max_coord[reg] = mc;
    if (!(mc > 0.f && isfinite(mc))) { nan_row(false); return; }                // workgroup-uniform: coincident points, or an overflow

    // ---- 5. the histograms --------------------------------------------------------------------------------------------------------------
    for (int i = tid; i < 4 * GASD_COPIES * ISMHIP_GASD_DIM; i += 256) sm.cnt[i] = 0u;
    __syncthreads();
    uint32_t* hist = sm.cnt + (wv * GASD_COPIES + (lane % GASD_COPIES)) * ISMHIP_GASD_DIM;
    const uint32_t* rgba = a.with_color ? a.rgba + base : nullptr;
    span_sweep<false>(sp, sp, n, tid, [&](const float4& p, const float4&) {
        if (!selected(p)) return;
        float tx, ty, tz;
        rotate(p, tx, ty, tz);
        const float ux = tx / mc, uy = ty / mc, uz = tz / mc;
        const int bx = gasd_cell(ux, 3.0f), by = gasd_cell(uy, 3.0f), bz = gasd_cell(uz, 3.0f);
        if ((bx | by | bz) >= 0) atomicAdd(&hist[(bx * 6 + by) * 6 + bz], 1u);
        if (!rgba) return;
        const int gx = gasd_cell(ux, 2.0f), gy = gasd_cell(uy, 2.0f), gz = gasd_cell(uz, 2.0f);
        if ((gx | gy | gz) < 0) return;
        const int hb = gasd_hue_bin(rgba[__float_as_uint(p.w)]);
        if (hb >= 0) atomicAdd(&hist[GASD_SHAPE_BINS + ((gx * 4 + gy) * 4 + gz) * GASD_HUE_BINS + hb], 1u);
    });
    __syncthreads();
    // counts -> row: one product per bin (order-free); without colour the bins past the shape block are zeros
    const double incr = (double)(100.0f / (float)(nsel - 1u));
    const int live = a.with_color ? ISMHIP_GASD_DIM : GASD_SHAPE_BINS;
    for (int b = tid; b < D; b += 256) {
        uint32_t c = 0;
        if (b < live) for (int k = 0; k < 4 * GASD_COPIES; ++k) c += sm.cnt[k * ISMHIP_GASD_DIM + b];
        if (crow) crow[b] = c;
        row[b] = (float)((double)c * incr);
    }
}

__global__ __launch_bounds__(256) void k_gasd_hue_probe(int n, const uint32_t* __restrict__ rgba, uint8_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int hb = gasd_hue_bin(rgba[i]);
    out[i] = hb < 0 ? (uint8_t)255 : (uint8_t)hb;
}

int global_check(ismhip_ctx* ctx, const char* name, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                 const float* region_radius, const uint32_t* n_sel_out, const float* centroid_out, const float* radius_out, const float* lrf9_out,
                 const float* desc_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    const bool arrays = region_obj && region_center && region_radius && n_sel_out && centroid_out && radius_out && lrf9_out && desc_out;
    if (!cloud || n_regions < 0 || (n_regions > 0 && !arrays))                     // no region: nothing is read or written
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, std::string(name) + ": bad argument");
    return ISMHIP_OK;
}

GlobalArgs global_args(const ismhip_cloud* cloud, const int32_t* region_obj, const float* region_center, const float* region_radius,
                       uint32_t* n_sel_out, float* centroid_out, float* radius_out, float* lrf9_out, float* desc_out) {
    GlobalArgs a{};
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.sp4 = cloud->sp4; a.sn4 = cloud->sn4; a.slab4 = cloud->slab4;
    a.x = cloud->x; a.y = cloud->y; a.z = cloud->z; a.n_obj = cloud->n_obj;
    a.reg_obj = region_obj; a.reg_center = region_center; a.reg_radius = region_radius;
    a.n_sel = n_sel_out; a.centroid = centroid_out; a.radius = radius_out; a.lrf = lrf9_out; a.desc = desc_out;
    return a;
}

}  // namespace

extern "C" {

int ismhip_global_short_shot(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                             const float* region_radius, double min_radius, int log_radius, int r_bins, int e_bins, int a_bins,
                             uint32_t* n_sel_out, float* centroid_out, float* radius_out, float* lrf9_out, float* desc_out, uint32_t* count_out) {
    int rc = global_check(ctx, "global_short_shot", cloud, n_regions, region_obj, region_center, region_radius, n_sel_out, centroid_out, radius_out,
                          lrf9_out, desc_out);
    if (rc != ISMHIP_OK) return rc;
    if (r_bins < 1 || e_bins < 1 || a_bins < 1) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_short_shot: fewer than one bin on an axis");
    if ((long long)r_bins * e_bins * a_bins > ISMHIP_SHORT_SHOT_MAX_DIM)
        return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "global_short_shot: more than 256 bins");
    if (log_radius && !(min_radius > 0.0 && std::isfinite(min_radius)))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_short_shot: logarithmic radius needs min_radius > 0");
    if (n_regions == 0) return ISMHIP_OK;
    GlobalArgs a = global_args(cloud, region_obj, region_center, region_radius, n_sel_out, centroid_out, radius_out, lrf9_out, desc_out);
    a.counts = count_out;
    a.r_bins = r_bins; a.e_bins = e_bins; a.a_bins = a_bins; a.log_radius = log_radius ? 1 : 0;
    a.min_radius = min_radius; a.ln_rmin = log_radius ? log(min_radius) : 0.0;
    TimerScope ts(ctx, "global_short_shot");
    hipLaunchKernelGGL(k_global<false>, dim3((unsigned)n_regions), dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_global<short_shot>");
    return ISMHIP_OK;
}

int ismhip_global_shot352(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                          const float* region_radius, uint32_t* n_sel_out, float* centroid_out, float* radius_out, float* lrf9_out, float* desc_out) {
    int rc = global_check(ctx, "global_shot352", cloud, n_regions, region_obj, region_center, region_radius, n_sel_out, centroid_out, radius_out,
                          lrf9_out, desc_out);
    if (rc != ISMHIP_OK || n_regions == 0) return rc;
    GlobalArgs a = global_args(cloud, region_obj, region_center, region_radius, n_sel_out, centroid_out, radius_out, lrf9_out, desc_out);
    TimerScope ts(ctx, "global_shot352");
    hipLaunchKernelGGL(k_global<true>, dim3((unsigned)n_regions), dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_global<shot352>");
    return ISMHIP_OK;
}

int ismhip_global_vfh(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                      const float* region_radius, const float viewpoint[3], int fill_size_component, uint32_t* n_sel_out, float* centroid_out,
                      float* radius_out, float* normal_centroid_out, float* desc_out, uint32_t* count_out) {
    // global_check's rules; there is no frame: the normal centroid is the fourth per-region output it asks for
    int rc = global_check(ctx, "global_vfh", cloud, n_regions, region_obj, region_center, region_radius, n_sel_out, centroid_out, radius_out,
                          normal_centroid_out, desc_out);
    if (rc != ISMHIP_OK) return rc;
    if (!viewpoint || !(std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2])))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_vfh: the viewpoint is not finite");
    if (n_regions == 0) return ISMHIP_OK;
    VfhArgs a{};
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.sp4 = cloud->sp4; a.sn4 = cloud->sn4; a.n_obj = cloud->n_obj;
    a.reg_obj = region_obj; a.reg_center = region_center; a.reg_radius = region_radius;
    a.vpx = viewpoint[0]; a.vpy = viewpoint[1]; a.vpz = viewpoint[2]; a.fill_size = fill_size_component ? 1 : 0;
    a.n_sel = n_sel_out; a.centroid = centroid_out; a.radius = radius_out; a.ncen = normal_centroid_out; a.desc = desc_out; a.counts = count_out;
    TimerScope ts(ctx, "global_vfh");
    hipLaunchKernelGGL(k_vfh, dim3((unsigned)n_regions), dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_vfh");
    return ISMHIP_OK;
}

int ismhip_global_gasd(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                       const float* region_radius, const float view_direction[3], int with_color, uint32_t* n_sel_out, float* centroid_out,
                       float* radius_out, float* frame9_out, float* max_coord_out, float* desc_out, uint32_t* count_out) {
    int rc = global_check(ctx, "global_gasd", cloud, n_regions, region_obj, region_center, region_radius, n_sel_out, centroid_out, radius_out,
                          frame9_out, desc_out);
    if (rc != ISMHIP_OK) return rc;
    if (n_regions > 0 && !max_coord_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_gasd: bad argument");
    const float* v = view_direction;
    if (!v || !(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2])) || (v[0] == 0.f && v[1] == 0.f && v[2] == 0.f))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_gasd: the view direction is zero or not finite");
    if (with_color && !cloud->rgba) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_gasd: colour arrays missing");
    if (n_regions == 0) return ISMHIP_OK;
    GasdArgs a{};
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.sp4 = cloud->sp4; a.rgba = cloud->rgba; a.n_obj = cloud->n_obj;
    a.reg_obj = region_obj; a.reg_center = region_center; a.reg_radius = region_radius;
    a.vdx = v[0]; a.vdy = v[1]; a.vdz = v[2]; a.with_color = with_color ? 1 : 0;
    a.n_sel = n_sel_out; a.centroid = centroid_out; a.radius = radius_out; a.frame = frame9_out; a.max_coord = max_coord_out;
    a.desc = desc_out; a.counts = count_out;
    TimerScope ts(ctx, "global_gasd");
    hipLaunchKernelGGL(k_gasd, dim3((unsigned)n_regions), dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_gasd");
    return ISMHIP_OK;
}

int ismhip_gasd_hue_bins(ismhip_ctx* ctx, int n, const uint32_t* rgba, uint8_t* out) {
    if (!ctx || n < 0 || (n > 0 && (!rgba || !out))) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "gasd_hue_bins: bad argument");
    if (n == 0) return ISMHIP_OK;
    hipLaunchKernelGGL(k_gasd_hue_probe, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, ctx->stream, n, rgba, out);
    ISM_CHECK_LAUNCH(ctx, "k_gasd_hue_probe");
    return ISMHIP_OK;
}

}  // extern "C"

// culling.hip — VoxelGridCulling keypoints (Keypoints type "VoxelGridCulling") on the device: quality scores and culling.
// Reference seam: KeypointsVoxelGridCulling (keypoints/keypoints_voxel_grid_culling.cpp): voxel-grid keypoints, a geometry score and a
// colour score per keypoint over its LeafSize ball (getScoresForKeypoints :280-344, computeKPQ :441-471, computeColorScore :474-506),
// per-object thresholds (computeThresholds :346-432) and the acceptance rule (:204-272). Where PCL decides the arithmetic (the normal
// curvature of NormalEstimation, PrincipalCurvaturesEstimation) the definition is this library's own, restated from knowledge of PCL 1.10
// (tests/culling_ref.py); where the reference's own source decides it, the text is followed as written.
//
// Every ball has radius LeafSize and follows the rule of ismhip_filter_radius: unfused float d2, strictly below (float)((double)r * r),
// non-finite points are never neighbours.
//   k_cull_nmax / k_cull_kmax : per object the largest squared normal length / the largest finite |pc1 * pc2|: the scales of the grids below
//   k_cull_pc                 : dense, one thread per surface point in cell order (the sweep of k_iss_saliency): scatter of the normals
//                               projected into the point's tangent plane, eigen-solve, pc1 / pc2 in original point order
//   k_cull_scores             : one wave per keypoint (A/B below): one sweep fills the geometry score (curvature or kpq) and the colour score
//   k_cull_select             : one workgroup per object: min / max, combined scores, the three order statistics, acceptance -> keep mask
//   ism_compact_keypoints     : the mask -> ordered compaction of compact.hip (over a view of the keypoint arrays)
//
// Every sum that depends on the neighbours' order is ORDER FREE, as in iss3d.hip: a term is rounded to a multiple of q = 2^(e - bits), 2^e
// a power of two above the terms' bound, by adding 1.5 * 2^(e - bits + 52), and the integers are added. bits = 48 for an object of up to
// 2^14 - 1 finite points, one fewer per doubling beyond (bits + log2(points + 1) <= 62), so a ball that holds the whole object fits 64
// bits. The bounds: r^2 for the products and r for the components of p - keypoint (curvature); B (1 + B)^2 and its root for the projected
// normals, B the object's largest squared normal length (a per-object reduction: normals need not be unit); the object's largest finite
// |K| for kpq's sum of K = pc1 * pc2. Results are the same bits for any cell size, lane mapping and run, and an object's results do not
// depend on the other objects of the batch.
#include "common.h"
#include "eigen3.h"
#include "moments.h"
#include <cfloat>
#include <cmath>

namespace {

struct CullView {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4* sp4;
    int n_obj, nbx;
};

__device__ __forceinline__ bool fin3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// one workgroup per object: the largest squared length (double) over the finite normals of its finite points
__global__ __launch_bounds__(256) void k_cull_nmax(const uint32_t* __restrict__ pt_off, const GridMeta* __restrict__ meta, const float4* __restrict__ sn4,
                                                   double* __restrict__ nmax2) {
    const int o = blockIdx.x;
    const uint32_t base = pt_off[o], n = meta[o].n_finite;
    unsigned long long best = 0ull;                      // non-negative doubles order as their bits
    for (uint32_t t = threadIdx.x; t < n; t += 256) {
        const float4 v = sn4[base + t];
        if (!fin3(v.x, v.y, v.z)) continue;
        const double l2 = ((double)v.x * (double)v.x + (double)v.y * (double)v.y) + (double)v.z * (double)v.z;
        const unsigned long long b = (unsigned long long)__double_as_longlong(l2);
        best = b > best ? b : best;
    }
    __shared__ unsigned long long red[4];
    best = block_max_u64(best, red);
    if (threadIdx.x == 0) nmax2[o] = __longlong_as_double((long long)best);
}

// one workgroup per object: the largest finite |pc1 * pc2| (float product, as computeKPQ forms it)
__global__ __launch_bounds__(256) void k_cull_kmax(const uint32_t* __restrict__ pt_off, const float* __restrict__ pc1, const float* __restrict__ pc2,
                                                   float* __restrict__ kmax) {
    const int o = blockIdx.x;
    const uint32_t b = pt_off[o], e = pt_off[o + 1];
    uint32_t best = 0u;                                  // non-negative floats order as their bits
    for (uint32_t i = b + threadIdx.x; i < e; i += 256) {
        const float K = fabsf(pc1[i] * pc2[i]);
        if (isfinite(K)) best = max(best, __float_as_uint(K));
    }
    __shared__ uint32_t red[4];
    best = block_max_u32(best, red);
    if (threadIdx.x == 0) kmax[o] = __uint_as_float(best);
}

// one thread per (cell-sorted) surface point
__global__ __launch_bounds__(256) void k_cull_pc(CullView cv, const float4* __restrict__ sn4, const double* __restrict__ nmax2, float radius, float r2,
                                                 float* __restrict__ pc1, float* __restrict__ pc2, uint32_t* __restrict__ count) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const float4 q = cv.sp4[base + t];
    const float4 nq = sn4[base + t];
    const uint32_t orig = base + __float_as_uint(q.w);
    if (!fin3(nq.x, nq.y, nq.z)) return;                 // the outputs were filled with NaN / 0 before
    const double B = nmax2[o];
    const int e2 = exp_above(B * ((1.0 + B) * (1.0 + B)));
    const GridScale G = grid_scale(e2, half_exp_up(e2), grid_bits(m.n_finite));
    const double nx = (double)nq.x, ny = (double)nq.y, nz = (double)nq.z;
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    Moments s;
    int cnt = 0;
    ball_rows_for_each(m, cs, q.x, q.y, q.z, radius, [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = cv.sp4[base + i];
            if (!(sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < r2)) continue;
            const float4 nj = sn4[base + i];
            if (!fin3(nj.x, nj.y, nj.z)) continue;
            const double jx = (double)nj.x, jy = (double)nj.y, jz = (double)nj.z;
            const double dot = (nx * jx + ny * jy) + nz * jz;
            s.add(G, jx - nx * dot, jy - ny * dot, jz - nz * dot);
            cnt++;
        }
        return true;
    });
    double w[3], tr;
    s.centred_eigenvalues(G, cnt, w, tr);                // cnt >= 1: the point itself
    pc1[orig] = (float)(w[2] / (double)cnt);
    pc2[orig] = (float)(w[1] / (double)cnt);
    if (count) count[orig] = (uint32_t)cnt;
}

struct ScoreArgs {
    const uint32_t* kp_off; const float *kx, *ky, *kz; const uint32_t* krgba;
    const float4* slab4; const float *pc1, *pc2, *kmax; const float *lut_srgb, *lut_sxyz;
    float radius, r2, max_color_dist;
    int geometry, color;                                 // ISMHIP_CULLING_GEOMETRY_*, colour score on / off
    float *geo, *col; uint32_t* count;
};

// One WAVE per keypoint on the flattened sweep of k_pca_normals (ball_for_each): one sweep over the keypoint's ball fills both scores.
// Measured against one thread per keypoint on ball_rows_for_each (256 objects of 16384 points, leaf 0.1, 320 keypoints
// per object, 239 ball points per keypoint): curvature 0.33 against 0.99 ms, kpq 0.21 against 1.63 ms, colordistance 0.15 against 1.45 ms,
// kpq + colordistance 0.26 against 2.29 ms. Unlike the dense sweeps (every point a query, k_cull_pc, k_iss_saliency) the keypoints are a
// leaf apart, so the 64 keypoints of a wave share few cell rows and a thread per keypoint walks 240 records with its lanes on different
// rows; the thread mapping was dropped. The sums are order free, so the mapping does not show in the results.
__global__ __launch_bounds__(256) void k_cull_scores(CullView cv, ScoreArgs a) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const uint32_t k = a.kp_off[o] + (uint32_t)bx * 4 + (threadIdx.x >> 6);
    if (k >= a.kp_off[o + 1]) return;                        // wave-uniform
    const int lane = lane_id();
    const GridMeta m = cv.meta[o];
    const uint32_t base = cv.pt_off[o];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float qx = a.kx[k], qy = a.ky[k], qz = a.kz[k];
    const int bits = grid_bits(m.n_finite);
    GridScale G = {};
    if (a.geometry == ISMHIP_CULLING_GEOMETRY_CURVATURE) {
        G = ball_grid_scale(a.r2, bits);
    }
    double k_magic = 0.0, k_q = 0.0;
    if (a.geometry == ISMHIP_CULLING_GEOMETRY_KPQ) {
        const int e = exp_above((double)a.kmax[o]);
        k_magic = ldexp(1.5, e - bits + 52); k_q = ldexp(1.0, e - bits);
    }
    float LRef = 0.f, aRef = 0.f, bRef = 0.f;
    if (a.color) rgb2lab_norm(a.lut_srgb, a.lut_sxyz, a.krgba[k], LRef, aRef, bRef);
    Moments s;
    int cnt = 0, distant = 0, K_flags = 0;                   // K_flags: 1 a NaN K, 2 a +inf K, 4 a -inf K
    float max_k1 = FLT_MIN, min_k2 = FLT_MAX, max_K = FLT_MIN, min_K = FLT_MAX;
    long long sum_K = 0;
    CellRange cr;
    __shared__ WaveRows s_rows[4];
    if (fin3(qx, qy, qz) && m.n_finite > 0 && ball_cells(m, qx, qy, qz, a.radius, cr))
        ball_for_each(m, cs, cr, qx, qy, qz, a.radius, lane, s_rows[threadIdx.x >> 6],
                      [&](uint32_t t, bool) { return cv.sp4[base + t]; },
                      [&](const float4& p, uint32_t i, bool v) {
            if (!v || !(sqdist3(p.x, p.y, p.z, qx, qy, qz) < a.r2)) return;
            cnt++;
            if (a.geometry == ISMHIP_CULLING_GEOMETRY_CURVATURE)
                s.add(G, (double)p.x - (double)qx, (double)p.y - (double)qy, (double)p.z - (double)qz);
            if (a.geometry == ISMHIP_CULLING_GEOMETRY_KPQ) {
                const uint32_t orig = base + __float_as_uint(p.w);
                const float k_1 = a.pc1[orig], k_2 = a.pc2[orig];
                const float K = k_1 * k_2;
                if (k_1 > max_k1) max_k1 = k_1;
                if (k_2 < min_k2) min_k2 = k_2;
                if (K > max_K) max_K = K;
                if (K < min_K) min_K = K;
                if (isfinite(K)) sum_K += on_grid((double)K, k_magic);
                else K_flags |= isnan(K) ? 1 : (K > 0.f ? 2 : 4);
            }
            if (a.color) {
                const float4 lab = a.slab4[base + i];
                const float dL = LRef - lab.x, da = aRef - lab.y, db = bRef - lab.z;
                double cd = ((double)fabsf(dL) + ((double)fabsf(da) + (double)fabsf(db)) / 2.0) / 3.0;
                if (cd > 1.0) cd = 1.0;
                if (cd < 0.0) cd = 0.0;
                if ((float)cd > a.max_color_dist) distant++;
            }
        });
    // the lanes' parts: integer sums, and minima / maxima that never hold a NaN (a NaN never passes the comparisons above)
    cnt = wave_sum_i(cnt);
    float g = 0.f, c = 0.f;
    if (a.geometry == ISMHIP_CULLING_GEOMETRY_CURVATURE) {
        s.x = (long long)wave_sum_u64((unsigned long long)s.x); s.y = (long long)wave_sum_u64((unsigned long long)s.y);
        s.z = (long long)wave_sum_u64((unsigned long long)s.z); s.xx = (long long)wave_sum_u64((unsigned long long)s.xx);
        s.xy = (long long)wave_sum_u64((unsigned long long)s.xy); s.xz = (long long)wave_sum_u64((unsigned long long)s.xz);
        s.yy = (long long)wave_sum_u64((unsigned long long)s.yy); s.yz = (long long)wave_sum_u64((unsigned long long)s.yz);
        s.zz = (long long)wave_sum_u64((unsigned long long)s.zz);
        g = s.curvature(G, cnt);
    }
    if (a.geometry == ISMHIP_CULLING_GEOMETRY_KPQ) {
        sum_K = (long long)wave_sum_u64((unsigned long long)sum_K);
        max_k1 = wave_max_f(max_k1); max_K = wave_max_f(max_K); min_k2 = wave_min_f(min_k2); min_K = wave_min_f(min_K);
        const bool K_nan = __ballot(K_flags & 1) != 0ull, K_pinf = __ballot(K_flags & 2) != 0ull, K_ninf = __ballot(K_flags & 4) != 0ull;
        g = __builtin_nanf("");
        if (cnt > 0) {
            float sum = (float)((double)sum_K * k_q);
            if (K_nan || (K_pinf && K_ninf)) sum = __builtin_nanf("");
            else if (K_pinf) sum = __builtin_inff();
            else if (K_ninf) sum = -__builtin_inff();
            const float num = (float)cnt;
            g = (1000.0f / num * num) * sum + 100.0f * max_K + fabsf(100.0f * min_K) + 10.0f * max_k1 + fabsf(10.0f * min_k2);
        }
    }
    if (a.color) c = (float)wave_sum_i(distant) / (float)cnt;   // 0 / 0: NaN for an empty ball
    if (lane != 0) return;
    a.geo[k] = g; a.col[k] = c;
    if (a.count) a.count[k] = (uint32_t)cnt;
}

// ---- selection --------------------------------------------------------------------------------------------------------------------
// ascending order of std::sort's `<` on floats with NaN behind +inf: -0 and +0 share a key (ties go by index)
__device__ __forceinline__ uint32_t order_key(float v) {
    if (isnan(v)) return 0xffffffffu;
    if (v == 0.f) return 0x80000000u;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct SelectArgs {
    const uint32_t* kp_off; const float *geo, *col;
    int geo_on, col_on, geo_cutoff, col_cutoff, combine;
    float geo_threshold, col_threshold, ratio;
    float* combined; uint8_t* keep; float* thresholds;   // thresholds may be NULL
};

struct SelectShared {
    unsigned long long red64[4];
    uint32_t red32[4];
    BlockRank<256> rank;
    float picked;
};

// the element of v[0 .. n) at position `idx` of the ascending order (order_key, then index); every thread of the workgroup calls
__device__ float select_nth(const float* __restrict__ v, uint32_t n, uint32_t idx, SelectShared& sh) {
    uint32_t key = 0u;
    for (int bit = 31; bit >= 0; --bit) {                 // the largest key with at most idx elements below it
        const uint32_t trial = key | (1u << bit);
        uint32_t below = 0u;
        for (uint32_t i = threadIdx.x; i < n; i += 256) below += order_key(v[i]) < trial ? 1u : 0u;
        below = block_sum_i(below, sh.red32);
        if (below <= idx) key = trial;
    }
    uint32_t below = 0u;
    for (uint32_t i = threadIdx.x; i < n; i += 256) below += order_key(v[i]) < key ? 1u : 0u;
    below = block_sum_i(below, sh.red32);
    const uint32_t want = idx - below;                    // among the elements with that key, in index order
    uint32_t total = 0u;
    for (uint32_t c = 0; c < n; c += 256) {
        const uint32_t i = c + threadIdx.x;
        const bool hit = i < n && order_key(v[i]) == key;
        const uint32_t pos = sh.rank.step(hit, total);
        if (hit && pos == want) sh.picked = v[i];
    }
    __syncthreads();
    const float r = sh.picked;
    __syncthreads();
    return r;
}

// first smallest / first largest non-NaN element as std::min_element / std::max_element find them; none: +inf / -inf
__device__ void minmax_of(const float* __restrict__ v, uint32_t n, SelectShared& sh, float& mn, float& mx) {
    unsigned long long lo = ~0ull, hi = 0ull;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const float f = v[i];
        if (isnan(f)) continue;
        const unsigned long long key = (unsigned long long)order_key(f) << 32;
        const unsigned long long a = key | i, b = key | (0xffffffffu - i);
        lo = a < lo ? a : lo; hi = b > hi ? b : hi;
    }
    lo = block_min_u64(lo, sh.red64);
    hi = block_max_u64(hi, sh.red64);
    mn = lo == ~0ull ? __builtin_inff() : v[(uint32_t)(lo & 0xffffffffull)];
    mx = hi == 0ull ? -__builtin_inff() : v[0xffffffffu - (uint32_t)(hi & 0xffffffffull)];
}

__global__ __launch_bounds__(256) void k_cull_select(SelectArgs a) {
    const int o = blockIdx.x;
    const uint32_t b = a.kp_off[o], n = a.kp_off[o + 1] - b;
    const float* geo = a.geo + b; const float* col = a.col + b;
    float* comb = a.combined + b;
    __shared__ SelectShared sh;
    float thr_g = FLT_MIN, thr_c = FLT_MIN, thr_x = FLT_MIN;
    if (n > 0) {
        float gmin, gmax, cmin, cmax;
        minmax_of(geo, n, sh, gmin, gmax);
        minmax_of(col, n, sh, cmin, cmax);
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            const float geo_norm = (geo[i] - gmin) / gmax, color_norm = (col[i] - cmin) / cmax;
            comb[i] = geo_norm + color_norm;
        }
        __syncthreads();                                  // comb is read by other threads below
        uint32_t idx = (uint32_t)(a.ratio * (float)n);
        if (idx > n - 1) idx = n - 1;
        if (a.geo_on && a.geo_cutoff) thr_g = select_nth(geo, n, idx, sh);
        if (a.col_on && a.col_cutoff) thr_c = select_nth(col, n, idx, sh);
        if (a.geo_on && a.col_on && a.geo_cutoff && a.col_cutoff) thr_x = select_nth(comb, n, idx, sh);
    }
    if (a.geo_on && !a.geo_cutoff) thr_g = a.geo_threshold;
    if (a.col_on && !a.col_cutoff) thr_c = a.col_threshold;
    if (a.thresholds && threadIdx.x == 0) { a.thresholds[o * 3] = thr_g; a.thresholds[o * 3 + 1] = thr_c; a.thresholds[o * 3 + 2] = thr_x; }
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const bool geo_passed = !(a.geo_on && geo[i] < thr_g), color_passed = !(a.col_on && col[i] < thr_c);
        bool accept = geo_passed && color_passed;
        if (a.geo_on && a.col_on) {
            const bool combined_passed = !(comb[i] < thr_x);
            accept = a.combine == ISMHIP_CULLING_REQUIRE_ONE ? (geo_passed || color_passed)
                   : a.combine == ISMHIP_CULLING_REQUIRE_BOTH ? (geo_passed && color_passed) : combined_passed;
        }
        a.keep[b + i] = accept ? 1 : 0;
    }
}

CullView view_of(const ismhip_cloud* c, uint32_t longest_run) {
    CullView v;
    v.pt_off = c->pt_off; v.meta = c->meta; v.cell_start = c->cell_start; v.sp4 = c->sp4;
    v.n_obj = c->n_obj; v.nbx = (int)((longest_run + 255) / 256);
    if (v.nbx < 1) v.nbx = 1;
    return v;
}

bool positive(float v) { return v > 0.f && std::isfinite(v); }

}  // namespace

extern "C" {

int ismhip_principal_curvatures(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, float* pc1_out, float* pc2_out, uint32_t* count_out) {
    if (!ctx || !cloud || !positive(radius)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "principal_curvatures: bad argument");
    const size_t n = cloud->n_pts;
    if (n == 0) return ISMHIP_OK;
    if (!pc1_out || !pc2_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "principal_curvatures: pc1_out / pc2_out is NULL");
    const float r2 = (float)((double)radius * (double)radius);
    if (!(r2 > 0.f) || !std::isfinite(r2)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "principal_curvatures: radius out of range");
    double* nmax2 = (double*)ism_scratch(ctx, SCR_CULL_SCALE, (size_t)cloud->n_obj * 8);
    if (!nmax2) return ISMHIP_ERR_NOMEM;
    TimerScope ts(ctx, "culling_pc");
    // points whose position or own normal is not finite: NaN, count 0
    ISM_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)pc1_out, 0x7fc00000, n, ctx->stream));
    ISM_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)pc2_out, 0x7fc00000, n, ctx->stream));
    if (count_out) ISM_HIP(ctx, hipMemsetAsync(count_out, 0, n * 4, ctx->stream));
    hipLaunchKernelGGL(k_cull_nmax, dim3(cloud->n_obj), dim3(256), 0, ctx->stream, cloud->pt_off, cloud->meta, cloud->sn4, nmax2);
    ISM_CHECK_LAUNCH(ctx, "k_cull_nmax");
    const CullView cv = view_of(cloud, cloud->max_pts);
    hipLaunchKernelGGL(k_cull_pc, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(256), 0, ctx->stream, cv, cloud->sn4, nmax2, radius, r2,
                       pc1_out, pc2_out, count_out);
    ISM_CHECK_LAUNCH(ctx, "k_cull_pc");
    return ISMHIP_OK;
}

int ismhip_culling_scores(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h, const float* kx, const float* ky, const float* kz,
                          const uint32_t* krgba, float leaf, int geometry_method, int color_method, float max_similar_color_distance,
                          const float* pc1, const float* pc2, float* geo_out, float* color_out, uint32_t* count_out) {
    if (!ctx || !cloud || !kp_offsets_h || !positive(leaf) || geometry_method < ISMHIP_CULLING_GEOMETRY_NONE || geometry_method > ISMHIP_CULLING_GEOMETRY_KPQ ||
        color_method < ISMHIP_CULLING_COLOR_NONE || color_method > ISMHIP_CULLING_COLOR_DISTANCE || std::isnan(max_similar_color_distance))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "culling_scores: bad argument");
    const float r2 = (float)((double)leaf * (double)leaf);
    if (!(r2 > 0.f) || !std::isfinite(r2)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "culling_scores: leaf out of range");
    RaggedOffsets kp;
    int rc = ism_ragged_offsets(ctx, "culling_scores", kp_offsets_h, cloud->n_obj, SCR_KP_OFF, RAGGED_START0, &kp);
    if (rc != ISMHIP_OK) return rc;
    if (kp.total == 0) return ISMHIP_OK;
    if (!kx || !ky || !kz || !geo_out || !color_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "culling_scores: keypoint or output array is NULL");
    if (geometry_method == ISMHIP_CULLING_GEOMETRY_KPQ && (!pc1 || !pc2))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "culling_scores: kpq needs pc1 and pc2 (ismhip_principal_curvatures)");
    // a recycled cloud keeps its slab4 allocation: rgba says whether THIS cloud has colours
    if (color_method == ISMHIP_CULLING_COLOR_DISTANCE && (!krgba || !cloud->rgba || !cloud->slab4))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "culling_scores: colordistance needs a cloud with colours and the keypoints' colours");
    if (!kp.dev) return ISMHIP_ERR_NOMEM;
    float* kmax = (float*)ism_scratch(ctx, SCR_CULL_SCALE, (size_t)cloud->n_obj * 8);
    if (!kmax) return ISMHIP_ERR_NOMEM;
    TimerScope ts(ctx, "culling_scores");
    if (geometry_method == ISMHIP_CULLING_GEOMETRY_KPQ) {
        hipLaunchKernelGGL(k_cull_kmax, dim3(cloud->n_obj), dim3(256), 0, ctx->stream, cloud->pt_off, pc1, pc2, kmax);
        ISM_CHECK_LAUNCH(ctx, "k_cull_kmax");
    }
    ScoreArgs a;
    a.kp_off = kp.dev; a.kx = kx; a.ky = ky; a.kz = kz; a.krgba = krgba;
    a.slab4 = cloud->slab4; a.pc1 = pc1; a.pc2 = pc2; a.kmax = kmax; a.lut_srgb = ctx->lut_srgb; a.lut_sxyz = ctx->lut_sxyz;
    a.radius = leaf; a.r2 = r2; a.max_color_dist = max_similar_color_distance;
    a.geometry = geometry_method; a.color = color_method == ISMHIP_CULLING_COLOR_DISTANCE;
    a.geo = geo_out; a.col = color_out; a.count = count_out;
    const CullView cv = view_of(cloud, kp.max_run * 64);   // four keypoints, one per wave, to a workgroup
    hipLaunchKernelGGL(k_cull_scores, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(256), 0, ctx->stream, cv, a);
    ISM_CHECK_LAUNCH(ctx, "k_cull_scores");
    return ISMHIP_OK;
}

int ismhip_culling_select(ismhip_ctx* ctx, int n_obj, const uint32_t* kp_offsets_h, const float* geo, const float* color, int geometry_on, int color_on,
                          int geometry_type, int color_type, float geometry_threshold, float color_threshold, float cutoff_ratio, int combine,
                          const float* kx, const float* ky, const float* kz, const uint32_t* krgba, uint32_t capacity, float* kx_out, float* ky_out,
                          float* kz_out, uint32_t* krgba_out, uint8_t* keep_mask_out, float* combined_out, float* thresholds_out,
                          uint32_t* kp_offsets_h_out) {
    if (!ctx || n_obj <= 0 || !kp_offsets_h || !kp_offsets_h_out || geometry_type < ISMHIP_CULLING_TYPE_CUTOFF || geometry_type > ISMHIP_CULLING_TYPE_THRESHOLD ||
        color_type < ISMHIP_CULLING_TYPE_CUTOFF || color_type > ISMHIP_CULLING_TYPE_THRESHOLD || combine < ISMHIP_CULLING_REQUIRE_ONE ||
        combine > ISMHIP_CULLING_REQUIRE_COMBINED_LIST || !(cutoff_ratio >= 0.f && cutoff_ratio < 1.f))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "culling_select: bad argument");
    for (int o = 0; o <= n_obj; ++o) kp_offsets_h_out[o] = 0;
    RaggedOffsets kp;
    int rc = ism_ragged_offsets(ctx, "culling_select", kp_offsets_h, n_obj, SCR_KP_OFF, RAGGED_START0 | RAGGED_EMPTY, &kp);
    if (rc != ISMHIP_OK) return rc;
    const size_t n = kp.total;
    if (n > 0 && (!geo || !color || !kx || !ky || !kz || !kx_out || !ky_out || !kz_out || (krgba && !krgba_out)))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "culling_select: score, keypoint or output array is NULL");
    if (n > 0 && (kx == kx_out || ky == ky_out || kz == kz_out || (krgba && krgba == krgba_out)))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "culling_select: the output arrays must not alias the inputs");
    if (!kp.dev) return ISMHIP_ERR_NOMEM;
    // scratch: [combined scores] [keep mask], whichever the caller does not take
    char* scr = (char*)ism_scratch(ctx, SCR_CULL_SELECT, n * 5 + 16);
    if (!scr) return ISMHIP_ERR_NOMEM;
    SelectArgs a;
    a.kp_off = kp.dev; a.geo = geo; a.col = color;
    a.geo_on = geometry_on != 0; a.col_on = color_on != 0;
    a.geo_cutoff = geometry_type == ISMHIP_CULLING_TYPE_CUTOFF; a.col_cutoff = color_type == ISMHIP_CULLING_TYPE_CUTOFF; a.combine = combine;
    a.geo_threshold = geometry_threshold; a.col_threshold = color_threshold; a.ratio = cutoff_ratio;
    a.combined = combined_out ? combined_out : (float*)scr;
    a.keep = keep_mask_out ? keep_mask_out : (uint8_t*)(scr + n * 4);
    a.thresholds = thresholds_out;
    {
        TimerScope ts(ctx, "culling_select");
        hipLaunchKernelGGL(k_cull_select, dim3(n_obj), dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_cull_select");
        if (n == 0) { ISM_HIP(ctx, hipStreamSynchronize(ctx->stream)); return ISMHIP_OK; }
        // the keypoint arrays seen as the points of a cloud: ism_compact_keypoints reads these fields only
        ismhip_cloud view;
        view.n_obj = n_obj; view.pt_off_h.assign(kp_offsets_h, kp_offsets_h + n_obj + 1);
        view.x = kx; view.y = ky; view.z = kz; view.rgba = krgba;
        return ism_compact_keypoints(ctx, "culling_select", &view, a.keep, capacity, kx_out, ky_out, kz_out, krgba_out, nullptr, kp_offsets_h_out);
    }
}

}  // extern "C"

// sift3d.hip — SIFT3D keypoints (Keypoints type "SIFT3D") on the device: the one detector that looks at more than one scale.
// Reference seam: KeypointsSIFT3D::iComputeKeypoints (keypoints/keypoints_sift3d.cpp:24-86) -> pcl::SIFTKeypoint on an XYZI cloud whose
// intensity is the normal's curvature, setScales(Radius, 4, 3), setMinimumContrast(0.0). PCL is external: the arithmetic is this
// library's definition (restated from PCL 1.10 sift_keypoint.hpp in tests/sift3d_ref.py).
//
// Per object, on finite points only, every squared distance the unfused float of sqdist3:
//   k_sift_curvature      : dense, one thread per surface point in cell order (the sweep of k_iss_saliency): the CURVATURE geometry score
//                           of k_cull_scores with the point itself as the keypoint -- the same Moments of moments.h, the same bits
//   (voxel.hip)           : one octave's downsampling, ismhip_voxel_downsample_xyzi
//   k_sift_gather / _imax : the intensities in cell order; per object the largest finite |I|, the scale of the numerator's grid
//   k_sift_scale_space    : dense, one thread per point in cell order on ball_rows_for_each: ONE sweep of the 3 * (largest scale) ball
//                           feeds the Gaussian sums of every scale whose own bound d2 <= 9 s2 the neighbour meets
//   k_sift_extrema        : one thread per point: its k nearest by (d2, index) with the growing box of k_sor_meandist (prefilter.hip),
//                           the list kept as 64-bit keys so that the order is total, then the strict comparisons against the
//                           neighbours' rows
//   k_sift_count / _emit  : the driver's bookkeeping: flags per object, ordered compaction into the caller's arrays
//
// The Gaussian sums are ORDER FREE, as the moments of iss3d.hip, culling.hip and rift.hip: a term (double) is rounded to a multiple of
// q = 2^(e - bits) by adding 1.5 * 2^(e - bits + 52), and the integers are added. w <= 1 < 2^1 for the denominator, |w I| < 2^ei, the
// power of two above the object's largest finite |I|, for the numerator; bits = 48 for an object of up to 2^14 - 2 points, one fewer
// per doubling beyond (grid_bits), so a ball that holds the whole object fits 64 bits. The columns are therefore the same bits for any
// cell size, lane mapping and run; the neighbour lists are exact whatever cells the box search read.
#include "common.h"
#include "eigen3.h"
#include "knn_box.h"
#include "moments.h"
#include <cfloat>
#include <cmath>

namespace {

#define SIFT_MAX_SCALES 16
#define SIFT_KNN_STEPS 64      // more box growth steps than any grid needs (knn_box.h: eight reach every cell): the search always completes
#define SIFT_KNN_BLOCK 64      // threads (queries) per block of k_sift_extrema; the key lists take k * 64 * 8 bytes of LDS

struct SiftView {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4* sp4;
    int n_obj, nbx;
};

SiftView view_of(const ismhip_cloud* c, unsigned per_block) {
    SiftView v;
    v.pt_off = c->pt_off; v.meta = c->meta; v.cell_start = c->cell_start; v.sp4 = c->sp4;
    v.n_obj = c->n_obj; v.nbx = (int)((c->max_pts + per_block - 1) / per_block);
    if (v.nbx < 1) v.nbx = 1;
    return v;
}

bool positive(float v) { return v > 0.f && std::isfinite(v); }

// ---- normal curvature ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sift_curvature(SiftView cv, float radius, float r2, float* __restrict__ curv, uint32_t* __restrict__ count) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q = cv.sp4[base + t];
    const GridScale G = ball_grid_scale(r2, grid_bits(m.n_finite));
    Moments s;
    int cnt = 0;
    ball_rows_for_each(m, cs, q.x, q.y, q.z, radius, [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = cv.sp4[base + i];
            if (!(sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < r2)) continue;
            s.add(G, (double)p.x - (double)q.x, (double)p.y - (double)q.y, (double)p.z - (double)q.z);
            cnt++;
        }
        return true;
    });
    const uint32_t orig = base + __float_as_uint(q.w);
    curv[orig] = s.curvature(G, cnt);
    if (count) count[orig] = (uint32_t)cnt;
}

// ---- scale space --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sift_gather(SiftView cv, const float* __restrict__ inten, float* __restrict__ si) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= cv.meta[o].n_finite) return;
    const uint32_t base = cv.pt_off[o];
    si[base + t] = inten[base + __float_as_uint(cv.sp4[base + t].w)];
}

// one workgroup per object: the largest finite |I| of its finite points (non-negative floats order as their bits)
__global__ __launch_bounds__(256) void k_sift_imax(const uint32_t* __restrict__ pt_off, const GridMeta* __restrict__ meta, const float* __restrict__ si,
                                                   float* __restrict__ imax) {
    const int o = blockIdx.x;
    const uint32_t base = pt_off[o], n = meta[o].n_finite;
    uint32_t best = 0u;
    for (uint32_t t = threadIdx.x; t < n; t += 256) {
        const float a = fabsf(si[base + t]);
        if (isfinite(a)) best = max(best, __float_as_uint(a));
    }
    __shared__ uint32_t red[4];
    best = block_max_u32(best, red);
    if (threadIdx.x == 0) imax[o] = __uint_as_float(best);
}

struct ScaleArgs {
    float s2[SIFT_MAX_SCALES], lim[SIFT_MAX_SCALES];      // scales[i]^2 and 9 * that, in float
    float radius, lim_max;                                // of the largest scale: the ball that is swept, the bound that counts
    int n;
};

// NS: the unrolled length of the per-scale loops (n <= NS); the sums stay in registers
template <int NS>
__global__ __launch_bounds__(256) void k_sift_scale_space(SiftView cv, const float* __restrict__ si, const float* __restrict__ imax, ScaleArgs A,
                                                          float* __restrict__ dog, uint32_t* __restrict__ count) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    if (!isfinite(si[base + t])) return;                  // the outputs were filled with NaN / 0 before
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q = cv.sp4[base + t];
    const int bits = grid_bits(m.n_finite);
    int ei = 0; (void)frexpf(imax[o], &ei);               // every finite |I| of the object < 2^ei
    const double magic_n = ldexp(1.5, ei - bits + 52), q_n = ldexp(1.0, ei - bits);
    const double magic_d = ldexp(1.5, 1 - bits + 52), q_d = ldexp(1.0, 1 - bits);
    long long num[NS], den[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) { num[s] = 0; den[s] = 0; }
    int cnt = 0;
    ball_rows_for_each(m, cs, q.x, q.y, q.z, A.radius, [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = cv.sp4[base + i];
            const float d2 = sqdist3(p.x, p.y, p.z, q.x, q.y, q.z);
            if (!(d2 <= A.lim_max)) continue;
            const float I = si[base + i];
            if (!isfinite(I)) continue;
            cnt++;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (s >= A.n || !(d2 <= A.lim[s])) continue;
                const float w = expf((-0.5f * d2) / A.s2[s]);
                num[s] += on_grid((double)(w * I), magic_n);
                den[s] += on_grid((double)w, magic_d);
            }
        }
        return true;
    });
    const uint32_t orig = base + __float_as_uint(q.w);
    if (count) count[orig] = (uint32_t)cnt;
    float* row = dog + (size_t)orig * (A.n - 1);
    float prev = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s >= A.n) continue;
        const float resp = (float)(((double)num[s] * q_n) / ((double)den[s] * q_d));   // den >= 1: the point itself
        if (s > 0) row[s - 1] = resp - prev;
        prev = resp;
    }
}

// ---- extrema ------------------------------------------------------------------------------------------------------------------
// The k nearest of every finite point (itself included) by (d2, index inside the object), exactly: the growing box of cells of
// knn_box.h, as in k_sor_meandist (prefilter.hip), on keys (bits of d2) << 32 | index, whose order is total (non-negative floats order
// as their bits). The search ends with the k-th squared distance strictly inside the nearest unread box face, so no tie waits outside.
// There is no step limit and no scan kernel behind it. Then the comparisons.
__global__ __launch_bounds__(SIFT_KNN_BLOCK) void k_sift_extrema(SiftView cv, int k, const float* __restrict__ dog, int n_cols, float min_contrast,
                                                                 uint8_t* __restrict__ flags, int32_t* __restrict__ nn) {
    extern __shared__ unsigned long long s_keys[];        // [k][SIFT_KNN_BLOCK]: slot j of thread t at j * SIFT_KNN_BLOCK + t
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * SIFT_KNN_BLOCK + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q4 = cv.sp4[base + t];
    const float q[3] = {q4.x, q4.y, q4.z};
    const unsigned long long NONE = ~0ull;
    unsigned long long* L = s_keys + threadIdx.x;
    for (int j = 0; j < k; ++j) L[j * SIFT_KNN_BLOCK] = NONE;
    // unsorted while it is filled, as in k_sor_meandist: a key below the largest one overwrites it, the new largest is found by a read of the k slots
    unsigned long long kth = NONE;
    float kth_d2 = INFINITY;                              // the largest squared distance of the full list; +inf while it is being filled
    int cnt = 0, kpos = 0;
    auto consider = [&](float d2, uint32_t idx) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | idx;
        if (!(key < kth)) return;
        if (cnt < k) { L[cnt * SIFT_KNN_BLOCK] = key; if (++cnt < k) return; }
        else L[kpos * SIFT_KNN_BLOCK] = key;
        unsigned long long mx = 0ull;
        for (int j = 0; j < k; ++j) { const unsigned long long v = L[j * SIFT_KNN_BLOCK]; if (v >= mx) { mx = v; kpos = j; } }
        kth = mx; kth_d2 = __uint_as_float((uint32_t)(mx >> 32));
    };
    auto span = [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = cv.sp4[base + i];
            consider(sqdist3(p.x, p.y, p.z, q[0], q[1], q[2]), __float_as_uint(p.w));
        }
    };
    (void)knn_box_search(m, cs, q, SIFT_KNN_STEPS, kth_d2, span);
    for (int i = 1; i < k; ++i) {                          // insertion sort, ascending; the empty slots stay behind
        const unsigned long long v = L[i * SIFT_KNN_BLOCK];
        int j = i;
        while (j > 0 && L[(j - 1) * SIFT_KNN_BLOCK] > v) { L[j * SIFT_KNN_BLOCK] = L[(j - 1) * SIFT_KNN_BLOCK]; --j; }
        L[j * SIFT_KNN_BLOCK] = v;
    }
    const uint32_t me = __float_as_uint(q4.w);
    const size_t self = (size_t)base + me;
    if (nn)
        for (int j = 0; j < k; ++j) {
            const unsigned long long v = L[j * SIFT_KNN_BLOCK];
            nn[self * k + j] = v == NONE ? -1 : (int32_t)(uint32_t)(v & 0xffffffffull);
        }
    // candidates by the point's own row, then every neighbour's three columns; strict throughout, so a NaN fails every test
    constexpr int MC = SIFT_MAX_SCALES - 1;
    float own[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) own[c] = c < n_cols ? dog[self * n_cols + c] : 0.f;
    uint32_t is_max = 0u, is_min = 0u;
#pragma unroll
    for (int c = 1; c < MC - 1; ++c) {
        if (c >= n_cols - 1 || !(fabsf(own[c]) >= min_contrast)) continue;
        if (own[c] > own[c - 1] && own[c] > own[c + 1]) is_max |= 1u << c;
        if (own[c] < own[c - 1] && own[c] < own[c + 1]) is_min |= 1u << c;
    }
    for (int j = 0; j < k && (is_max | is_min); ++j) {
        const unsigned long long v = L[j * SIFT_KNN_BLOCK];
        if (v == NONE) break;
        const uint32_t idx = (uint32_t)(v & 0xffffffffull);
        if (idx == me) continue;
        const float* dq = dog + ((size_t)base + idx) * n_cols;
        float d[MC];
#pragma unroll
        for (int c = 0; c < MC; ++c) d[c] = c < n_cols ? dq[c] : 0.f;
#pragma unroll
        for (int c = 1; c < MC - 1; ++c) {
            if (c >= n_cols - 1) continue;
            if (!(own[c] > d[c - 1] && own[c] > d[c] && own[c] > d[c + 1])) is_max &= ~(1u << c);
            if (!(own[c] < d[c - 1] && own[c] < d[c] && own[c] < d[c + 1])) is_min &= ~(1u << c);
        }
    }
    for (int c = 1; c < n_cols - 1; ++c) flags[self * n_cols + c] = ((is_max >> c) & 1u) ? 2 : (((is_min >> c) & 1u) ? 1 : 0);
}

// ---- the driver's bookkeeping -------------------------------------------------------------------------------------------------
// one workgroup per object: the set flags of its rows
__global__ __launch_bounds__(256) void k_sift_count(const uint32_t* __restrict__ pt_off, const uint8_t* __restrict__ flags, int n_cols,
                                                    uint32_t* __restrict__ obj_count) {
    const int o = blockIdx.x;
    const size_t b = (size_t)pt_off[o] * n_cols, e = (size_t)pt_off[o + 1] * n_cols;
    uint32_t c = 0;
    for (size_t i = b + threadIdx.x; i < e; i += 256) c += flags[i] ? 1u : 0u;
    __shared__ uint32_t red[4];
    c = block_sum_i(c, red);
    if (threadIdx.x == 0) obj_count[o] = c;
}

struct ScaleRow { float s[SIFT_MAX_SCALES]; };

// one workgroup per object: its set flags in (point, column) order -> keypoints from dest[o] on; dest[o] = ~0: nothing to write
__global__ __launch_bounds__(256) void k_sift_emit(const uint32_t* __restrict__ pt_off, const uint8_t* __restrict__ flags, int n_cols, ScaleRow scales,
                                                   const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                   const uint32_t* __restrict__ dest, float* __restrict__ kx, float* __restrict__ ky,
                                                   float* __restrict__ kz, float* __restrict__ kscale) {
    const int o = blockIdx.x;
    const uint32_t d0 = dest[o];
    if (d0 == 0xffffffffu) return;                        // uniform over the workgroup
    const uint32_t p0 = pt_off[o];
    const size_t n = (size_t)(pt_off[o + 1] - p0) * n_cols;
    __shared__ BlockScan<256> scan;
    scan.init();
    for (size_t c0 = 0; c0 < n; c0 += 256) {
        const size_t i = c0 + threadIdx.x;
        const bool hit = i < n && flags[(size_t)p0 * n_cols + i] != 0;
        const uint32_t before = scan.step(hit ? 1u : 0u);
        if (hit) {
            const uint32_t p = p0 + (uint32_t)(i / n_cols), c = (uint32_t)(i % n_cols), d = d0 + before;
            kx[d] = x[p]; ky[d] = y[p]; kz[d] = z[p];
            if (kscale) kscale[d] = scales.s[c];
        }
    }
}

int normal_curvature(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, float r2, float* curv_out, uint32_t* count_out) {
    const size_t n = cloud->n_pts;
    TimerScope ts(ctx, "normal_curvature");
    ISM_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)curv_out, 0x7fc00000, n, ctx->stream));
    if (count_out) ISM_HIP(ctx, hipMemsetAsync(count_out, 0, n * 4, ctx->stream));
    const SiftView cv = view_of(cloud, 256);
    hipLaunchKernelGGL(k_sift_curvature, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(256), 0, ctx->stream, cv, radius, r2, curv_out, count_out);
    ISM_CHECK_LAUNCH(ctx, "k_sift_curvature");
    return ISMHIP_OK;
}

// false: a scale is not positive and finite, or its ball's radius or bound is not finite
bool scale_args(const float* scales_h, int n_scales, ScaleArgs& A) {
    A.n = n_scales; A.radius = 0.f; A.lim_max = 0.f;
    for (int i = 0; i < SIFT_MAX_SCALES; ++i) { A.s2[i] = 1.f; A.lim[i] = 0.f; }
    for (int i = 0; i < n_scales; ++i) {
        const float s = scales_h[i];
        if (!positive(s)) return false;
        A.s2[i] = s * s; A.lim[i] = 9.0f * A.s2[i];
        if (!positive(A.s2[i]) || !positive(A.lim[i]) || !positive(3.0f * s)) return false;
        A.radius = std::max(A.radius, 3.0f * s); A.lim_max = std::max(A.lim_max, A.lim[i]);
    }
    return true;
}

int scale_space(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* intensity, const ScaleArgs& A, float* dog_out, uint32_t* count_out) {
    const size_t n = cloud->n_pts;
    float* si = (float*)ism_scratch(ctx, SCR_SIFT3D, n * sizeof(float));
    float* imax = (float*)ism_scratch(ctx, SCR_SIFT3D_SCALE, (size_t)cloud->n_obj * sizeof(float));
    if (!si || !imax) return ISMHIP_ERR_NOMEM;
    TimerScope ts(ctx, "sift3d_scale_space");
    // points that are not finite, or whose intensity is not: NaN rows, count 0
    ISM_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)dog_out, 0x7fc00000, n * (size_t)(A.n - 1), ctx->stream));
    if (count_out) ISM_HIP(ctx, hipMemsetAsync(count_out, 0, n * 4, ctx->stream));
    const SiftView cv = view_of(cloud, 256);
    const dim3 grid(xcd_object_grid((unsigned)cv.nbx, cv.n_obj));
    hipLaunchKernelGGL(k_sift_gather, grid, dim3(256), 0, ctx->stream, cv, intensity, si);
    ISM_CHECK_LAUNCH(ctx, "k_sift_gather");
    hipLaunchKernelGGL(k_sift_imax, dim3(cloud->n_obj), dim3(256), 0, ctx->stream, cloud->pt_off, cloud->meta, si, imax);
    ISM_CHECK_LAUNCH(ctx, "k_sift_imax");
    if (A.n <= 6) hipLaunchKernelGGL(k_sift_scale_space<6>, grid, dim3(256), 0, ctx->stream, cv, si, imax, A, dog_out, count_out);
    else hipLaunchKernelGGL(k_sift_scale_space<SIFT_MAX_SCALES>, grid, dim3(256), 0, ctx->stream, cv, si, imax, A, dog_out, count_out);
    ISM_CHECK_LAUNCH(ctx, "k_sift_scale_space");
    return ISMHIP_OK;
}

int extrema(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* dog, int n_cols, int k, float min_contrast, uint8_t* flags_out, int32_t* nn_idx_out) {
    const size_t n = cloud->n_pts;
    TimerScope ts(ctx, "sift3d_extrema");
    ISM_HIP(ctx, hipMemsetAsync(flags_out, 0, n * (size_t)n_cols, ctx->stream));
    if (nn_idx_out) ISM_HIP(ctx, hipMemsetAsync(nn_idx_out, 0xff, n * (size_t)k * 4, ctx->stream));
    const SiftView cv = view_of(cloud, SIFT_KNN_BLOCK);
    hipLaunchKernelGGL(k_sift_extrema, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(SIFT_KNN_BLOCK), (size_t)k * SIFT_KNN_BLOCK * 8, ctx->stream,
                       cv, k, dog, n_cols, min_contrast, flags_out, nn_idx_out);
    ISM_CHECK_LAUNCH(ctx, "k_sift_extrema");
    return ISMHIP_OK;
}

}  // namespace

extern "C" {

int ismhip_normal_curvature(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, float* curv_out, uint32_t* count_out) {
    if (!ctx || !cloud || !positive(radius)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "normal_curvature: bad argument");
    if (cloud->n_pts == 0) return ISMHIP_OK;
    if (!curv_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "normal_curvature: curv_out is NULL");
    const float r2 = (float)((double)radius * (double)radius);
    if (!positive(r2)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "normal_curvature: radius out of range");
    return normal_curvature(ctx, cloud, radius, r2, curv_out, count_out);
}

int ismhip_sift3d_scale_space(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* intensity, const float* scales_h, int n_scales, float* dog_out,
                              uint32_t* count_out) {
    ScaleArgs A;
    if (!ctx || !cloud || !scales_h || n_scales < 3 || n_scales > SIFT_MAX_SCALES || !scale_args(scales_h, n_scales, A))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_scale_space: bad argument (3 to 16 positive scales)");
    if (cloud->n_pts == 0) return ISMHIP_OK;
    if (!intensity || !dog_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_scale_space: intensity or dog_out is NULL");
    return scale_space(ctx, cloud, intensity, A, dog_out, count_out);
}

int ismhip_sift3d_extrema(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* dog, int n_cols, int k, float min_contrast, uint8_t* flags_out,
                          int32_t* nn_idx_out) {
    if (!ctx || !cloud || n_cols < 3 || n_cols > SIFT_MAX_SCALES - 1 || k < 1 || std::isnan(min_contrast))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_extrema: bad argument");
    if (k > ISMHIP_SOR_MAX_MEAN_K) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "sift3d_extrema: k above ISMHIP_SOR_MAX_MEAN_K (64) is not built");
    if (cloud->n_pts == 0) return ISMHIP_OK;
    if (!dog || !flags_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_extrema: dog or flags_out is NULL");
    return extrema(ctx, cloud, dog, n_cols, k, min_contrast, flags_out, nn_idx_out);
}

int ismhip_sift3d_keypoints(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* intensity, float min_scale, int nr_octaves, int nr_scales,
                            float min_contrast, uint32_t capacity, float* kx, float* ky, float* kz, float* kscale_out, uint32_t* kp_offsets_h_out,
                            uint32_t* octave_sizes_h_out) {
    if (!ctx || !cloud || !kp_offsets_h_out || !positive(min_scale) || nr_octaves < 1 || nr_octaves > ISMHIP_SIFT3D_MAX_OCTAVES || nr_scales < 1 ||
        nr_scales + 3 > SIFT_MAX_SCALES || !(min_contrast >= 0.f))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_keypoints: bad argument");
    const int n_obj = cloud->n_obj, n_sc = nr_scales + 3, n_cols = n_sc - 1;
    for (int o = 0; o <= n_obj; ++o) kp_offsets_h_out[o] = 0;
    if (octave_sizes_h_out) for (int i = 0; i < n_obj * nr_octaves; ++i) octave_sizes_h_out[i] = 0;
    if (cloud->n_pts == 0) return ISMHIP_OK;
    if (!intensity) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_keypoints: intensity is NULL");

    struct Octave {
        float *x, *y, *z, *i; uint8_t* flags;
        std::vector<uint32_t> off, dest;                  // the octave's cloud; per object the first keypoint inside the object's range (~0: none)
        ScaleRow scales;
    };
    std::vector<Octave> octs;
    octs.reserve(nr_octaves);                             // the offsets below are uploaded asynchronously: no element may move
    // the driver's block: [flag counts per object] [per octave: its offsets | destinations]
    uint32_t* drv = (uint32_t*)ism_scratch(ctx, SCR_SIFT3D_DRIVER, ((size_t)n_obj + (size_t)nr_octaves * (2 * n_obj + 1)) * 4);
    if (!drv) return ISMHIP_ERR_NOMEM;
    std::vector<char> alive(n_obj, 1);
    std::vector<uint32_t> total(n_obj, 0), cnt_h(n_obj);
    const float *cx = cloud->x, *cy = cloud->y, *cz = cloud->z, *ci = intensity;
    std::vector<uint32_t> cur_off = cloud->pt_off_h;
    float scale = min_scale;
    for (int oc = 0; oc < nr_octaves; ++oc, scale *= 2.0f) {
        const uint32_t cur_n = cur_off[n_obj];
        if (cur_n == 0 || !positive(scale)) break;
        // this octave's block: [x | y | z | i] [dog] [flags]
        const size_t n4 = ((size_t)cur_n + 3) & ~(size_t)3;
        char* blk = (char*)ism_scratch(ctx, SCR_SIFT3D_OCTAVE + oc, n4 * 16 + n4 * (size_t)n_cols * 5);
        if (!blk) return ISMHIP_ERR_NOMEM;
        octs.emplace_back();
        Octave& O = octs.back();
        O.x = (float*)blk; O.y = O.x + n4; O.z = O.y + n4; O.i = O.z + n4;
        float* dog = O.i + n4;
        O.flags = (uint8_t*)(dog + n4 * (size_t)n_cols);
        O.off.assign(n_obj + 1, 0); O.dest.assign(n_obj, 0xffffffffu);
        int rc = ismhip_voxel_downsample_xyzi(ctx, n_obj, cur_off.data(), cx, cy, cz, ci, scale, cur_n, O.x, O.y, O.z, O.i, O.off.data());
        if (rc != ISMHIP_OK) return rc;
        bool any = false;
        for (int o = 0; o < n_obj; ++o) {
            if (!alive[o]) continue;
            const uint32_t sz = O.off[o + 1] - O.off[o];
            if (octave_sizes_h_out) octave_sizes_h_out[(size_t)o * nr_octaves + oc] = sz;
            if (sz < ISMHIP_SIFT3D_MIN_POINTS) alive[o] = 0;
            else any = true;
        }
        if (!any) break;
        float scales[SIFT_MAX_SCALES];
        for (int i = 0; i < n_sc; ++i) scales[i] = scale * powf(2.0f, ((float)i - 1.0f) / (float)nr_scales);
        for (int i = 0; i < SIFT_MAX_SCALES; ++i) O.scales.s[i] = i < n_sc ? scales[i] : 0.f;
        ScaleArgs A;
        if (!scale_args(scales, n_sc, A)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_keypoints: scale out of range");
        // the octave's search grid; the stages never read the normals, the positions stand in for them
        ismhip_cloud* oc_cloud = nullptr;
        rc = ismhip_cloud_create(ctx, n_obj, O.off.data(), O.x, O.y, O.z, O.x, O.y, O.z, nullptr, 0.4f * (3.0f * scales[n_sc - 1]), &oc_cloud);
        if (rc != ISMHIP_OK) return rc;
        rc = scale_space(ctx, oc_cloud, O.i, A, dog, nullptr);
        if (rc == ISMHIP_OK) rc = extrema(ctx, oc_cloud, dog, n_cols, ISMHIP_SIFT3D_MIN_POINTS, min_contrast, O.flags, nullptr);
        if (rc == ISMHIP_OK) {
            hipLaunchKernelGGL(k_sift_count, dim3(n_obj), dim3(256), 0, ctx->stream, oc_cloud->pt_off, O.flags, n_cols, drv);
            if (hipGetLastError() != hipSuccess) rc = ism_set_err(ctx, ISMHIP_ERR_HIP, "launch k_sift_count");
        }
        if (rc == ISMHIP_OK && (hipMemcpyAsync(cnt_h.data(), drv, (size_t)n_obj * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                                hipStreamSynchronize(ctx->stream) != hipSuccess))
            rc = ism_set_err(ctx, ISMHIP_ERR_HIP, "sift3d_keypoints: reading the octave's counts");
        ismhip_cloud_destroy(ctx, oc_cloud);
        if (rc != ISMHIP_OK) return rc;
        for (int o = 0; o < n_obj; ++o) {
            if (!alive[o] || cnt_h[o] == 0) continue;
            O.dest[o] = total[o];
            total[o] += cnt_h[o];
        }
        cx = O.x; cy = O.y; cz = O.z; ci = O.i; cur_off = O.off;
    }
    unsigned long long sum = 0;
    for (int o = 0; o < n_obj; ++o) sum += total[o];
    if (sum > capacity) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_keypoints: output capacity too small");
    for (int o = 0; o < n_obj; ++o) kp_offsets_h_out[o + 1] = kp_offsets_h_out[o] + total[o];
    if (sum == 0) return ISMHIP_OK;
    if (!kx || !ky || !kz) {
        for (int o = 0; o <= n_obj; ++o) kp_offsets_h_out[o] = 0;
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "sift3d_keypoints: output array is NULL");
    }
    {
        TimerScope ts(ctx, "sift3d_emit");
        for (size_t oc = 0; oc < octs.size(); ++oc) {
            Octave& O = octs[oc];
            bool any = false;
            for (int o = 0; o < n_obj; ++o)
                if (O.dest[o] != 0xffffffffu) { O.dest[o] += kp_offsets_h_out[o]; any = true; }
            if (!any) continue;
            // [the octave's offsets | destinations]: the octave's slice of the driver block
            O.off.insert(O.off.end(), O.dest.begin(), O.dest.end());
            uint32_t* both = drv + n_obj + oc * (size_t)(2 * n_obj + 1);
            const uint32_t *off_d = both, *dest_d = both + n_obj + 1;
            ISM_HIP(ctx, hipMemcpyAsync(both, O.off.data(), (size_t)(2 * n_obj + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_sift_emit, dim3(n_obj), dim3(256), 0, ctx->stream, off_d, O.flags, n_cols, O.scales, O.x, O.y, O.z, dest_d, kx, ky, kz,
                               kscale_out);
            ISM_CHECK_LAUNCH(ctx, "k_sift_emit");
        }
    }
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));       // the uploads above were pageable host memory
    return ISMHIP_OK;
}

}  // extern "C"

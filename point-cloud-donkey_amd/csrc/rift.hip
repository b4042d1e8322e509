// rift.hip — the RIFT descriptor (Features type "RIFT"), n_distance_bins x n_gradient_bins floats, 128 at the reference's 8 x 16: the
// intensity gradient of a coloured cloud, histogrammed per keypoint over (distance from the keypoint, angle between the gradient and the
// direction away from the keypoint). Reference seam: FeaturesRIFT::iComputeDescriptors (features/features_rift.cpp:29-96) -> PCL 1.10
// PointCloudXYZRGBtoXYZI, IntensityGradientEstimation and RIFTEstimation::computeRIFT. PCL is external: the arithmetic is this
// library's definition with the named deviations D1-D5 (restated in tests/rift_ref.py).
//
// Two entries, every ball by the rule of ismhip_filter_radius (unfused float d2, strictly below (float)((double)r * r), finite points):
//   ismhip_intensity_gradients (timer "intensity_gradients")
//     k_rift_intensity : per cell-sorted point I = (0.299f R + 0.587f G) + 0.114f B, once per call
//     k_rift_gradient  : dense, one thread per point in cell order on ball_rows_for_each (the sweep of k_iss_saliency): the moments of
//                        the ball about the query, the centred 3 x 3 system A x = b, its pseudo-inverse over eigen_sym3, the projection
//                        into the point's tangent plane -> three floats in original point order
//   ismhip_rift (timer "rift")
//     k_rift_gmax      : per object the largest finite gradient magnitude: the scale of the histogram's fixed point
//     k_rift           : one wave per keypoint on ball_for_each (as k_pca_normals): bilinear deposits into a 64-bit fixed-point LDS
//                        histogram, L2 normalisation
//
// The moments are ORDER FREE, as in iss3d.hip and culling.hip: a term (double) is rounded to a multiple of q = 2^(e - bits), 2^e a power
// of two above the term's bound, by adding 1.5 * 2^(e - bits + 52), and the integers are added. bits = 48 for an object of up to 2^14 - 2
// finite points, one fewer per doubling beyond. Bounds, with d = p_j - q and dI = I_j - I_q (intensities are taken about the query's like
// the positions: a uniform colour then gives b = 0 and a zero gradient exactly): |d_a d_b| < 2^e2 (the power of two above r^2), |d_a| <
// 2^e1 (e1 = ceil(e2 / 2)), |dI| < 2^8, |d_a dI| < 2^(e1 + 8). The histogram is order free the same way: a deposit v = w * |g| (float,
// w <= 1) enters as round(v * 2^(hb - eg)), 2^eg the power of two above the object's largest |g|, hb = 40 bits for an object of up to
// 2^22 - 2 points; a ball point puts at most one deposit into a bin. Gradients and rows are the same bits for any cell size, lane
// mapping and run.
#include "shot_wave.h"
#include "eigen3.h"
#include <cfloat>
#include <cmath>

namespace {

#define RIFT_MAX_BINS 256                                // n_distance_bins * n_gradient_bins of one row: the LDS histogram of a wave

struct RiftView {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4 *sp4, *sn4;
    int n_obj, nbx;
};

__host__ __device__ inline int rift_bits(uint32_t n_points, int most) {
    int bits = most;
    while (bits > 24 && ((unsigned long long)n_points + 1ull) >= (1ull << (62 - bits))) --bits;
    return bits;
}
__device__ __forceinline__ long long on_grid(double v, double magic) { return __double_as_longlong(v + magic) - __double_as_longlong(magic); }
__device__ __forceinline__ bool fin3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }
// |g| as both kernels of ismhip_rift take it
__device__ __forceinline__ float grad_mag(float gx, float gy, float gz) { return sqrtf((gx * gx + gy * gy) + gz * gz); }

// ---- the gradient pass --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rift_intensity(RiftView cv, const uint32_t* __restrict__ rgba, float* __restrict__ si) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= cv.meta[o].n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const uint32_t c4 = rgba[base + __float_as_uint(cv.sp4[base + t].w)];
    const float R = (float)((c4 >> 16) & 0xff), G = (float)((c4 >> 8) & 0xff), B = (float)(c4 & 0xff);
    si[base + t] = (0.299f * R + 0.587f * G) + 0.114f * B;
}

// the four grids of the moments (head of the file)
struct RiftGrids { double m2, q2, m1, q1, mi, qi, mdi, qdi; };

__global__ __launch_bounds__(256) void k_rift_gradient(RiftView cv, const float* __restrict__ si, float radius, float r2, int e2,
                                                       float* __restrict__ grad, uint32_t* __restrict__ count) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q = cv.sp4[base + t];
    const double iq = (double)si[base + t];
    const int bits = rift_bits(m.n_finite, 48), e1 = e2 >= 0 ? (e2 + 1) / 2 : -((-e2) / 2);
    RiftGrids G;
    G.m2 = ldexp(1.5, e2 - bits + 52); G.q2 = ldexp(1.0, e2 - bits);
    G.m1 = ldexp(1.5, e1 - bits + 52); G.q1 = ldexp(1.0, e1 - bits);
    G.mi = ldexp(1.5, 8 - bits + 52); G.qi = ldexp(1.0, 8 - bits);
    G.mdi = ldexp(1.5, e1 + 8 - bits + 52); G.qdi = ldexp(1.0, e1 + 8 - bits);
    long long sx = 0, sy = 0, sz = 0, xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0, s_i = 0, xi = 0, yi = 0, zi = 0;
    int cnt = 0;
    ball_rows_for_each(m, cs, q.x, q.y, q.z, radius, [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = cv.sp4[base + i];
            if (!(sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < r2)) continue;
            const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
            const double di = (double)si[base + i] - iq;
            sx += on_grid(dx, G.m1); sy += on_grid(dy, G.m1); sz += on_grid(dz, G.m1);
            xx += on_grid(dx * dx, G.m2); xy += on_grid(dx * dy, G.m2); xz += on_grid(dx * dz, G.m2);
            yy += on_grid(dy * dy, G.m2); yz += on_grid(dy * dz, G.m2); zz += on_grid(dz * dz, G.m2);
            s_i += on_grid(di, G.mi);
            xi += on_grid(dx * di, G.mdi); yi += on_grid(dy * di, G.mdi); zi += on_grid(dz * di, G.mdi);
            cnt++;
        }
        return true;
    });
    const uint32_t orig = base + __float_as_uint(q.w);
    if (count) count[orig] = (uint32_t)cnt;
    const float4 nq = cv.sn4[base + t];
    if (cnt < 3 || !fin3(nq.x, nq.y, nq.z)) return;      // the output was filled with NaN before
    // A = sum (d - mean d)(d - mean d)^T, b = sum (d - mean d)(dI - mean dI)
    const double inv = 1.0 / (double)cnt;
    const double mx = (double)sx * G.q1, my = (double)sy * G.q1, mz = (double)sz * G.q1, mi = (double)s_i * G.qi;
    double A[3][3], w[3], V[3][3];
    A[0][0] = (double)xx * G.q2 - mx * mx * inv; A[0][1] = A[1][0] = (double)xy * G.q2 - mx * my * inv;
    A[0][2] = A[2][0] = (double)xz * G.q2 - mx * mz * inv; A[1][1] = (double)yy * G.q2 - my * my * inv;
    A[1][2] = A[2][1] = (double)yz * G.q2 - my * mz * inv; A[2][2] = (double)zz * G.q2 - mz * mz * inv;
    const double b[3] = {(double)xi * G.qdi - mx * mi * inv, (double)yi * G.qdi - my * mi * inv, (double)zi * G.qdi - mz * mi * inv};
    eigen_sym3(A, w, V);
    // D2: the pseudo-inverse over the eigenvalues above 1e-12 of the largest; none when the largest is not positive
    double x[3] = {0.0, 0.0, 0.0};
    if (w[2] > 0.0) {
        const double cut = 1e-12 * w[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!(w[k] > cut)) continue;
            const double c = ((V[0][k] * b[0] + V[1][k] * b[1]) + V[2][k] * b[2]) / w[k];
            x[0] += V[0][k] * c; x[1] += V[1][k] * c; x[2] += V[2][k] * c;
        }
    }
    const double nx = (double)nq.x, ny = (double)nq.y, nz = (double)nq.z;
    const double along = (nx * x[0] + ny * x[1]) + nz * x[2];
    grad[(size_t)orig * 3] = (float)(x[0] - nx * along);
    grad[(size_t)orig * 3 + 1] = (float)(x[1] - ny * along);
    grad[(size_t)orig * 3 + 2] = (float)(x[2] - nz * along);
}

// ---- the descriptor -----------------------------------------------------------------------------------------------------------
// one workgroup per object: the largest finite |g| (non-negative floats order as their bits)
__global__ __launch_bounds__(256) void k_rift_gmax(const uint32_t* __restrict__ pt_off, const float* __restrict__ grad, float* __restrict__ gmax) {
    const int o = blockIdx.x;
    const uint32_t b = pt_off[o], e = pt_off[o + 1];
    uint32_t best = 0u;
    for (uint32_t i = b + threadIdx.x; i < e; i += 256) {
        const float mag = grad_mag(grad[(size_t)i * 3], grad[(size_t)i * 3 + 1], grad[(size_t)i * 3 + 2]);
        if (isfinite(mag)) best = max(best, __float_as_uint(mag));
    }
    __shared__ uint32_t red[4];
    best = block_max_u32(best, red);
    if (threadIdx.x == 0) gmax[o] = __uint_as_float(best);
}

struct RiftArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4* sp4;
    const uint32_t* kp_off; const float *kx, *ky, *kz;
    const float *grad, *gmax;
    float radius, r2;
    int nd, ng;
    float d_scale, a_scale;               // divisors of the two bin coordinates: Radius + FLT_EPSILON, (float)M_PI + FLT_EPSILON
    float* desc; uint32_t* count;
    int n_obj, nbx;
    const uint32_t* kp_perm;
};

// 12 KiB static LDS per workgroup: four histograms of 256 bins, four row tables
__global__ __launch_bounds__(256) void k_rift(RiftArgs a) {
    __shared__ __attribute__((aligned(16))) shot_bin_t s_hist[4][RIFT_MAX_BINS];
    __shared__ WaveRows s_rows[4];
    ShotWave w;
    const int nd = a.nd, ng = a.ng, D = nd * ng;
    if (!shot_wave_place(a, D, w)) return;
    if (!shot_wave_ball(a, D, w, w.m.n_finite > 0)) return;   // D4: a ball that misses the grid holds no point -> NaN row, count 0
    const int lane = w.lane;
    shot_bin_t* hist = s_hist[w.wv];
    for (int i = lane; i < D; i += 64) hist[i] = 0ull;
    const uint32_t base = a.pt_off[w.o];
    const uint32_t* cs = a.cell_start + (size_t)w.o * ISM_GRID_STRIDE;
    int eg = 0; (void)frexpf(a.gmax[w.o], &eg);          // every finite |g| of the object < 2^eg
    const double fix = ldexp(1.0, rift_bits(w.m.n_finite, 40) - eg);
    const float fnd = (float)nd, fng = (float)ng;
    int cnt = 0;
    bool bad = false;                                    // a ball point whose gradient is not finite: the whole row NaN
    ball_for_each<8, true>(w.m, cs, w.cr, w.cx, w.cy, w.cz, a.radius, lane, s_rows[w.wv],
                  [&](uint32_t t, bool) { return a.sp4[base + t]; },
                  [&](const float4& p, uint32_t, bool v) {
        if (!v) return;
        const float d2 = sqdist3(p.x, p.y, p.z, w.cx, w.cy, w.cz);
        if (!(d2 < a.r2)) return;
        cnt++;
        const float* g = a.grad + (size_t)(base + __float_as_uint(p.w)) * 3;
        const float gx = g[0], gy = g[1], gz = g[2];
        const float mag = grad_mag(gx, gy, gz);
        if (!isfinite(mag)) { bad = true; return; }
        if (mag == 0.f) return;                          // every deposit is 0
        const float ux = p.x - w.cx, uy = p.y - w.cy, uz = p.z - w.cz;
        const float cx = gy * uz - gz * uy, cy = gz * ux - gx * uz, cz = gx * uy - gy * ux;
        const float sn = sqrtf((cx * cx + cy * cy) + cz * cz), cs_ = (gx * ux + gy * uy) + gz * uz;
        const float angle = (sn == 0.f && cs_ == 0.f) ? 0.f : shot_atan2(sn, cs_);   // D3; u = 0: angle 0
        const float d = fnd * sqrtf(d2) / a.d_scale, an = fng * angle / a.a_scale;
        if (!(d >= 0.f && d <= fnd && an >= 0.f && an <= fng)) { bad = true; return; }   // products that overflowed
        // the bins within 1 of d and of an: floor and floor + 1 (a third one, at an integer coordinate, has weight 0)
        const int i0 = (int)floorf(d), j0 = (int)floorf(an);
        const float wd[2] = {1.f - fabsf(d - (float)i0), 1.f - fabsf(d - (float)(i0 + 1))};
        const float wa[2] = {1.f - fabsf(an - (float)j0), 1.f - fabsf(an - (float)(j0 + 1))};
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int gj = (j0 + jj) % ng;               // cyclic in the angle (0 <= j0 <= ng)
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int di = i0 + ii;
                const float dep = (wd[ii] * wa[jj]) * mag;
                if (di > nd - 1 || gj > ng - 1 || !(dep > 0.f)) continue;   // past the last distance bin: dropped
                atomicAdd(&hist[gj * nd + di], (shot_bin_t)__double2ull_rn((double)dep * fix));
            }
        }
    });
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the deposits of the other lanes are read below
    cnt = wave_sum_i(cnt);
    const bool nan_row = __ballot(bad) != 0ull || cnt == 0;
    double ss = 0.0;                                     // a fixed bin -> lane map and a fixed reduction: the same bits whatever the ball's order
    for (int i = lane; i < D; i += 64) { const double h = (double)hist[i]; ss += h * h; }
    ss = wave_sum_d(ss);
    const double norm = sqrt(ss);
    for (int i = lane; i < D; i += 64)
        w.row[i] = nan_row ? __builtin_nanf("") : (ss > 0.0 ? (float)((double)hist[i] / norm) : 0.f);
    if (a.count && lane == 0) a.count[w.k] = (uint32_t)cnt;
}

RiftView view_of(const ismhip_cloud* c) {
    RiftView v;
    v.pt_off = c->pt_off; v.meta = c->meta; v.cell_start = c->cell_start; v.sp4 = c->sp4; v.sn4 = c->sn4;
    v.n_obj = c->n_obj; v.nbx = (int)((c->max_pts + 255) / 256);
    if (v.nbx < 1) v.nbx = 1;
    return v;
}

// r2 and the power of two above it; false: the radius is not positive and finite, or its square leaves the range of the grids
bool radius_ok(float radius, float& r2, int& e2) {
    if (!(radius > 0.f) || !std::isfinite(radius)) return false;
    r2 = (float)((double)radius * (double)radius);
    if (!(r2 > 0.f) || !std::isfinite(r2)) return false;
    (void)std::frexp((double)r2, &e2);
    return e2 > -900 && e2 < 900;
}

}  // namespace

extern "C" {

int ismhip_intensity_gradients(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, float* grad_out, uint32_t* count_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    float r2 = 0.f; int e2 = 0;
    if (!cloud || !radius_ok(radius, r2, e2)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "intensity_gradients: bad argument");
    if (!cloud->rgba) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "intensity_gradients: colour arrays missing");
    const size_t n = cloud->n_pts;
    if (n == 0) return ISMHIP_OK;
    if (!grad_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "intensity_gradients: grad_out is NULL");
    float* si = (float*)ism_scratch(ctx, SCR_RIFT, n * sizeof(float));
    if (!si) return ISMHIP_ERR_NOMEM;
    TimerScope ts(ctx, "intensity_gradients");
    // points that are not finite, balls of fewer than three points and points without a finite normal: NaN (count 0 for the first)
    ISM_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)grad_out, 0x7fc00000, n * 3, ctx->stream));
    if (count_out) ISM_HIP(ctx, hipMemsetAsync(count_out, 0, n * 4, ctx->stream));
    const RiftView cv = view_of(cloud);
    const dim3 grid(xcd_object_grid((unsigned)cv.nbx, cv.n_obj));
    hipLaunchKernelGGL(k_rift_intensity, grid, dim3(256), 0, ctx->stream, cv, cloud->rgba, si);
    ISM_CHECK_LAUNCH(ctx, "k_rift_intensity");
    hipLaunchKernelGGL(k_rift_gradient, grid, dim3(256), 0, ctx->stream, cv, si, radius, r2, e2, grad_out, count_out);
    ISM_CHECK_LAUNCH(ctx, "k_rift_gradient");
    return ISMHIP_OK;
}

int ismhip_rift(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h, const float* kpx, const float* kpy, const float* kpz,
                float radius, int n_distance_bins, int n_gradient_bins, const float* grad, float* desc_out, uint32_t* neighbour_count_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    float r2 = 0.f; int e2 = 0;
    if (!cloud || !kp_offsets_h || !radius_ok(radius, r2, e2) || n_distance_bins < 1 || n_gradient_bins < 1)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rift: bad argument");
    if (!cloud->rgba) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rift: colour arrays missing");
    if ((long long)n_distance_bins * n_gradient_bins > RIFT_MAX_BINS)
        return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "rift: more than 256 bins (n_distance_bins * n_gradient_bins)");
    RaggedOffsets kp;
    int rc = ism_ragged_offsets(ctx, "rift", kp_offsets_h, cloud->n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK || kp.max_run == 0) return rc;
    if (!kpx || !kpy || !kpz || !desc_out || (!grad && cloud->n_pts > 0))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "rift: keypoint, gradient or output array is NULL");
    float* gmax = (float*)ism_scratch(ctx, SCR_RIFT_SCALE, (size_t)cloud->n_obj * sizeof(float));
    if (!gmax) return ISMHIP_ERR_NOMEM;
    RiftArgs a = {};
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.cell_start = cloud->cell_start; a.sp4 = cloud->sp4;
    a.kp_off = kp.dev; a.kx = kpx; a.ky = kpy; a.kz = kpz;
    a.grad = grad; a.gmax = gmax;
    a.radius = radius; a.r2 = r2;
    a.nd = n_distance_bins; a.ng = n_gradient_bins;
    a.d_scale = radius + FLT_EPSILON; a.a_scale = (float)M_PI + FLT_EPSILON;
    a.desc = desc_out; a.count = neighbour_count_out;
    a.n_obj = ctx->xcd_map ? cloud->n_obj : 0; a.nbx = (int)((kp.max_run + 3) / 4);
    TimerScope ts(ctx, "rift");
    hipLaunchKernelGGL(k_rift_gmax, dim3(cloud->n_obj), dim3(256), 0, ctx->stream, cloud->pt_off, grad, gmax);
    ISM_CHECK_LAUNCH(ctx, "k_rift_gmax");
    a.kp_perm = ism_kp_order(ctx, cloud, kp_offsets_h, a.kp_off, kpx, kpy, kpz, kp.max_run);
    const dim3 grid(ctx->xcd_map ? xcd_object_grid((unsigned)a.nbx, cloud->n_obj) : (unsigned)a.nbx * (unsigned)cloud->n_obj);
    hipLaunchKernelGGL(k_rift, grid, dim3(256), 0, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_rift");
    return ISMHIP_OK;
}

}  // extern "C"

// iss3d.hip — ISS3D keypoints (Keypoints type "ISS3D") on the device.
// Reference seam: KeypointsISS3D::iComputeKeypoints (keypoints/keypoints_iss3d.cpp:31-72) -> pcl::ISSKeypoint3D without border estimation
// (the reference never sets BorderRadius; NormalRadius is unused). PCL is external: the arithmetic is this library's definition
// (restated from PCL 1.10 iss_3d.hpp in tests/iss3d_ref.py).
//
// Per object, on the finite points of the cloud, every neighbourhood by the rule of ismhip_filter_radius (unfused float d2, strictly
// below (float)((double)r * r), the query included):
//   k_iss_saliency[_wave]   : scatter matrix about the query over the SalientRadius ball, 3x3 eigen-solve (eigen3.h), the two ratio
//                             tests -> saliency = smallest eigenvalue or 0, in original point order and in cell-sorted order
//   k_iss_nms               : one thread per candidate (saliency > 0) in cell-sorted order, second sweep over the NonMaxRadius ball: at
//                             least MinNeighbors neighbours and none with a strictly larger saliency; ends at the first larger one
//   ism_compact_keypoints   : the mask -> ordered compaction of compact.hip
//
// The scatter sums are ORDER FREE. Every product d_a * d_b (double) is rounded to a multiple of q = 2^(e - 44), 2^e the power of two
// above r^2, by adding 1.5 * 2^(e + 8) -- the sum's mantissa then holds the rounded product as an integer -- and the integers are
// added. |d_a d_b| < 2^e, so a term is below 2^44 in units of q and 2^18 neighbours fit 64 bits with room to spare (a batch with a
// larger object takes fewer bits, iss_saliency). Rounding error per term q / 2, i.e. about 1e-13 of the largest eigenvalue whatever
// the neighbour count. Bought with it: the result does not depend on the cell size the cloud was made with, on the lane a neighbour
// lands in, on the mapping of queries to lanes (the two saliency kernels give the same bits) or on the run. Cost: DMUL + DADD + a
// 64-bit integer add per entry instead of one DFMA.
//
// Query-to-lane mapping of the saliency sweep, measured (256 objects of 16384 points, 258 neighbours per query): one
// thread per query in cell order on ball_rows_for_each, as k_ror_count (prefilter.hip), 5.7 ms; one wave per query on ball_for_each,
// as k_pca_normals (lrf.hip), 13.6 ms (that sibling itself: 14.7 ms). Every point is a query here, so the 64 queries of a wave sit in
// the same few cells and read the same runs of records, where a wave per query pays its row set-up, its six 64-bit wave reductions
// and a mostly idle wave at the eigen-solve for every single point. The thread mapping is the default; the wave mapping stays behind
// ISMHIP_ISS3D_MAP=wave for A/B runs.
#include "common.h"
#include "eigen3.h"
#include <cmath>

namespace {

struct IssView {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4* sp4;
    int n_obj, nbx;
};
struct IssParams {
    float radius, r2;
    double magic, quantum;        // 1.5 * 2^(e + 8) and 2^(e - 44), see the head of the file
    double gamma21, gamma32;
    int min_nb;
};
struct IssOut { double* saliency; double* saliency_sorted; double* eig; uint32_t* count; };

// the six entries of d d^T on the integer grid
struct Scatter {
    long long xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
    __device__ __forceinline__ void add(const IssParams& P, const float4& p, const float4& q) {
        const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
        const long long m0 = __double_as_longlong(P.magic);
        xx += __double_as_longlong(dx * dx + P.magic) - m0; xy += __double_as_longlong(dx * dy + P.magic) - m0;
        xz += __double_as_longlong(dx * dz + P.magic) - m0; yy += __double_as_longlong(dy * dy + P.magic) - m0;
        yz += __double_as_longlong(dy * dz + P.magic) - m0; zz += __double_as_longlong(dz * dz + P.magic) - m0;
    }
};

// eigenvalues, ratio tests and the stores of one query (one thread)
__device__ __forceinline__ void iss_finish(const IssParams& P, const IssOut& out, const Scatter& s, int cnt, uint32_t orig, uint32_t sorted) {
    double e1 = 0.0, e2 = 0.0, e3 = 0.0, sal = 0.0;
    if (cnt >= P.min_nb) {
        const double xx = (double)s.xx * P.quantum, xy = (double)s.xy * P.quantum, xz = (double)s.xz * P.quantum;
        const double yy = (double)s.yy * P.quantum, yz = (double)s.yz * P.quantum, zz = (double)s.zz * P.quantum;
        double A[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}}, w[3], V[3][3];
        eigen_sym3(A, w, V);
        e1 = w[2]; e2 = w[1]; e3 = w[0];
        if (isfinite(e1) && isfinite(e2) && isfinite(e3) && !(e3 < 0.0) && e2 / e1 < P.gamma21 && e3 / e2 < P.gamma32) sal = e3;
    }
    out.saliency[orig] = sal;
    if (out.saliency_sorted) out.saliency_sorted[sorted] = sal;
    if (out.eig) { out.eig[(size_t)orig * 3] = e1; out.eig[(size_t)orig * 3 + 1] = e2; out.eig[(size_t)orig * 3 + 2] = e3; }
    if (out.count) out.count[orig] = (uint32_t)cnt;
}

// one wave per (cell-sorted) point, the sweep of k_pca_normals (A/B runs only)
__global__ __launch_bounds__(256) void k_iss_saliency_wave(IssView cv, IssParams P, IssOut out) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t sidx = (uint32_t)bx * 4 + (threadIdx.x >> 6);
    if (sidx >= m.n_finite) return;
    const int lane = lane_id();
    const uint32_t base = cv.pt_off[o];
    const float4 q = cv.sp4[base + sidx];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    CellRange cr;
    Scatter s;
    int cnt = 0;
    __shared__ WaveRows s_rows[4];
    if (ball_cells(m, q.x, q.y, q.z, P.radius, cr))
        ball_for_each(m, cs, cr, q.x, q.y, q.z, P.radius, lane, s_rows[threadIdx.x >> 6],
                      [&](uint32_t t, bool) { return cv.sp4[base + t]; },
                      [&](const float4& p, uint32_t, bool v) {
            if (!v) return;
            if (sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < P.r2) { s.add(P, p, q); cnt++; }
        });
    s.xx = (long long)wave_sum_u64((unsigned long long)s.xx); s.xy = (long long)wave_sum_u64((unsigned long long)s.xy);
    s.xz = (long long)wave_sum_u64((unsigned long long)s.xz); s.yy = (long long)wave_sum_u64((unsigned long long)s.yy);
    s.yz = (long long)wave_sum_u64((unsigned long long)s.yz); s.zz = (long long)wave_sum_u64((unsigned long long)s.zz);
    cnt = wave_sum_i(cnt);
    if (lane != 0) return;
    iss_finish(P, out, s, cnt, base + __float_as_uint(q.w), base + sidx);
}

// one thread per (cell-sorted) point, the sweep of k_ror_count. Four records in flight per lane (the span loop of k_sor_meandist) bought
// nothing here: 5.82 against 5.66 ms on the batch of DESIGN.md §4.14.
__global__ __launch_bounds__(256) void k_iss_saliency(IssView cv, IssParams P, IssOut out) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q = cv.sp4[base + t];
    Scatter s;
    int cnt = 0;
    ball_rows_for_each(m, cs, q.x, q.y, q.z, P.radius, [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = cv.sp4[base + i];
            if (sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < P.r2) { s.add(P, p, q); cnt++; }
        }
        return true;
    });
    iss_finish(P, out, s, cnt, base + __float_as_uint(q.w), base + t);
}

// keep[original index] = 1 for the keypoints; the mask was cleared before (non-finite points stay 0)
__global__ __launch_bounds__(256) void k_iss_nms(IssView cv, float radius, float r2, int min_nb, const double* __restrict__ sal_sorted,
                                                 uint8_t* __restrict__ keep) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const double mine = sal_sorted[base + t];
    if (!(mine > 0.0)) return;
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q = cv.sp4[base + t];
    int cnt = 0;
    bool beaten = false;
    ball_rows_for_each(m, cs, q.x, q.y, q.z, radius, [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = cv.sp4[base + i];
            const double other = sal_sorted[base + i];
            if (sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < r2) { cnt++; beaten |= mine < other; }
        }
        return !beaten;
    });
    if (!beaten && cnt >= min_nb) keep[base + __float_as_uint(q.w)] = 1;
}

IssView view_of(const ismhip_cloud* c, unsigned per_block) {
    IssView v;
    v.pt_off = c->pt_off; v.meta = c->meta; v.cell_start = c->cell_start; v.sp4 = c->sp4;
    v.n_obj = c->n_obj; v.nbx = (int)((c->max_pts + per_block - 1) / per_block);
    if (v.nbx < 1) v.nbx = 1;
    return v;
}

bool positive(double v) { return v > 0.0 && std::isfinite(v); }

// the saliency pass; saliency / saliency_sorted: device [n_pts] (the latter may be NULL)
int iss_saliency(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, double gamma21, double gamma32, int min_nb, const IssOut& out) {
    const size_t n = cloud->n_pts;
    IssParams P;
    P.radius = radius; P.r2 = (float)((double)radius * (double)radius);
    int e = 0; (void)std::frexp((double)P.r2, &e);                  // r2 < 2^e
    if (e < -900 || e > 900) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "iss3d: radius out of range");
    // 44 bits per term; a batch with an object of more than 2^18 points takes a coarser grid so that a ball holding them all still fits
    int bits = 44;
    while (bits > 24 && ((unsigned long long)cloud->max_pts << bits) >= (1ull << 62)) --bits;
    P.magic = std::ldexp(1.5, e - bits + 52); P.quantum = std::ldexp(1.0, e - bits);
    P.gamma21 = gamma21; P.gamma32 = gamma32; P.min_nb = min_nb;
    TimerScope ts(ctx, "iss3d_saliency");
    // points that are not finite never enter the sorted copy: saliency, eigenvalues and count 0
    ISM_HIP(ctx, hipMemsetAsync(out.saliency, 0, n * 8, ctx->stream));
    if (out.eig) ISM_HIP(ctx, hipMemsetAsync(out.eig, 0, n * 24, ctx->stream));
    if (out.count) ISM_HIP(ctx, hipMemsetAsync(out.count, 0, n * 4, ctx->stream));
    if (ctx->iss3d_wave) {
        const IssView cv = view_of(cloud, 4);
        hipLaunchKernelGGL(k_iss_saliency_wave, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(256), 0, ctx->stream, cv, P, out);
    } else {
        const IssView cv = view_of(cloud, 256);
        hipLaunchKernelGGL(k_iss_saliency, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(256), 0, ctx->stream, cv, P, out);
    }
    ISM_CHECK_LAUNCH(ctx, "k_iss_saliency");
    return ISMHIP_OK;
}

}  // namespace

extern "C" {

int ismhip_iss3d_saliency(ismhip_ctx* ctx, const ismhip_cloud* cloud, float salient_radius, double gamma21, double gamma32, int min_neighbors,
                          double* saliency_out, double* eig_out, uint32_t* count_out) {
    if (!ctx || !cloud || !positive(salient_radius) || !positive(gamma21) || !positive(gamma32) || min_neighbors < 0)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "iss3d_saliency: bad argument");
    if (cloud->n_pts == 0) return ISMHIP_OK;
    if (!saliency_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "iss3d_saliency: saliency_out is NULL");
    return iss_saliency(ctx, cloud, salient_radius, gamma21, gamma32, min_neighbors, IssOut{saliency_out, nullptr, eig_out, count_out});
}

int ismhip_iss3d_keypoints(ismhip_ctx* ctx, const ismhip_cloud* cloud, float salient_radius, float non_max_radius, double gamma21, double gamma32,
                           int min_neighbors, uint32_t capacity, float* kx, float* ky, float* kz, uint32_t* krgba, uint32_t* src_index_out,
                           uint32_t* kp_offsets_h_out) {
    if (!ctx || !cloud || !kx || !ky || !kz || !kp_offsets_h_out || !positive(salient_radius) || !positive(non_max_radius) || !positive(gamma21) ||
        !positive(gamma32) || min_neighbors < 0)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "iss3d_keypoints: bad argument");
    for (int o = 0; o <= cloud->n_obj; ++o) kp_offsets_h_out[o] = 0;
    const size_t n = cloud->n_pts;
    if (n == 0) return ISMHIP_OK;
    // one scratch block: [saliency, original order] [saliency, cell order] [keep mask]
    char* scr = (char*)ism_scratch(ctx, SCR_ISS3D, n * 17);
    if (!scr) return ISMHIP_ERR_NOMEM;
    double* sal = (double*)scr; double* sal_sorted = sal + n;
    uint8_t* keep = (uint8_t*)(sal_sorted + n);
    int rc = iss_saliency(ctx, cloud, salient_radius, gamma21, gamma32, min_neighbors, IssOut{sal, sal_sorted, nullptr, nullptr});
    if (rc != ISMHIP_OK) return rc;
    {
        TimerScope ts(ctx, "iss3d_nms");
        ISM_HIP(ctx, hipMemsetAsync(keep, 0, n, ctx->stream));
        const IssView cv = view_of(cloud, 256);
        hipLaunchKernelGGL(k_iss_nms, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(256), 0, ctx->stream, cv, non_max_radius,
                           (float)((double)non_max_radius * (double)non_max_radius), min_neighbors, sal_sorted, keep);
        ISM_CHECK_LAUNCH(ctx, "k_iss_nms");
    }
    return ism_compact_keypoints(ctx, "iss3d_keypoints", cloud, keep, capacity, kx, ky, kz, krgba, src_index_out, kp_offsets_h_out);
}

}  // extern "C"

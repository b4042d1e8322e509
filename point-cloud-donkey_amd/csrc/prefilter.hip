// prefilter.hip — point-cloud pre-filters in front of normals / keypoints / features.
// Reference: ImplicitShapeModel::computeFeatures (implicit_shape_model.cpp:739-758, :810-821) -> pcl::StatisticalOutlierRemoval,
// pcl::RadiusOutlierRemoval (radius-search branch: the reference's clouds are is_dense = false) and pcl::PassThrough on z. PCL is
// external: the arithmetic is this library's definition, restated in tests/prefilter_ref.py.
//
// Both searches run over the caller's ismhip_cloud: the per-object grid and the cell-sorted 16-byte point records of grid.hip. A
// query is a point of the cloud itself, so ONE THREAD takes one query and the threads of a block walk the cell-sorted order: the 64
// queries of a wave sit in the same or in adjacent cells and read the same x-runs of candidate records (the wave-per-query sweep of
// lrf.hip / shot.hip is laid out for a few thousand keypoints per object, not for every point).
#include "common.h"
#include "knn_box.h"
#include <cfloat>
#include <cmath>

namespace {

#define SOR_BLOCK 128          // threads (queries) per block of k_sor_meandist; the candidate lists take (MeanK + 1) * 128 * 4 bytes of LDS
#define SOR_STEPS 3            // box growth steps of the per-thread search (radius 0, half the smallest cell edge, the largest cell edge) before the wave scan takes over
#define SOR_SCAN_NBX 16        // blocks (4 waves each) per object of the scan kernel; each wave strides over the object's open queries

struct SorView {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4* sp4;
    int n_obj, nbx;
};

// ascending double sum of the square roots of list[1 .. k] (list[0], the query itself, is dropped) over k, rounded to float
template <class G>
__device__ __forceinline__ float sor_mean(int k, G&& get) {
    double s = 0.0;
    for (int j = 1; j <= k; ++j) s += sqrt((double)get(j));
    return (float)(s / (double)k);
}

// Exact (k + 1) smallest squared distances of every finite point to the finite points of its object, by the growing box of cells of
// knn_box.h. Queries still open after SOR_STEPS steps (isolated outliers: their neighbours are many cells away, and a lane that walked
// there would hold its whole wave) are appended to `open_list` for k_sor_scan.
__global__ __launch_bounds__(SOR_BLOCK) void k_sor_meandist(SorView cv, int k, float* __restrict__ mean_dist,
                                                            uint32_t* __restrict__ open_count, uint32_t* __restrict__ open_list) {
    extern __shared__ float s_list[];                     // [k + 1][SOR_BLOCK]: slot j of thread t at j * SOR_BLOCK + t (conflict free)
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * SOR_BLOCK + threadIdx.x;
    if ((int)m.n_finite < k + 1 || t >= m.n_finite) return;      // small objects are kept whole (k_sor_threshold)
    const uint32_t base = cv.pt_off[o];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q4 = cv.sp4[base + t];
    const float q[3] = {q4.x, q4.y, q4.z};
    // The list is kept UNSORTED while it is filled: a candidate below the current (k + 1)-th value overwrites the slot that holds that
    // value and the new maximum is found by reading the k + 1 slots again -- independent LDS reads that pipeline, where a sorted
    // insertion is a chain of dependent read-compare-write steps that the whole wave waits for. It is sorted once, at the end.
    float* L = s_list + threadIdx.x;
    for (int j = 0; j <= k; ++j) L[j * SOR_BLOCK] = INFINITY;
    float kth = INFINITY;                                  // the largest value of the full list; +inf while it is being filled
    int cnt = 0, kpos = 0;
    auto consider = [&](float d2) {
        if (!(d2 < kth)) return;
        if (cnt <= k) { L[cnt * SOR_BLOCK] = d2; if (++cnt <= k) return; }
        else L[kpos * SOR_BLOCK] = d2;
        float mx = -1.f;
        for (int j0 = 0; j0 <= k; j0 += 8) {               // eight independent reads per wait
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = L[min(j0 + u, k) * SOR_BLOCK];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (v[u] > mx) { mx = v[u]; kpos = min(j0 + u, k); }
        }
        kth = mx;
    };
    auto span = [&](uint32_t b, uint32_t e) {              // four records in flight per lane
        for (uint32_t i = b; i < e; i += 4) {
            float4 p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = cv.sp4[base + min(i + u, e - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + u < e) consider(sqdist3(p[u].x, p[u].y, p[u].z, q[0], q[1], q[2]));
        }
    };
    const bool done = knn_box_search(m, cs, q, SOR_STEPS, kth, span);
    const uint32_t me = __float_as_uint(q4.w);
    if (done) {
        for (int i = 1; i <= k; ++i) {                      // insertion sort, ascending
            const float v = L[i * SOR_BLOCK];
            int j = i;
            while (j > 0 && L[(j - 1) * SOR_BLOCK] > v) { L[j * SOR_BLOCK] = L[(j - 1) * SOR_BLOCK]; --j; }
            L[j * SOR_BLOCK] = v;
        }
        mean_dist[base + me] = sor_mean(k, [&](int j) { return L[j * SOR_BLOCK]; });
    }
    // open queries: one list per object inside the object's own point range, one atomic per wave (a wave never spans two objects).
    // The arrival order only decides WHICH wave scans a query, never its value.
    const unsigned long long open = __ballot(!done);
    if (open) {
        const int leader = __ffsll((long long)open) - 1;
        uint32_t pos = 0;
        if (lane_id() == leader) pos = atomicAdd(&open_count[o], (uint32_t)__popcll(open));
        pos = __shfl(pos, leader, 64) + (uint32_t)__popcll(open & ((1ull << lane_id()) - 1ull));
        if (!done) open_list[base + pos] = t;
    }
}

// The bounded path: one wave per open query reads the object's n_finite point records once (coalesced, 64 per step) and keeps the
// k + 1 smallest squared distances in a sorted list spread over the lanes (slot l in lane l, slot 64 in lane 0). A candidate below
// the current (k + 1)-th value is inserted by one wave-wide shift. The list ends as the same multiset the box search would have
// found and is summed in the same order, so the two paths are interchangeable bit for bit.
__global__ __launch_bounds__(256) void k_sor_scan(SorView cv, int k, float* __restrict__ mean_dist,
                                                  const uint32_t* __restrict__ open_count, const uint32_t* __restrict__ open_list) {
    __shared__ float s_l[4][65];
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;        // an object's scans run on one XCD: its records stay in that L2
    const int w = threadIdx.x >> 6, lane = lane_id();
    const uint32_t n_open = open_count[o];
    const uint32_t base = cv.pt_off[o], n = cv.meta[o].n_finite;
    for (uint32_t qi = (uint32_t)bx * 4 + w; qi < n_open; qi += (uint32_t)cv.nbx * 4) {
        const float4 q4 = cv.sp4[base + open_list[base + qi]];
        float a0 = INFINITY, a1 = INFINITY, kth = INFINITY;
        for (uint32_t i0 = 0; i0 < n; i0 += 256) {           // four coalesced 1 KB loads in flight
            float4 p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const uint32_t i = i0 + u * 64 + lane; p[u] = cv.sp4[base + (i < n ? i : 0u)]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = i0 + u * 64 + lane;
                const float d2 = sqdist3(p[u].x, p[u].y, p[u].z, q4.x, q4.y, q4.z);
                unsigned long long pend = __ballot(i < n && d2 < kth);
                while (pend) {
                    const int l = __ffsll((long long)pend) - 1;
                    pend &= pend - 1;
                    const float v = __shfl(d2, l, 64);
                    if (!(v < kth)) continue;              // kth has dropped since the ballot (wave-uniform)
                    float left = __shfl_up(a0, 1, 64);
                    if (lane == 0) left = -INFINITY;
                    const float a63 = __shfl(a0, 63, 64);
                    a1 = a1 <= v ? a1 : (a63 <= v ? v : a63);
                    a0 = a0 <= v ? a0 : (left <= v ? v : left);
                    kth = k < 64 ? __shfl(a0, k, 64) : __shfl(a1, 0, 64);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        s_l[w][lane] = a0;
        if (lane == 0) s_l[w][64] = a1;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane == 0) mean_dist[base + __float_as_uint(q4.w)] = sor_mean(k, [&](int j) { return s_l[w][j]; });
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// One block per object: mean and variance of the finite points' mean distances in double, in a FIXED order (thread t sums the
// points t, t + 256, ... ascending; the DPP tree of wave_sum_d; the four wave partials in wave order: block_sum_d_left of common.h),
// threshold, then the mask.
__global__ __launch_bounds__(256) void k_sor_threshold(const uint32_t* __restrict__ pt_off, const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ z, int k, double mul, float* __restrict__ mean_dist,
                                                       uint8_t* __restrict__ keep, double* __restrict__ thr_out) {
    const int o = blockIdx.x;
    const uint32_t b = pt_off[o], e = pt_off[o + 1];
    __shared__ double s_d[4];
    __shared__ uint32_t s_n[4];
    double sum = 0.0, sq = 0.0; uint32_t n = 0;
    for (uint32_t i = b + threadIdx.x; i < e; i += 256)
        if (isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i])) { n++; }
    const uint32_t nf = block_sum_i(n, s_n);
    const bool small = nf < (uint32_t)(k + 1);                 // fewer than MeanK + 1 finite points: the object is kept whole
    if (!small)
        for (uint32_t i = b + threadIdx.x; i < e; i += 256)
            if (isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i])) { const double d = (double)mean_dist[i]; sum += d; sq += d * d; }
    const double S = block_sum_d_left(sum, s_d), Q = block_sum_d_left(sq, s_d);
    double thr = INFINITY;
    if (!small) {
        const double N = (double)nf;
        const double mean = S / N, var = (Q - S * S / N) / (N - 1.0);
        thr = mean + mul * sqrt(var);
    }
    if (threadIdx.x == 0) thr_out[o] = thr;
    for (uint32_t i = b + threadIdx.x; i < e; i += 256) {
        const bool fin = isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i]);
        if (!fin || small) mean_dist[i] = __builtin_nanf("");
        keep[i] = !fin ? 0 : (small ? 1 : (!((double)mean_dist[i] > thr) ? 1 : 0));
    }
}

// count of the object's finite points with d2 < r2 (the query included), one thread per query in cell-sorted order. The rows of
// cells the ball touches and the chord of every row come from ball_cells / row_cells, as for the descriptors (ball_rows_for_each).
template <bool FULL>
__global__ __launch_bounds__(256) void k_ror_count(SorView cv, float radius, float r2, int min_nb,
                                                   uint8_t* __restrict__ keep, uint32_t* __restrict__ count_out) {
    int o, bx;
    if (!xcd_object_block(cv.nbx, cv.n_obj, o, bx)) return;
    const GridMeta m = cv.meta[o];
    const uint32_t t = (uint32_t)bx * 256 + threadIdx.x;
    if (t >= m.n_finite) return;
    const uint32_t base = cv.pt_off[o];
    const uint32_t* cs = cv.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const float4 q = cv.sp4[base + t];
    int cnt = 0;
    if (FULL || cnt <= min_nb)            // a negative min_nb keeps the point without a sweep
        ball_rows_for_each(m, cs, q.x, q.y, q.z, radius, [&](uint32_t b, uint32_t e) {
            for (uint32_t i = b; i < e; ++i) {
                const float4 p = cv.sp4[base + i];
                cnt += sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < r2 ? 1 : 0;
            }
            return FULL || cnt <= min_nb;
        });
    const uint32_t me = base + __float_as_uint(q.w);
    keep[me] = cnt > min_nb ? 1 : 0;
    if (FULL) count_out[me] = (uint32_t)cnt;
}

// non-finite points of a cloud: mask 0, count 0 (the search kernels only visit the finite ones)
__global__ void k_clear_mask(uint32_t n, uint8_t* __restrict__ keep, uint32_t* __restrict__ count_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keep[i] = 0;
    if (count_out) count_out[i] = 0u;
}

__global__ void k_pass_z(uint32_t n, const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, float z_min, float z_max,
                         uint8_t* __restrict__ keep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float pz = z[i];
    keep[i] = (isfinite(x[i]) && isfinite(y[i]) && isfinite(pz) && !(pz < z_min || pz > z_max)) ? 1 : 0;
}

SorView view_of(const ismhip_cloud* c, unsigned block) {
    SorView v;
    v.pt_off = c->pt_off; v.meta = c->meta; v.cell_start = c->cell_start; v.sp4 = c->sp4;
    v.n_obj = c->n_obj; v.nbx = (int)((c->max_pts + block - 1) / block);
    if (v.nbx < 1) v.nbx = 1;
    return v;
}

}  // namespace

extern "C" {

int ismhip_filter_statistical(ismhip_ctx* ctx, const ismhip_cloud* cloud, int mean_k, float stddev_mul, uint8_t* keep_out,
                              float* mean_dist_out, double* threshold_h_out) {
    if (!ctx || !cloud || !keep_out || mean_k < 1) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "filter_statistical: bad argument");
    if (mean_k > ISMHIP_SOR_MAX_MEAN_K) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "filter_statistical: MeanK above ISMHIP_SOR_MAX_MEAN_K (64) is not built");
    if (cloud->n_pts == 0) { if (threshold_h_out) for (int o = 0; o < cloud->n_obj; ++o) threshold_h_out[o] = INFINITY; return ISMHIP_OK; }
    const size_t n = cloud->n_pts;
    // one scratch block: [thresholds] [open counters per object] [open lists, in the objects' point ranges] [mean distances, when the caller wants none]
    const size_t thr_bytes = (size_t)cloud->n_obj * 8, cnt_bytes = ((size_t)cloud->n_obj * 4 + 15) & ~(size_t)15, list_bytes = n * 4;
    char* scr = (char*)ism_scratch(ctx, SCR_PREFILTER, thr_bytes + cnt_bytes + list_bytes + (mean_dist_out ? 0 : n * 4));
    if (!scr) return ISMHIP_ERR_NOMEM;
    double* thr = (double*)scr;
    uint32_t* open_count = (uint32_t*)(scr + thr_bytes);
    uint32_t* open_list = (uint32_t*)(scr + thr_bytes + cnt_bytes);
    float* md = mean_dist_out ? mean_dist_out : (float*)(scr + thr_bytes + cnt_bytes + list_bytes);
    {
        TimerScope ts(ctx, "filter_sor");
        ISM_HIP(ctx, hipMemsetAsync(open_count, 0, (size_t)cloud->n_obj * 4, ctx->stream));
        SorView cv = view_of(cloud, SOR_BLOCK);
        hipLaunchKernelGGL(k_sor_meandist, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(SOR_BLOCK), (size_t)(mean_k + 1) * SOR_BLOCK * 4,
                           ctx->stream, cv, mean_k, md, open_count, open_list);
        ISM_CHECK_LAUNCH(ctx, "k_sor_meandist");
        cv.nbx = SOR_SCAN_NBX;
        hipLaunchKernelGGL(k_sor_scan, dim3(xcd_object_grid((unsigned)cv.nbx, cv.n_obj)), dim3(256), 0, ctx->stream, cv, mean_k, md, open_count, open_list);
        ISM_CHECK_LAUNCH(ctx, "k_sor_scan");
        hipLaunchKernelGGL(k_sor_threshold, dim3(cloud->n_obj), dim3(256), 0, ctx->stream, cloud->pt_off, cloud->x, cloud->y, cloud->z, mean_k,
                           (double)stddev_mul, md, keep_out, thr);
        ISM_CHECK_LAUNCH(ctx, "k_sor_threshold");
    }
    if (threshold_h_out) ISM_HIP(ctx, hipMemcpyAsync(threshold_h_out, thr, thr_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ISMHIP_OK;
}

int ismhip_filter_radius(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, int min_neighbors, uint8_t* keep_out, uint32_t* count_out) {
    if (!ctx || !cloud || !keep_out || !(radius > 0.f) || !std::isfinite(radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "filter_radius: bad argument");
    if (cloud->n_pts == 0) return ISMHIP_OK;
    const float r2 = (float)((double)radius * (double)radius);
    TimerScope ts(ctx, "filter_ror");
    hipLaunchKernelGGL(k_clear_mask, dim3((cloud->n_pts + 255) / 256), dim3(256), 0, ctx->stream, cloud->n_pts, keep_out, count_out);
    ISM_CHECK_LAUNCH(ctx, "k_clear_mask");
    const SorView cv = view_of(cloud, 256);
    const dim3 g(xcd_object_grid((unsigned)cv.nbx, cv.n_obj));
    if (count_out) hipLaunchKernelGGL(k_ror_count<true>, g, dim3(256), 0, ctx->stream, cv, radius, r2, min_neighbors, keep_out, count_out);
    else hipLaunchKernelGGL(k_ror_count<false>, g, dim3(256), 0, ctx->stream, cv, radius, r2, min_neighbors, keep_out, count_out);
    ISM_CHECK_LAUNCH(ctx, "k_ror_count");
    return ISMHIP_OK;
}

int ismhip_filter_passthrough_z(ismhip_ctx* ctx, uint32_t n_pts, const float* x, const float* y, const float* z, float z_min, float z_max,
                                uint8_t* keep_out) {
    if (!ctx || (n_pts && (!x || !y || !z || !keep_out))) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "filter_passthrough_z: bad argument");
    if (n_pts == 0) return ISMHIP_OK;
    hipLaunchKernelGGL(k_pass_z, dim3((n_pts + 255) / 256), dim3(256), 0, ctx->stream, n_pts, x, y, z, z_min, z_max, keep_out);
    ISM_CHECK_LAUNCH(ctx, "k_pass_z");
    return ISMHIP_OK;
}

}  // extern "C"

// cvfh.hip -- the clustered viewpoint feature histogram: ismhip_global_cvfh, the one region descriptor with MORE THAN ONE ROW per region.
// Reference seam: FeaturesCVFH::iComputeDescriptors (features/features_cvfh.cpp) -> pcl::CVFHEstimation. PCL is external: the arithmetic
// is this library's definition (include/ismhip.h; DESIGN.md section 4.25 names the deviations from PCL 1.10 cvfh.hpp / vfh.hpp).
//
// The region, n_sel, centroid and radius are k_global's (global.hip), bit for bit. Then, per region:
//   k_cvfh_region   one workgroup per region: count, centroid, radius (k_global's steps 1 and 2)
//   k_cvfh_init     DENSE: every (region, original point) starts unselected
//   k_cvfh_normals  DENSE, one thread per (region, cell-sorted point): the clustering normal of every selected point -- the PCA normal of
//                   the SELECTED points inside normal_radius, moments on the integer grids of moments.h (order free: the same bits for any
//                   cell size), or the cloud's own normal -- and parent[i] = i for a selected point
//   k_cvfh_link     DENSE, same shape: the ball sweep of the cluster tolerance enumerates the links (they are never stored); each link
//                   (i, j), j < i in ORIGINAL index, is one union: the larger root is hooked under the smaller with atomicMin
//   k_cvfh_flatten  DENSE: label[i] = root of i = the smallest original index of i's component, whatever order the hooks ran in;
//                   component sizes by integer atomicAdd
//   k_cvfh_select   one workgroup per region: the roots with size >= min_points in ascending index (ordered compaction): the kept
//                   clusters in PCL's seed order; n_clusters, never clipped; none kept and n_sel > 0: the one fallback row
//   k_cvfh_rows     one workgroup per (region, row): the cluster's centroid and mean normal on integer grids (order free), then the VFH
//                   deposit of vfh_deposit.h over ALL selected points of the region against that centroid and normal, per-wave copies of
//                   integer bins as k_vfh, the distance block normalised by the largest distance, the counts divided by 47278.0f
// The workspace is per (region, point) with the stride of the cloud's largest object: regions that overlap on one object do not
// interfere. No float atomics, no host round trip: every output is the same bits on every call and for every grid cell size.
#include "vfh_deposit.h"
#include "moments.h"
#include <cmath>

namespace {

#define CVFH_NONE 0xffffffffu
#define CVFH_NORM 47278.0f       /* features.cpp:282-297, normalizeDescriptors: the sum of the bin INDICES 0 .. 307 */

struct CvfhArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4 *sp4, *sn4;
    int n_obj; uint32_t stride, nbx;                         // workspace entries per region = the largest object; blocks of 256 per region
    const int32_t* reg_obj; const float* reg_center; const float* reg_radius;
    float vpx, vpy, vpz;
    float tol, tol2, nrad, nrad2; uint32_t min_points; double cos_thr;
    int max_rows;
    // workspace
    float4* wn4;                                             // clustering normal per (region, SORTED point)
    uint32_t* parent;                                        // per (region, ORIGINAL point): union-find parent; CVFH_NONE: not selected
    uint32_t* csize;                                         // per (region, original point): size of the component rooted there
    uint32_t* label;                                         // per (region, original point): the root; the caller's array when it asks for labels
    uint32_t* row_root;                                      // per (region, row): the kept cluster's root, CVFH_NONE for the fallback row
    // outputs
    uint32_t* n_sel; float* centroid; float* radius; uint32_t* n_clusters;
    float* row_centroid; float* row_normal; uint32_t* row_size; float* desc; uint32_t* counts;
};

struct CvfhRegion {
    uint32_t base, n, npts; GridMeta m; bool whole; float qx, qy, qz, r2s;
    __device__ __forceinline__ bool selected(const float4& p) const { return whole || sqdist3(p.x, p.y, p.z, qx, qy, qz) < r2s; }
};
__device__ __forceinline__ CvfhRegion cvfh_region(const CvfhArgs& a, uint32_t reg) {
    CvfhRegion g{};
    const int o = a.reg_obj[reg];
    if (o >= 0 && o < a.n_obj) {
        g.m = a.meta[o];
        g.base = a.pt_off[o]; g.npts = a.pt_off[o + 1] - g.base;
        g.n = g.m.n_finite < g.npts ? g.m.n_finite : g.npts;  // the sorted span holds the finite points first
    }
    g.qx = a.reg_center[reg * 3]; g.qy = a.reg_center[reg * 3 + 1]; g.qz = a.reg_center[reg * 3 + 2];
    const float rs = a.reg_radius[reg];
    g.whole = rs < 0.f;
    g.r2s = (float)((double)rs * (double)rs);
    return g;
}
__device__ __forceinline__ bool finite3(const float4& v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// ---- count, centroid, radius: k_global's steps 1 and 2 ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cvfh_region(CvfhArgs a) {
    __shared__ double red_d[4];
    __shared__ uint32_t red_u[4];
    __shared__ float red_f[4];
    const int tid = threadIdx.x;
    const uint32_t reg = blockIdx.x;
    const CvfhRegion g = cvfh_region(a, reg);
    const float4* sp = a.sp4 + g.base;
    const float qnan = __builtin_nanf("");
    uint32_t nsel; float cx, cy, cz;
    if (g.whole) {
        nsel = g.n; cx = g.m.centroid[0]; cy = g.m.centroid[1]; cz = g.m.centroid[2];
    } else {
        uint32_t c = 0; double sx = 0, sy = 0, sz = 0;
        for (uint32_t i = tid; i < g.n; i += 256) {
            const float4 p = sp[i];
            if (g.selected(p)) { sx += (double)p.x; sy += (double)p.y; sz += (double)p.z; c++; }
        }
        nsel = block_sum_i(c, red_u);
        sx = block_sum_d_left(sx, red_d); sy = block_sum_d_left(sy, red_d); sz = block_sum_d_left(sz, red_d);
        cx = (float)(sx / (double)nsel); cy = (float)(sy / (double)nsel); cz = (float)(sz / (double)nsel);
    }
    if (tid == 0) a.n_sel[reg] = nsel;
    if (nsel == 0) {                                          // workgroup-uniform
        if (tid < 3) a.centroid[reg * 3 + tid] = qnan;
        if (tid == 0) a.radius[reg] = 0.f;
        return;
    }
    if (tid == 0) { a.centroid[reg * 3] = cx; a.centroid[reg * 3 + 1] = cy; a.centroid[reg * 3 + 2] = cz; }
    float R = 0.f;
    for (uint32_t i = tid; i < g.n; i += 256) {
        const float4 p = sp[i];
        if (!g.selected(p)) continue;
        const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        const float d = sqrtf(dx * dx + dy * dy + dz * dz);
        if (d > R) R = d;
    }
    R = block_max_f(R, red_f);
    if (tid == 0) a.radius[reg] = R;
}

// every (region, original point) starts unselected: the points that are not finite never show up in the span and stay so
__global__ __launch_bounds__(256) void k_cvfh_init(CvfhArgs a) {
    const uint32_t reg = blockIdx.x / a.nbx, i = (blockIdx.x % a.nbx) * 256 + threadIdx.x;
    if (i >= a.stride) return;
    const size_t w = (size_t)reg * a.stride + i;
    a.parent[w] = CVFH_NONE; a.csize[w] = 0u; a.label[w] = CVFH_NONE;
}

// ---- clustering normals; the labelling starts -----------------------------------------------------------------------------------------------
// The covariance is k_pca_normals' (lrf.hip): moments of p - q over the ball, E[vv^T] - E[v]E[v]^T, eigen_sym3, the smallest eigenvalue's
// vector cast to float, flipped towards the viewpoint in float -- with the sums taken on the integer grids of moments.h instead of in
// traversal order.
__global__ __launch_bounds__(256) void k_cvfh_normals(CvfhArgs a) {
    const uint32_t reg = blockIdx.x / a.nbx, t = (blockIdx.x % a.nbx) * 256 + threadIdx.x;
    const CvfhRegion g = cvfh_region(a, reg);
    if (t >= g.n) return;
    const size_t w0 = (size_t)reg * a.stride;
    const float4* sp = a.sp4 + g.base;
    const float4 q = sp[t];
    const float qnan = __builtin_nanf("");
    float4 nrm = make_float4(qnan, qnan, qnan, 0.f);
    if (g.selected(q)) {
        const uint32_t orig = __float_as_uint(q.w);
        if (orig < g.npts) a.parent[w0 + orig] = orig;
        if (!(a.nrad > 0.f) || a.n_sel[reg] < a.min_points) {
            nrm = a.sn4[g.base + t];
        } else {
            const uint32_t* cs = a.cell_start + (size_t)a.reg_obj[reg] * ISM_GRID_STRIDE;
            const GridScale G = ball_grid_scale(a.nrad2, grid_bits(g.m.n_finite));
            Moments s;
            int cnt = 0;
            ball_rows_for_each(g.m, cs, q.x, q.y, q.z, a.nrad, [&](uint32_t b, uint32_t e) {
                for (uint32_t i = b; i < e; ++i) {
                    const float4 p = sp[i];
                    if (!(sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < a.nrad2) || !g.selected(p)) continue;
                    s.add(G, (double)p.x - (double)q.x, (double)p.y - (double)q.y, (double)p.z - (double)q.z);
                    cnt++;
                }
                return true;
            });
            if (cnt >= 3) {
                const double inv = 1.0 / (double)cnt;
                const double mx = ((double)s.x * G.q1) * inv, my = ((double)s.y * G.q1) * inv, mz = ((double)s.z * G.q1) * inv;
                const double xx = (double)s.xx * G.q2, xy = (double)s.xy * G.q2, xz = (double)s.xz * G.q2;
                const double yy = (double)s.yy * G.q2, yz = (double)s.yz * G.q2, zz = (double)s.zz * G.q2;
                double A[3][3] = {{xx * inv - mx * mx, xy * inv - mx * my, xz * inv - mx * mz}, {xy * inv - mx * my, yy * inv - my * my, yz * inv - my * mz},
                                  {xz * inv - mx * mz, yz * inv - my * mz, zz * inv - mz * mz}};
                double w[3], V[3][3];
                eigen_sym3(A, w, V);
                float n0 = (float)V[0][0], n1 = (float)V[1][0], n2 = (float)V[2][0];
                const float vx = a.vpx - q.x, vy = a.vpy - q.y, vz = a.vpz - q.z;   // flip when (viewpoint - point) . n < 0
                if (vx * n0 + vy * n1 + vz * n2 < 0) { n0 = -n0; n1 = -n1; n2 = -n2; }
                nrm = make_float4(n0, n1, n2, 0.f);
            }
        }
    }
    a.wn4[w0 + t] = nrm;
}

// ---- links and unions -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cvfh_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the root of x as far as this thread can see it: a parent is a smaller index of the same component (or x itself), so the walk ends
__device__ __forceinline__ uint32_t cvfh_find(const uint32_t* parent, uint32_t x) {
    for (;;) { const uint32_t p = cvfh_load(parent + x); if (p >= x) return x; x = p; }
}
// Joins the components of i and j. A stale view only costs another turn: atomicMin on a node that is no longer a root returns its
// parent, a smaller member of the same component, and the union goes on from there. Every store lowers a parent to a member of the
// same component, so the roots at the end are the component minima whatever the interleaving.
__device__ __forceinline__ void cvfh_union(uint32_t* parent, uint32_t i, uint32_t j) {
    for (;;) {
        i = cvfh_find(parent, i); j = cvfh_find(parent, j);
        if (i == j) return;
        if (i < j) { const uint32_t t = i; i = j; j = t; }    // i the larger root
        const uint32_t old = atomicMin(parent + i, j);
        if (old == i) return;                                 // i was a root and now hangs under j
        i = old;                                              // hooked in between: old < i, same component; join old and j
    }
}
// The link predicate on the normals (include/ismhip.h): the cosine in double from the float normals, clamped to [-1, 1]; the angle is
// below the threshold iff the clamped cosine is ABOVE cos(threshold), acos being decreasing: no acos on the device.
__device__ __forceinline__ bool cvfh_link(const float4& n1, const float4& n2, double cos_thr) {
    double d = ((double)n1.x * (double)n2.x + (double)n1.y * (double)n2.y) + (double)n1.z * (double)n2.z;
    d = d > 1.0 ? 1.0 : (d < -1.0 ? -1.0 : d);
    return d > cos_thr;
}
__global__ __launch_bounds__(256) void k_cvfh_link(CvfhArgs a) {
    const uint32_t reg = blockIdx.x / a.nbx, t = (blockIdx.x % a.nbx) * 256 + threadIdx.x;
    const CvfhRegion g = cvfh_region(a, reg);
    if (t >= g.n) return;
    const size_t w0 = (size_t)reg * a.stride;
    const float4* sp = a.sp4 + g.base;
    const float4 q = sp[t];
    if (!g.selected(q)) return;
    const float4 nq = a.wn4[w0 + t];
    if (!finite3(nq)) return;
    const uint32_t oi = __float_as_uint(q.w);
    if (oi >= g.npts) return;                                 // cannot happen: the record carries the index inside its object
    const uint32_t* cs = a.cell_start + (size_t)a.reg_obj[reg] * ISM_GRID_STRIDE;
    uint32_t* parent = a.parent + w0;
    ball_rows_for_each(g.m, cs, q.x, q.y, q.z, a.tol, [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; ++i) {
            const float4 p = sp[i];
            const uint32_t oj = __float_as_uint(p.w);
            if (oj >= oi) continue;                            // each link once, from its larger end
            if (!(sqdist3(p.x, p.y, p.z, q.x, q.y, q.z) < a.tol2) || !g.selected(p)) continue;
            const float4 np = a.wn4[w0 + i];
            if (!finite3(np) || !cvfh_link(nq, np, a.cos_thr)) continue;
            cvfh_union(parent, oi, oj);
        }
        return true;
    });
}
// label = root; sizes. k_cvfh_link has ended: every parent chain ends in its component's minimum, and nothing is stored into it here.
__global__ __launch_bounds__(256) void k_cvfh_flatten(CvfhArgs a) {
    const uint32_t reg = blockIdx.x / a.nbx, i = (blockIdx.x % a.nbx) * 256 + threadIdx.x;   // i: ORIGINAL index
    const CvfhRegion g = cvfh_region(a, reg);
    if (i >= g.npts) return;
    const size_t w0 = (size_t)reg * a.stride;
    if (a.parent[w0 + i] == CVFH_NONE) return;
    const uint32_t root = cvfh_find(a.parent + w0, i);
    a.label[w0 + i] = root;
    atomicAdd(a.csize + w0 + root, 1u);
}

// ---- kept clusters in ascending root ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cvfh_select(CvfhArgs a) {
    __shared__ BlockRank<256> rank;
    const uint32_t reg = blockIdx.x;
    const CvfhRegion g = cvfh_region(a, reg);
    const size_t w0 = (size_t)reg * a.stride;
    uint32_t total = 0;
    for (uint32_t c = 0; c < g.npts; c += 256) {              // workgroup-uniform trip count
        const uint32_t i = c + threadIdx.x;
        const bool keep = i < g.npts && a.label[w0 + i] == i && a.csize[w0 + i] >= a.min_points;
        const uint32_t pos = rank.step(keep, total);
        if (keep && pos < (uint32_t)a.max_rows) a.row_root[(size_t)reg * a.max_rows + pos] = i;
    }
    if (threadIdx.x == 0) {
        if (total == 0 && a.n_sel[reg] > 0) { total = 1; a.row_root[(size_t)reg * a.max_rows] = CVFH_NONE; }   // the fallback row
        a.n_clusters[reg] = total;
    }
}

// ---- one row ------------------------------------------------------------------------------------------------------------------------------------------
struct CvfhRowSmem {
    double red_d[4];
    unsigned long long red_k[4];
    uint32_t red_u[4];
    float red_f[4];
    uint32_t cnt[4 * VFH_COPIES * ISMHIP_VFH_DIM];
};
__global__ __launch_bounds__(256) void k_cvfh_rows(CvfhArgs a) {
    __shared__ CvfhRowSmem sm;
    constexpr int D = ISMHIP_VFH_DIM;
    const int tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const uint32_t reg = blockIdx.x / (uint32_t)a.max_rows, k = blockIdx.x % (uint32_t)a.max_rows;
    const size_t slot = (size_t)reg * a.max_rows + k;
    const float qnan = __builtin_nanf("");
    float* row = a.desc + slot * D;
    uint32_t* crow = a.counts ? a.counts + slot * D : nullptr;
    auto nan_row = [&]() { for (int i = tid; i < D; i += 256) { row[i] = qnan; if (crow) crow[i] = 0u; } };
    const uint32_t ncl = a.n_clusters[reg];
    if (k >= ncl) {                                           // workgroup-uniform: a slot without a row
        if (tid < 3) { a.row_centroid[slot * 3 + tid] = qnan; a.row_normal[slot * 3 + tid] = qnan; }
        if (tid == 0) a.row_size[slot] = 0u;
        nan_row();
        return;
    }
    const CvfhRegion g = cvfh_region(a, reg);
    const size_t w0 = (size_t)reg * a.stride;
    const float4* sp = a.sp4 + g.base;
    const float4* sn = a.sn4 + g.base;
    const float4* wn = a.wn4 + w0;
    const uint32_t root = a.row_root[slot];
    const uint32_t* label = a.label + w0;

    // ---- centroid and normal of the cluster (the fallback row: of every selected point): integer grids, order free ----------------------------
    // coordinates: |p| <= |c| + R per axis for a selected point, c and R the region's; normals: components below 4
    const float rc0 = a.centroid[reg * 3], rc1 = a.centroid[reg * 3 + 1], rc2 = a.centroid[reg * 3 + 2], rR = a.radius[reg];
    const int bits = grid_bits(g.m.n_finite);
    const int ep = exp_above((double)fmaxf(fabsf(rc0), fmaxf(fabsf(rc1), fabsf(rc2))) + (double)rR) + 1;
    const double magic_p = ldexp(1.5, ep - bits + 52), q_p = ldexp(1.0, ep - bits);
    const double magic_n = ldexp(1.5, 2 - bits + 52), q_n = ldexp(1.0, 2 - bits);
    long long spx = 0, spy = 0, spz = 0, snx = 0, sny = 0, snz = 0;
    uint32_t members = 0, nfin = 0;
    for (uint32_t i = tid; i < g.n; i += 256) {
        const float4 p = sp[i];
        const uint32_t orig = __float_as_uint(p.w);
        const bool mem = root == CVFH_NONE ? g.selected(p) : (orig < g.npts && label[orig] == root);
        if (!mem) continue;
        members++;
        spx += on_grid((double)p.x, magic_p); spy += on_grid((double)p.y, magic_p); spz += on_grid((double)p.z, magic_p);
        const float4 nr = wn[i];
        if (finite3(nr) && fabsf(nr.x) < 4.f && fabsf(nr.y) < 4.f && fabsf(nr.z) < 4.f) {
            nfin++;
            snx += on_grid((double)nr.x, magic_n); sny += on_grid((double)nr.y, magic_n); snz += on_grid((double)nr.z, magic_n);
        }
    }
    members = block_sum_i(members, sm.red_u); nfin = block_sum_i(nfin, sm.red_u);
    // two's complement: the unsigned sum is the signed one
    spx = (long long)block_sum_u64((unsigned long long)spx, sm.red_k); spy = (long long)block_sum_u64((unsigned long long)spy, sm.red_k);
    spz = (long long)block_sum_u64((unsigned long long)spz, sm.red_k); snx = (long long)block_sum_u64((unsigned long long)snx, sm.red_k);
    sny = (long long)block_sum_u64((unsigned long long)sny, sm.red_k); snz = (long long)block_sum_u64((unsigned long long)snz, sm.red_k);
    const float cx = (float)(((double)spx * q_p) / (double)members), cy = (float)(((double)spy * q_p) / (double)members),
                cz = (float)(((double)spz * q_p) / (double)members);
    const double mnx = ((double)snx * q_n) / (double)nfin, mny = ((double)sny * q_n) / (double)nfin, mnz = ((double)snz * q_n) / (double)nfin;
    const double len = sqrt((mnx * mnx + mny * mny) + mnz * mnz);            // nfin = 0 or a zero mean: NaN
    const float ncx = (float)(mnx / len), ncy = (float)(mny / len), ncz = (float)(mnz / len);
    if (tid == 0) {
        a.row_centroid[slot * 3] = cx; a.row_centroid[slot * 3 + 1] = cy; a.row_centroid[slot * 3 + 2] = cz;
        a.row_normal[slot * 3] = ncx; a.row_normal[slot * 3 + 1] = ncy; a.row_normal[slot * 3 + 2] = ncz;
        a.row_size[slot] = members;
    }

    // ---- the largest distance and the number of depositing points: selected, finite CLOUD normal ------------------------------------------------
    float dmax = 0.f; uint32_t mt = 0;
    span_sweep<true>(sp, sn, g.n, tid, [&](const float4& p, const float4& nr) {
        if (!g.selected(p) || !finite3(nr)) return;
        const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        const float d = sqrtf((dx * dx + dy * dy) + dz * dz);                  // f4 of the deposit
        if (d > dmax) dmax = d;
        mt++;
    });
    dmax = block_max_f(dmax, sm.red_f);
    const uint32_t mfin = block_sum_i(mt, sm.red_u);
    if (mfin < 2u || !(isfinite(ncx) && isfinite(ncy) && isfinite(ncz)) || !(isfinite(cx) && isfinite(cy) && isfinite(cz))) { nan_row(); return; }   // workgroup-uniform

    float vdx, vdy, vdz;
    vfh_view_direction(a.vpx, a.vpy, a.vpz, cx, cy, cz, vdx, vdy, vdz);

    // ---- the histogram: k_vfh's, per-wave copies of integer bins -------------------------------------------------------------------------------------
    for (int i = tid; i < 4 * VFH_COPIES * D; i += 256) sm.cnt[i] = 0u;
    __syncthreads();
    uint32_t* hist = sm.cnt + (wv * VFH_COPIES + (lane % VFH_COPIES)) * D;
    const double ddmax = (double)dmax;
    span_sweep<true>(sp, sn, g.n, tid, [&](const float4& p, const float4& nr) {
        if (!g.selected(p)) return;
        // b4: the distance as a fraction of the largest one (a zero dmax: 0 / 0, no deposit)
        vfh_deposit(hist, cx, cy, cz, ncx, ncy, ncz, vdx, vdy, vdz, p, nr,
                    [ddmax](float f4) { return vfh_bin(((double)VFH_SHAPE_BINS * (double)f4) / ddmax, VFH_SHAPE_BINS - 1); });
    });
    __syncthreads();
    for (int b = tid; b < D; b += 256) {
        uint32_t c = 0;
        for (int j = 0; j < 4 * VFH_COPIES; ++j) c += sm.cnt[j * D + b];
        if (crow) crow[b] = c;
        row[b] = (float)c / CVFH_NORM;
    }
}

}  // namespace

extern "C" int ismhip_global_cvfh(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                                  const float* region_radius, const float viewpoint[3], float cluster_tolerance, float normal_radius, int min_points,
                                  double angle_threshold, int max_rows, uint32_t* n_sel_out, float* centroid_out, float* radius_out,
                                  uint32_t* n_clusters_out, float* row_centroid_out, float* row_normal_out, uint32_t* row_size_out, float* desc_out,
                                  uint32_t* count_out, uint32_t* label_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    const bool arrays = region_obj && region_center && region_radius && n_sel_out && centroid_out && radius_out && n_clusters_out && row_centroid_out &&
                        row_normal_out && row_size_out && desc_out;
    if (!cloud || n_regions < 0 || (n_regions > 0 && !arrays)) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_cvfh: bad argument");
    if (!viewpoint || !(std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2])))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_cvfh: the viewpoint is not finite");
    if (!(cluster_tolerance > 0.f) || !std::isfinite(cluster_tolerance) || !std::isfinite(normal_radius) || min_points < 1 || max_rows < 1 ||
        !(angle_threshold > 0.0 && angle_threshold < M_PI))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "global_cvfh: cluster tolerance, minimum size, row capacity or angle out of range");
    if (n_regions == 0) return ISMHIP_OK;
    const uint32_t stride = cloud->max_pts > 0 ? cloud->max_pts : 1u;
    const size_t cells = (size_t)n_regions * stride;
    const uint32_t nbx = (stride + 255) / 256;
    if ((unsigned long long)nbx * (unsigned long long)n_regions > 0x7fffffffull || (unsigned long long)max_rows * (unsigned long long)n_regions > 0x7fffffffull)
        return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "global_cvfh: more than 2^31 workgroups in one call");
    // one slab: normals (16 B), parent, size, label (4 B each) per (region, point), then the row roots
    const size_t bytes = cells * (16 + 4 + 4 + (label_out ? 0 : 4)) + (size_t)n_regions * max_rows * 4;
    char* ws = (char*)ism_scratch(ctx, SCR_CVFH, bytes);
    if (!ws) return ISMHIP_ERR_NOMEM;
    CvfhArgs a{};
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.cell_start = cloud->cell_start; a.sp4 = cloud->sp4; a.sn4 = cloud->sn4; a.n_obj = cloud->n_obj;
    a.stride = stride; a.nbx = nbx;
    a.reg_obj = region_obj; a.reg_center = region_center; a.reg_radius = region_radius;
    a.vpx = viewpoint[0]; a.vpy = viewpoint[1]; a.vpz = viewpoint[2];
    a.tol = cluster_tolerance; a.tol2 = (float)((double)cluster_tolerance * (double)cluster_tolerance);
    a.nrad = normal_radius; a.nrad2 = (float)((double)normal_radius * (double)normal_radius);
    a.min_points = (uint32_t)min_points; a.cos_thr = cos(angle_threshold); a.max_rows = max_rows;
    a.wn4 = (float4*)ws; ws += cells * 16;
    a.parent = (uint32_t*)ws; ws += cells * 4;
    a.csize = (uint32_t*)ws; ws += cells * 4;
    if (label_out) a.label = label_out; else { a.label = (uint32_t*)ws; ws += cells * 4; }
    a.row_root = (uint32_t*)ws;
    a.n_sel = n_sel_out; a.centroid = centroid_out; a.radius = radius_out; a.n_clusters = n_clusters_out;
    a.row_centroid = row_centroid_out; a.row_normal = row_normal_out; a.row_size = row_size_out; a.desc = desc_out; a.counts = count_out;
    TimerScope ts(ctx, "global_cvfh");
    const dim3 dense(nbx * (unsigned)n_regions), per_region((unsigned)n_regions);
    {
        TimerScope t1(ctx, "cvfh_normals");
        hipLaunchKernelGGL(k_cvfh_region, per_region, dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_cvfh_region");
        hipLaunchKernelGGL(k_cvfh_init, dense, dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_cvfh_init");
        hipLaunchKernelGGL(k_cvfh_normals, dense, dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_cvfh_normals");
    }
    {
        TimerScope t2(ctx, "cvfh_label");
        hipLaunchKernelGGL(k_cvfh_link, dense, dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_cvfh_link");
        hipLaunchKernelGGL(k_cvfh_flatten, dense, dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_cvfh_flatten");
    }
    {
        TimerScope t3(ctx, "cvfh_stats");
        hipLaunchKernelGGL(k_cvfh_select, per_region, dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_cvfh_select");
    }
    {
        TimerScope t4(ctx, "cvfh_rows");
        hipLaunchKernelGGL(k_cvfh_rows, dim3((unsigned)n_regions * (unsigned)max_rows), dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_cvfh_rows");
    }
    return ISMHIP_OK;
}

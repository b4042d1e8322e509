// mvbb.hip — the minimum-volume bounding box of a region (BoundingBoxType "MVBB"): Utils::computeMVBB (utils/utils.cpp:242-293), which
// is gdiam_approx_mvbb(points, n, 0.0) of the vendored libgdiam-1.3 and nothing else. One 256-thread workgroup per REGION, the region
// rule of global.hip. The arithmetic is this library's own statement of that algorithm, written out step by step in include/ismhip.h
// (steps A to D, the output convention, the degenerate inputs) and restated in float64 numpy by tests/mvbb_ref.py; DESIGN.md section
// 4.24 names the deviations. Everything is double and unfused (-ffp-contract=off), every reduction an order-free minimum or maximum
// of (value, index) keys or an integer sum: no float atomic, the same bits on every call.
//
// Per region:
//   0. the selected points, compacted in span order into the region's work buffer (a whole-object region reads the span itself)
//   A. the farthest pair: all pairs, tiled through LDS (four row points per thread in registers, 256 column points per tile, every lane
//      reads the same column point: an LDS broadcast); per-thread best (d2, (i, j)), then two key reductions
//   B. the same on the points projected across d1 (projected on the fly when a tile is staged)
//   C. bound in (d1, d2, d3) and in the identity axes: one sweep and six key reductions each (mvbb_bound, written once)
//   D. ten rounds: project with the orthonormal base of one axis of the best box (mvbb_base, written once) -> the extremes in eight
//      directions -> drop what lies inside their polygon by more than a rounding margin -> ordered compaction of the survivors (LDS
//      while they fit, else the work buffer) -> rank sort by (x, y, index) -> monotone chain on ONE thread -> one hull edge per
//      thread, each scanning the hull's vertices -> lift, bound, keep if strictly smaller
// Nothing is truncated: survivors and hull of any size go through the work buffer (all points on a circle: every point survives).
// Static LDS 53 KiB. Where the time goes (the FP64 pair search against the serial hull) is measured, not assumed: tools/mvbb_time.py.
#include "common.h"
#include <cmath>

namespace {

#define MVBB_LDS_PTS 768                  /* survivors staged in LDS; more go through the work buffer */
#define MVBB_MARGIN 9.094947017729282e-13 /* 2^-40: the pre-filter drops a point only if every cross product exceeds this x M^2 */
#define MVBB_ROWS 4                       /* row points per thread of the pair search */
#define MVBB_TAKE (1.0 - 0x1p-36)         /* a round's box is kept if its volume is below this x the best one's (ismhip.h, step D) */

typedef unsigned long long u64;

struct MvbbArgs {
    const uint32_t* pt_off; const GridMeta* meta; const float4* sp4;
    const float *x, *y, *z;                   // original order: the points of a pair by their index
    int n_obj;
    const int32_t* reg_obj; const float* reg_center; const float* reg_radius;
    uint32_t* n_sel; float* center; float* size; float* axes; double* volume; int32_t* trace;
    unsigned char* work; size_t work_stride; uint32_t cap; int reg0;
};

struct MvbbSmem {
    u64 red_k[4];
    uint32_t red_u[4];
    BlockRank<256> rank;
    double tile[3][256];
    uint32_t tile_idx[256];
    double2 pa[2 * MVBB_LDS_PTS], pb[MVBB_LDS_PTS];          // pa: the survivors, then the hull's stack: each chain pushes a point at most once
    uint32_t ia[2 * MVBB_LDS_PTS], ib[MVBB_LDS_PTS];
    uint32_t hull_n;
};

// doubles as keys whose unsigned order is the doubles' order (no NaN among them)
__device__ __forceinline__ u64 d2key(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key2d(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ double block_max_d(double v, u64* red) { return key2d(block_max_u64(d2key(v), red)); }
__device__ __forceinline__ double block_min_d(double v, u64* red) { return key2d(block_min_u64(d2key(v), red)); }

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void normalize3(double* v) {
    const double len = sqrt(dot3(v, v));
    if (len == 0.0) return;
    v[0] /= len; v[1] /= len; v[2] /= len;
}
__device__ __forceinline__ void set_norm3(double* o, double x, double y, double z) { o[0] = x; o[1] = y; o[2] = z; normalize3(o); }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = -(a[0] * b[2] - a[2] * b[0]);
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// gdiam_generate_orthonormal_base (gdiam.cpp:1226-1270), its case list as written: in is normalised in place
__device__ __forceinline__ void mvbb_base(double* in, double* o1, double* o2) {
    normalize3(in);
    if (in[0] == 0.0) {
        if (in[1] == 0.0) { set_norm3(o1, 1, 0, 0); set_norm3(o2, 0, 1, 0); return; }
        if (in[2] == 0.0) { set_norm3(o1, 1, 0, 0); set_norm3(o2, 0, 0, 1); return; }
        set_norm3(o1, 0, -in[2], in[1]); set_norm3(o2, 1, 0, 0); return;
    }
    if (in[1] == 0.0 && in[2] == 0.0) { set_norm3(o1, 0, 1, 0); set_norm3(o2, 0, 0, 1); return; }
    if (in[1] == 0.0) { set_norm3(o1, -in[2], 0, in[0]); set_norm3(o2, 0, 1, 0); return; }
    if (in[2] == 0.0) { set_norm3(o1, -in[1], in[0], 0); set_norm3(o2, 0, 0, 1); return; }
    set_norm3(o1, -in[1], in[0], 0);
    cross3(in, o1, o2);
    normalize3(o2);
}

struct MvbbBox { double ax[9], lo[3], hi[3], vol; };

// the bounding step: lo / hi of the points' products with the three rows of b.ax, and the volume (e0 * e1) * e2
__device__ __forceinline__ void mvbb_bound(const float4* __restrict__ pts, uint32_t m, MvbbBox& b, MvbbSmem& sm) {
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (uint32_t i = threadIdx.x; i < m; i += 256) {
        const float4 p = pts[i];
        const double q[3] = {(double)p.x, (double)p.y, (double)p.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double s = dot3(q, b.ax + 3 * k);
            if (s < lo[k]) lo[k] = s;
            if (s > hi[k]) hi[k] = s;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { b.lo[k] = block_min_d(lo[k], sm.red_k); b.hi[k] = block_max_d(hi[k], sm.red_k); }
    b.vol = ((b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1])) * (b.hi[2] - b.lo[2]);
}

// The pair (i, j), i < j by original index, of largest squared distance between the points xf maps the records to; ties go to the
// lowest (i, j). m < 2: key = ~0.
template <class XF>
__device__ __forceinline__ u64 mvbb_pair(const float4* __restrict__ pts, uint32_t m, MvbbSmem& sm, XF&& xf) {
    const int tid = threadIdx.x;
    double bd = -1.0;
    u64 bk = ~0ull;
    // MVBB_ROWS row points per thread at a time (rows r0 + 256 j + tid): one LDS read of a column point serves that many pairs, and
    // their distance chains are independent. Maximum and index tie-break do not depend on the order in which the pairs are met.
    for (uint32_t r0 = 0; r0 < m; r0 += 256 * MVBB_ROWS) {
        double rx[MVBB_ROWS], ry[MVBB_ROWS], rz[MVBB_ROWS];
        uint32_t ri[MVBB_ROWS];
#pragma unroll
        for (int j = 0; j < MVBB_ROWS; ++j) {
            const uint32_t r = r0 + 256u * j + tid;
            rx[j] = ry[j] = rz[j] = 0.0; ri[j] = 0u;
            if (r < m) { const float4 p = pts[r]; xf(p, rx[j], ry[j], rz[j]); ri[j] = __float_as_uint(p.w); }
        }
        auto pair = [&](int j, int k) {
            const double dx = rx[j] - sm.tile[0][k], dy = ry[j] - sm.tile[1][k], dz = rz[j] - sm.tile[2][k];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 >= bd) {
                const uint32_t ci = sm.tile_idx[k];
                const u64 key = ri[j] < ci ? ((u64)ri[j] << 32) | ci : ((u64)ci << 32) | ri[j];
                if (d2 > bd || key < bk) { bd = d2; bk = key; }
            }
        };
        for (uint32_t c0 = r0; c0 < m; c0 += 256) {
            __syncthreads();                                   // the previous tile has been read
            const uint32_t c = c0 + tid;
            if (c < m) {
                const float4 p = pts[c];
                double cx, cy, cz;
                xf(p, cx, cy, cz);
                sm.tile[0][tid] = cx; sm.tile[1][tid] = cy; sm.tile[2][tid] = cz;
                sm.tile_idx[tid] = __float_as_uint(p.w);
            }
            __syncthreads();
            const int cn = (int)min(256u, m - c0);
            if (c0 < r0 + 256u * MVBB_ROWS) {                  // a tile among the rows themselves: only the pairs with column > row, rows < m
                for (int k = 0; k < cn; ++k) {
#pragma unroll
                    for (int j = 0; j < MVBB_ROWS; ++j) {
                        const uint32_t r = r0 + 256u * j + tid;
                        if (r < m && c0 + (uint32_t)k > r) pair(j, k);
                    }
                }
            } else {                                           // beyond them: every row of the chunk exists (c0 < m lies behind it)
                for (int k = 0; k < cn; ++k) {
#pragma unroll
                    for (int j = 0; j < MVBB_ROWS; ++j) pair(j, k);
                }
            }
        }
    }
    const u64 top = block_max_u64(d2key(bd), sm.red_k);
    return block_min_u64(d2key(bd) == top ? bk : ~0ull, sm.red_k);
}

__global__ __launch_bounds__(256) void k_mvbb(MvbbArgs a) {
    __shared__ MvbbSmem sm;
    const int tid = threadIdx.x;
    const uint32_t reg = (uint32_t)a.reg0 + blockIdx.x;
    const float qnan = __builtin_nanf("");
    int32_t* tr = a.trace ? a.trace + (size_t)reg * ISMHIP_MVBB_TRACE : nullptr;
    if (tr && tid < ISMHIP_MVBB_TRACE) tr[tid] = (tid < 4 || (tid >= 8 && ((tid - 8) & 3) >= 2)) ? -1 : 0;   // indices -1, flags and sizes 0

    // ---- the region: as k_global -----------------------------------------------------------------------------------------------------
    const int o = a.reg_obj[reg];
    const bool obj_ok = o >= 0 && o < a.n_obj;
    uint32_t base = 0, n = 0;
    if (obj_ok) {
        base = a.pt_off[o];
        const uint32_t npts = a.pt_off[o + 1] - base, nf = a.meta[o].n_finite;
        n = nf < npts ? nf : npts;                            // the sorted span holds the finite points first
    }
    const float qx = a.reg_center[reg * 3], qy = a.reg_center[reg * 3 + 1], qz = a.reg_center[reg * 3 + 2];
    const float rs = a.reg_radius[reg];
    const bool whole = rs < 0.f;
    const float r2s = (float)((double)rs * (double)rs);
    const float4* sp = a.sp4 + base;

    // ---- the work buffer of this workgroup: selected points, two lists of (x, y) with their point index ----------------------------
    unsigned char* w = a.work + (size_t)blockIdx.x * a.work_stride;
    float4* sel = (float4*)w;
    double2* ga = (double2*)(w + (size_t)a.cap * 16);
    double2* gb = ga + 2 * (size_t)a.cap;
    uint32_t* gia = (uint32_t*)(gb + a.cap);
    uint32_t* gib = gia + 2 * (size_t)a.cap;

    // ---- 0. the selected points, in span order -----------------------------------------------------------------------------------------
    uint32_t m = 0;
    const float4* pts = sp;
    if (whole) m = n;
    else {
        for (uint32_t i0 = 0; i0 < n; i0 += 256) {
            const uint32_t i = i0 + tid;
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            bool f = false;
            if (i < n) { p = sp[i]; f = sqdist3(p.x, p.y, p.z, qx, qy, qz) < r2s; }
            const uint32_t pos = sm.rank.step(f, m);
            if (f) sel[pos] = p;
        }
        __syncthreads();
        pts = sel;
    }
    if (tid == 0) a.n_sel[reg] = m;
    if (m == 0) {                                             // workgroup-uniform
        if (tid < 3) { a.center[reg * 3 + tid] = qnan; a.size[reg * 3 + tid] = 0.f; }
        if (tid < 9) a.axes[(size_t)reg * 9 + tid] = qnan;
        if (tid == 0 && a.volume) a.volume[reg] = 0.0;
        return;
    }
    auto point_of = [&](uint32_t idx, double* q) { q[0] = (double)a.x[base + idx]; q[1] = (double)a.y[base + idx]; q[2] = (double)a.z[base + idx]; };

    MvbbBox best;
    for (int k = 0; k < 9; ++k) best.ax[k] = (k % 4 == 0) ? 1.0 : 0.0;
    bool degenerate = m < 2;

    // ---- A. the farthest pair ------------------------------------------------------------------------------------------------------------
    double d1[3] = {0, 0, 0};
    if (!degenerate) {
        const u64 pa = mvbb_pair(pts, m, sm, [](const float4& p, double& x, double& y, double& z) { x = (double)p.x; y = (double)p.y; z = (double)p.z; });
        double pi[3], pj[3];
        point_of((uint32_t)(pa >> 32), pi); point_of((uint32_t)pa, pj);
        for (int k = 0; k < 3; ++k) d1[k] = pi[k] - pj[k];
        if (dot3(d1, d1) == 0.0) degenerate = true;            // every point coincides with the first
        else {
            normalize3(d1);
            if (tr && tid == 0) { tr[0] = (int32_t)(pa >> 32); tr[1] = (int32_t)(uint32_t)pa; }
        }
    }
    if (degenerate) {                                         // identity axes, zero size, the point
        mvbb_bound(pts, m, best, sm);
        if (tid == 0) {                                       // constant indices: the box stays in registers
            for (int k = 0; k < 3; ++k) { a.center[reg * 3 + k] = (float)((best.lo[k] + best.hi[k]) * 0.5); a.size[reg * 3 + k] = 0.f; }
            for (int k = 0; k < 9; ++k) a.axes[(size_t)reg * 9 + k] = (float)best.ax[k];
            if (a.volume) a.volume[reg] = 0.0;
        }
        if (tr && tid == 0) tr[6] = 1;
        return;
    }

    // ---- B. the farthest pair across d1 ---------------------------------------------------------------------------------------------------
    {
        auto project = [&](const double* q, double* out) {
            const double t = dot3(q, d1);
            out[0] = q[0] - t * d1[0]; out[1] = q[1] - t * d1[1]; out[2] = q[2] - t * d1[2];
        };
        const u64 pb = mvbb_pair(pts, m, sm, [&](const float4& p, double& x, double& y, double& z) {
            const double q[3] = {(double)p.x, (double)p.y, (double)p.z};
            double r[3];
            project(q, r);
            x = r[0]; y = r[1]; z = r[2];
        });
        double pi[3], pj[3], ri[3], rj[3], v[3], d2[3], d3[3];
        point_of((uint32_t)(pb >> 32), pi); point_of((uint32_t)pb, pj);
        project(pi, ri); project(pj, rj);
        for (int k = 0; k < 3; ++k) v[k] = ri[k] - rj[k];
        const double prd = dot3(v, d1);
        for (int k = 0; k < 3; ++k) d2[k] = v[k] - prd * d1[k];
        const double len = sqrt(dot3(d2, d2));
        const bool collinear = len < 1e-6;
        if (collinear) mvbb_base(d1, d2, d3);
        else {
            for (int k = 0; k < 3; ++k) d2[k] /= len;
            cross3(d1, d2, d3);
            normalize3(d3);
        }
        for (int k = 0; k < 3; ++k) { best.ax[k] = d1[k]; best.ax[3 + k] = d2[k]; best.ax[6 + k] = d3[k]; }
        if (tr && tid == 0) { tr[2] = (int32_t)(pb >> 32); tr[3] = (int32_t)(uint32_t)pb; tr[5] = collinear ? 1 : 0; }
    }

    // ---- C. bound; the axis-aligned box if it is strictly smaller ------------------------------------------------------------------------
    mvbb_bound(pts, m, best, sm);
    {
        MvbbBox aabb;
        for (int k = 0; k < 9; ++k) aabb.ax[k] = (k % 4 == 0) ? 1.0 : 0.0;
        mvbb_bound(pts, m, aabb, sm);
        const bool take = aabb.vol < best.vol;
        if (take) best = aabb;
        if (tr && tid == 0) tr[4] = take ? 1 : 0;
    }

    // ---- D. ten rounds -------------------------------------------------------------------------------------------------------------------
    uint32_t most = 0;                                        // the most points the pre-filter left in a round (trace [7])
    for (int round = 0; round < ISMHIP_MVBB_ROUNDS; ++round) {
        double u[3], bx[3], by[3];
        const int ai = round % 3;
        for (int k = 0; k < 3; ++k) u[k] = ai == 0 ? best.ax[k] : (ai == 1 ? best.ax[3 + k] : best.ax[6 + k]);
        mvbb_base(u, bx, by);
        auto proj2 = [&](const float4& p, double& x, double& y) {
            const double q[3] = {(double)p.x, (double)p.y, (double)p.z};
            x = dot3(q, bx); y = dot3(q, by);
        };
        // the extremes in eight directions, counter-clockwise from +x: any point that attains one will do (the lowest position here)
        double fv[8];
        uint32_t fp[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { fv[k] = -INFINITY; fp[k] = 0xffffffffu; }
        for (uint32_t i = tid; i < m; i += 256) {
            double x, y;
            proj2(pts[i], x, y);
            const double f[8] = {x, x + y, y, y - x, -x, -(x + y), -y, x - y};
#pragma unroll
            for (int k = 0; k < 8; ++k) if (f[k] > fv[k]) { fv[k] = f[k]; fp[k] = i; }
        }
        double vx[8], vy[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const u64 top = block_max_u64(d2key(fv[k]), sm.red_k);
            const uint32_t pos = (uint32_t)block_min_u64(d2key(fv[k]) == top ? (u64)fp[k] : ~0ull, sm.red_k);
            proj2(pts[pos < m ? pos : 0], vx[k], vy[k]);
        }
        const double ex0 = vx[0] - vx[4], ey0 = vy[2] - vy[6];
        const double M = ex0 > ey0 ? ex0 : ey0, margin = MVBB_MARGIN * (M * M);
        // survivors, in the order of the selected points
        uint32_t S = 0;
        for (uint32_t i0 = 0; i0 < m; i0 += 256) {
            const uint32_t i = i0 + tid;
            bool keep = false;
            double x = 0, y = 0;
            uint32_t idx = 0;
            if (i < m) {
                const float4 p = pts[i];
                proj2(p, x, y);
                idx = __float_as_uint(p.w);
                int edges = 0;
                bool inside = true;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int k1 = (k + 1) & 7;
                    if (vx[k] == vx[k1] && vy[k] == vy[k1]) continue;
                    ++edges;
                    const double cr = (vx[k1] - vx[k]) * (y - vy[k]) - (vy[k1] - vy[k]) * (x - vx[k]);
                    if (!(cr > margin)) inside = false;
                }
                keep = !(inside && edges > 0);
            }
            const uint32_t pos = sm.rank.step(keep, S);
            if (keep) {
                ga[pos] = make_double2(x, y); gia[pos] = idx;
                if (pos < MVBB_LDS_PTS) { sm.pa[pos] = make_double2(x, y); sm.ia[pos] = idx; }
            }
        }
        __syncthreads();
        most = S > most ? S : most;
        const bool in_lds = S <= MVBB_LDS_PTS;
        double2* PA = in_lds ? sm.pa : ga; double2* PB = in_lds ? sm.pb : gb;
        uint32_t* IA = in_lds ? sm.ia : gia; uint32_t* IB = in_lds ? sm.ib : gib;
        // rank sort by (x, y, index)
        for (uint32_t s = tid; s < S; s += 256) {
            const double2 me = PA[s];
            const uint32_t mi = IA[s];
            uint32_t rank = 0;
            for (uint32_t t = 0; t < S; ++t) {
                const double2 q = PA[t];
                rank += (q.x < me.x || (q.x == me.x && (q.y < me.y || (q.y == me.y && IA[t] < mi)))) ? 1u : 0u;
            }
            PB[rank] = me; IB[rank] = mi;
        }
        __syncthreads();
        // the hull's strict vertices, counter-clockwise from the lowest (x, y): monotone chain over the sorted list, a point that
        // repeats the (x, y) of the one before it skipped
        if (tid == 0) {
            auto fresh = [&](uint32_t i) { return i == 0 || PB[i].x != PB[i - 1].x || PB[i].y != PB[i - 1].y; };
            auto turn = [&](const double2& o, const double2& p, const double2& q) { return (p.x - o.x) * (q.y - o.y) - (p.y - o.y) * (q.x - o.x); };
            uint32_t k = 0, last = 0;
            for (uint32_t i = 0; i < S; ++i) {
                if (!fresh(i)) continue;
                const double2 q = PB[i];
                while (k >= 2 && turn(PA[k - 2], PA[k - 1], q) <= 0.0) --k;
                PA[k] = q; IA[k] = IB[i]; ++k;
                last = i;
            }
            if (k > 1) {
                const uint32_t t = k + 1;
                for (uint32_t i = last; i-- > 0;) {
                    if (!fresh(i)) continue;
                    const double2 q = PB[i];
                    while (k >= t && turn(PA[k - 2], PA[k - 1], q) <= 0.0) --k;
                    PA[k] = q; IA[k] = IB[i]; ++k;
                }
                --k;                                           // the last vertex repeats the first
            }
            sm.hull_n = k;
        }
        __syncthreads();
        const uint32_t H = sm.hull_n;
        // the edge of smallest enclosing rectangle, one edge per thread; ties go to the lowest point index of the start vertex
        auto edge_dir = [&](uint32_t e, double& ex, double& ey) {
            const double2 p = PA[e], q = PA[e + 1 < H ? e + 1 : 0];
            ex = q.x - p.x; ey = q.y - p.y;
            const double len = sqrt(ex * ex + ey * ey);
            ex /= len; ey /= len;
        };
        double ba = INFINITY;
        u64 bk = ~0ull;
        if (H > 1) {
            for (uint32_t e = tid; e < H; e += 256) {
                double ex, ey;
                edge_dir(e, ex, ey);
                double smin = INFINITY, smax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
                for (uint32_t h = 0; h < H; ++h) {
                    const double2 p = PA[h];
                    const double s = p.x * ex + p.y * ey, t = p.y * ex - p.x * ey;
                    if (s < smin) smin = s;
                    if (s > smax) smax = s;
                    if (t < tmin) tmin = t;
                    if (t > tmax) tmax = t;
                }
                const double area = (smax - smin) * (tmax - tmin);
                const u64 key = ((u64)IA[e] << 32) | e;
                if (area < ba || (area == ba && key < bk)) { ba = area; bk = key; }
            }
        }
        const u64 low = block_min_u64(d2key(ba), sm.red_k);
        const u64 ek = block_min_u64(d2key(ba) == low ? bk : ~0ull, sm.red_k);
        double ex = 1.0, ey = 0.0;
        uint32_t e0 = 0, e1 = 0;
        if (H > 1) { e0 = (uint32_t)ek < H ? (uint32_t)ek : 0; e1 = e0 + 1 < H ? e0 + 1 : 0; edge_dir(e0, ex, ey); }
        const int32_t t0 = (int32_t)IA[e0], t1 = (int32_t)IA[e1];
        // lift the rectangle's sides, bound, keep if strictly smaller
        MvbbBox cand;
        for (int k = 0; k < 3; ++k) {
            cand.ax[k] = u[k];
            cand.ax[3 + k] = (-ey) * bx[k] + ex * by[k];        // across the edge first, then along it: the reference's order
            cand.ax[6 + k] = ex * bx[k] + ey * by[k];
        }
        normalize3(cand.ax + 3); normalize3(cand.ax + 6);
        mvbb_bound(pts, m, cand, sm);                          // its barriers also end this round's reads of the lists
        const bool take = cand.vol < best.vol * MVBB_TAKE;
        if (take) best = cand;
        if (tr && tid == 0) { int32_t* t = tr + 8 + 4 * round; t[0] = take ? 1 : 0; t[1] = (int32_t)H; t[2] = t0; t[3] = t1; }
    }

    if (tr && tid == 0) tr[7] = (int32_t)most;

    // ---- the output convention: descending extent, axes 1 and 2 signed by their largest component, axis 3 their cross product ----------
    if (tid == 0) {
        // a stable sort of three rows by conditional swaps, and the sign by the component itself: constant indices only, so the box
        // stays in registers
        double ax[9], lo[3], hi[3];
        for (int k = 0; k < 9; ++k) ax[k] = best.ax[k];
        for (int k = 0; k < 3; ++k) { lo[k] = best.lo[k]; hi[k] = best.hi[k]; }
        auto swap_if_longer = [&](int p, int q) {              // row q in front of row p if its extent is strictly larger
            if (hi[q] - lo[q] > hi[p] - lo[p]) {
                for (int k = 0; k < 3; ++k) { const double t = ax[3 * p + k]; ax[3 * p + k] = ax[3 * q + k]; ax[3 * q + k] = t; }
                double t = lo[p]; lo[p] = lo[q]; lo[q] = t;
                t = hi[p]; hi[p] = hi[q]; hi[q] = t;
            }
        };
        swap_if_longer(0, 1); swap_if_longer(1, 2); swap_if_longer(0, 1);
        auto flip = [&](int r) { for (int k = 0; k < 3; ++k) ax[3 * r + k] = -ax[3 * r + k]; const double t = lo[r]; lo[r] = -hi[r]; hi[r] = -t; };
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double big = ax[3 * r];
            if (fabs(ax[3 * r + 1]) > fabs(big)) big = ax[3 * r + 1];
            if (fabs(ax[3 * r + 2]) > fabs(big)) big = ax[3 * r + 2];
            if (big < 0.0) flip(r);
        }
        double a3[3];
        cross3(ax, ax + 3, a3);
        const bool neg = dot3(a3, ax + 6) < 0.0;
        for (int k = 0; k < 3; ++k) ax[6 + k] = a3[k];
        if (neg) { const double t = lo[2]; lo[2] = -hi[2]; hi[2] = -t; }
        const double mid[3] = {(lo[0] + hi[0]) * 0.5, (lo[1] + hi[1]) * 0.5, (lo[2] + hi[2]) * 0.5};
        for (int k = 0; k < 3; ++k) {
            a.center[reg * 3 + k] = (float)((mid[0] * ax[k] + mid[1] * ax[3 + k]) + mid[2] * ax[6 + k]);
            a.size[reg * 3 + k] = (float)(hi[k] - lo[k]);
        }
        for (int k = 0; k < 9; ++k) a.axes[(size_t)reg * 9 + k] = (float)ax[k];
        if (a.volume) a.volume[reg] = best.vol;
    }
}

}  // namespace

extern "C" int ismhip_region_mvbb(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                                  const float* region_radius, uint32_t* n_sel_out, float* center_out, float* size_out, float* axes9_out,
                                  double* volume_out, int32_t* trace_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    const bool arrays = region_obj && region_center && region_radius && n_sel_out && center_out && size_out && axes9_out;
    if (!cloud || n_regions < 0 || (n_regions > 0 && !arrays))                    // no region: nothing is read or written
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "region_mvbb: bad argument");
    if (n_regions == 0) return ISMHIP_OK;
    MvbbArgs a{};
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.sp4 = cloud->sp4; a.x = cloud->x; a.y = cloud->y; a.z = cloud->z; a.n_obj = cloud->n_obj;
    a.reg_obj = region_obj; a.reg_center = region_center; a.reg_radius = region_radius;
    a.n_sel = n_sel_out; a.center = center_out; a.size = size_out; a.axes = axes9_out; a.volume = volume_out; a.trace = trace_out;
    // per region: the selected points (16 B each), the survivors' (x, y) + index (20 B each) and the list they share with the hull's stack (40 B)
    a.cap = cloud->max_pts;
    a.work_stride = (((size_t)a.cap * 76 + 15) & ~(size_t)15) + 16;                 // never zero: a batch of empty objects
    size_t per_launch = (size_t)(((unsigned long long)ctx->mvbb_work_mb << 20) / a.work_stride);
    if (per_launch < 1) per_launch = 1;
    if (per_launch > (size_t)n_regions) per_launch = (size_t)n_regions;
    a.work = (unsigned char*)ism_scratch(ctx, SCR_MVBB, per_launch * a.work_stride);
    if (!a.work) return ISMHIP_ERR_NOMEM;
    TimerScope ts(ctx, "region_mvbb");
    for (int r0 = 0; r0 < n_regions; r0 += (int)per_launch) {                     // launches on one stream: the next one reuses the buffer in order
        a.reg0 = r0;
        const int nr = n_regions - r0 < (int)per_launch ? n_regions - r0 : (int)per_launch;
        hipLaunchKernelGGL(k_mvbb, dim3((unsigned)nr), dim3(256), 0, ctx->stream, a);
        ISM_CHECK_LAUNCH(ctx, "k_mvbb");
    }
    return ISMHIP_OK;
}

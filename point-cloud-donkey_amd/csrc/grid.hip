// grid.hip — search surface: per-object uniform grid + cell-sorted SoA copy of the cloud.
// Replaces the pcl::search::KdTree the reference builds per object (implicit_shape_model.cpp:823-831):
// an exact fixed-radius search over a grid is equivalent up to neighbour order.
//
// HBM layout: points of all objects are concatenated SoA (x|y|z|nx|ny|nz, 4-byte floats) as the caller hands them over. The
// sorted copy orders every object's points by cell id (x fastest, original index inside a cell) and packs them as 16-byte
// records (x,y,z,index | nx,ny,nz,0 | L,a,b,0), so the 2r-wide x-run of cells a query ball touches in one (y,z) row is ONE
// contiguous span read with one coalesced global_load_dwordx4 per candidate.
//
// The build is ONE kernel, one workgroup per object (k_grid_fused); batches with an object of more than GRID_FUSED_MAX_PTS points, and
// ISMHIP_GRID_FUSED=0, take the five kernels it replaced (k_bbox_meta, k_count, k_scan, k_members, k_scatter): same bytes either way.
#include "common.h"
#include <algorithm>
#include <cfloat>

namespace {

// GridMeta of one object from its finite-point count, coordinate sums and bounding box
__device__ __forceinline__ GridMeta make_grid_meta(uint32_t c, const double ss[3], float lo[3], float hi[3], float req_cell, float x_frac, int& ncell_out) {
    GridMeta m;
    if (c == 0) { for (int a = 0; a < 3; ++a) { lo[a] = 0.f; hi[a] = 0.f; } }
    // requested edge = the y/z edge; x cells are ISM_GRID_XFRAC times finer. An axis that would need more than
    // ISM_GRID_MAXDIM cells gets the smallest edge that fits.
    int ncell = 1;
    for (int a = 0; a < 3; ++a) {
        float cell = req_cell > 0.f ? req_cell : 1.f;
        if (a == 0) cell *= x_frac;
        if (!((hi[a] - lo[a]) / cell < (float)(ISM_GRID_MAXDIM - 1))) cell = fmaxf(cell, (hi[a] - lo[a]) / ((float)ISM_GRID_MAXDIM - 1.5f));
        m.cell[a] = cell; m.inv_cell[a] = 1.0f / cell;
        m.minv[a] = lo[a];
        int d = (int)floorf((hi[a] - lo[a]) * m.inv_cell[a]) + 1;
        d = d < 1 ? 1 : (d > ISM_GRID_MAXDIM ? ISM_GRID_MAXDIM : d);
        m.dim[a] = d; ncell *= d;
        m.centroid[a] = c ? (float)(ss[a] / (double)c) : 0.f;   // pcl::compute3DCentroid (double accumulate)
    }
    m.n_finite = c;
    ncell_out = ncell;
    return m;
}

__global__ __launch_bounds__(256) void k_bbox_meta(const uint32_t* __restrict__ pt_off,
                                                   const float* __restrict__ x, const float* __restrict__ y,
                                                   const float* __restrict__ z, float req_cell, float x_frac,
                                                   GridMeta* __restrict__ meta, uint32_t* __restrict__ cell_start) {
    const int o = blockIdx.x;
    const uint32_t b = pt_off[o], e = pt_off[o + 1];
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    double s[3] = {0, 0, 0};
    uint32_t cnt = 0;
    for (uint32_t i = b + threadIdx.x; i < e; i += blockDim.x) {
        const float px = x[i], py = y[i], pz = z[i];
        if (!(isfinite(px) && isfinite(py) && isfinite(pz))) continue;
        mn[0] = fminf(mn[0], px); mx[0] = fmaxf(mx[0], px);
        mn[1] = fminf(mn[1], py); mx[1] = fmaxf(mx[1], py);
        mn[2] = fminf(mn[2], pz); mx[2] = fmaxf(mx[2], pz);
        s[0] += px; s[1] += py; s[2] += pz; cnt++;
    }
    __shared__ float s_f[4];
    __shared__ double s_d[4];
    __shared__ uint32_t s_u[4];
    float lo[3], hi[3];
    double ss[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = block_min_f(mn[a], s_f); hi[a] = block_max_f(mx[a], s_f); ss[a] = block_sum_d_left(s[a], s_d); }
    const uint32_t c = block_sum_i(cnt, s_u);
    int ncell;
    const GridMeta m = make_grid_meta(c, ss, lo, hi, req_cell, x_frac, ncell);    // every thread: the same arithmetic on the same values
    if (threadIdx.x == 0) meta[o] = m;
    uint32_t* cs = cell_start + (size_t)o * ISM_GRID_STRIDE;
    for (int i = threadIdx.x; i <= ncell; i += blockDim.x) cs[i] = 0u;
}

// counts points per cell; remembers each point's cell and its arrival rank inside the cell
__global__ __launch_bounds__(256) void k_count(const uint32_t* __restrict__ pt_off, const float* __restrict__ x,
                                               const float* __restrict__ y, const float* __restrict__ z,
                                               const GridMeta* __restrict__ meta, uint32_t* __restrict__ cell_start,
                                               uint32_t* __restrict__ cell_of_pt, uint32_t* __restrict__ rank_of_pt) {
    const int o = blockIdx.y;
    const uint32_t b = pt_off[o], e = pt_off[o + 1];
    const uint32_t i = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e) return;
    const GridMeta m = meta[o];
    const float px = x[i], py = y[i], pz = z[i];
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) { cell_of_pt[i] = 0xffffffffu; return; }
    const int cx = cell_coord(px, m.minv[0], m.inv_cell[0], m.dim[0]);
    const int cy = cell_coord(py, m.minv[1], m.inv_cell[1], m.dim[1]);
    const int cz = cell_coord(pz, m.minv[2], m.inv_cell[2], m.dim[2]);
    const uint32_t c = (uint32_t)((cz * m.dim[1] + cy) * m.dim[0] + cx);
    cell_of_pt[i] = c;
    rank_of_pt[i] = atomicAdd(&cell_start[(size_t)o * ISM_GRID_STRIDE + c], 1u);
}

// exclusive scan of the per-cell counts of one object (<= 32768 cells), in place; entry [ncell] = total
__global__ __launch_bounds__(1024) void k_scan(const GridMeta* __restrict__ meta, uint32_t* __restrict__ cell_start) {
    const int o = blockIdx.x;
    const GridMeta m = meta[o];
    const int ncell = m.dim[0] * m.dim[1] * m.dim[2];
    uint32_t* cs = cell_start + (size_t)o * ISM_GRID_STRIDE;
    __shared__ BlockScan<1024> scan;
    scan.init();
    for (int base = 0; base < ncell; base += 1024) {
        const int i = base + threadIdx.x;
        const uint32_t start = scan.step(i < ncell ? cs[i] : 0u);
        if (i < ncell) cs[i] = start;
    }
    if (threadIdx.x == 0) cs[ncell] = scan.total();
}

// members[b + cell_start[c] + arrival rank] = object-local index: the points of every cell, grouped (arrival order)
__global__ __launch_bounds__(256) void k_members(const uint32_t* __restrict__ pt_off, const uint32_t* __restrict__ cell_start,
                                                 const uint32_t* __restrict__ cell_of_pt, const uint32_t* __restrict__ rank_of_pt,
                                                 uint32_t* __restrict__ members) {
    const int o = blockIdx.y;
    const uint32_t b = pt_off[o], e = pt_off[o + 1];
    const uint32_t i = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e) return;
    const uint32_t c = cell_of_pt[i];
    if (c == 0xffffffffu) return;
    members[b + cell_start[(size_t)o * ISM_GRID_STRIDE + c] + rank_of_pt[i]] = i - b;
}

// SingleObjectHelper::getModelRadius (single_object_mode_helper.cpp:15-27): max over the points of |p - centroid| (Eigen norm: sqrt of
// the float sum x^2 + y^2 + z^2); max is order-free, points with a non-finite coordinate never compare greater
__global__ __launch_bounds__(256) void k_cloud_radii(const uint32_t* __restrict__ pt_off, const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                     const float* __restrict__ centroid, float* __restrict__ radius) {
    __shared__ float s_m[4];
    const int o = blockIdx.x;
    const float cx = centroid[o * 3], cy = centroid[o * 3 + 1], cz = centroid[o * 3 + 2];
    float m = 0.f;
    for (uint32_t i = pt_off[o] + threadIdx.x; i < pt_off[o + 1]; i += 256) {
        const float dx = x[i] - cx, dy = y[i] - cy, dz = z[i] - cz;
        const float d = sqrtf(dx * dx + dy * dy + dz * dz);
        if (d > m) m = d;
    }
    m = block_max_f(m, s_m);
    if (threadIdx.x == 0) radius[o] = m;
}

__device__ __forceinline__ float4 rgba_to_lab4(uint32_t c4, const float* __restrict__ lut_srgb, const float* __restrict__ lut_sxyz) {
    // RGB2CIELAB, reference: features/features_short_cshot.cpp:651-687 (PCL cshot.hpp); normalised L/100, a/120, b/120
    const float fr = lut_srgb[(c4 >> 16) & 0xff], fg = lut_srgb[(c4 >> 8) & 0xff], fb = lut_srgb[c4 & 0xff];
    const float X = fr * 0.412453f + fg * 0.357580f + fb * 0.180423f;
    const float Y = fr * 0.212671f + fg * 0.715160f + fb * 0.072169f;
    const float Z = fr * 0.019334f + fg * 0.119193f + fb * 0.950227f;
    float vx = X / 0.95047f, vy = Y, vz = Z / 1.08883f;
    int ix = (int)(vx * 4000), iy = (int)(vy * 4000), iz = (int)(vz * 4000);
    ix = ix < 0 ? 0 : (ix > 3999 ? 3999 : ix); iy = iy < 0 ? 0 : (iy > 3999 ? 3999 : iy); iz = iz < 0 ? 0 : (iz > 3999 ? 3999 : iz);
    vx = lut_sxyz[ix]; vy = lut_sxyz[iy]; vz = lut_sxyz[iz];
    float L = 116.0f * vy - 16.0f; if (L > 100) L = 100.0f;
    float A = 500.0f * (vx - vy); if (A > 120) A = 120.0f; else if (A < -120) A = -120.0f;
    float B = 200.0f * (vy - vz); if (B > 120) B = 120.0f; else if (B < -120) B = -120.0f;
    return make_float4(L / 100.0f, A / 120.0f, B / 120.0f, 0.f);
}

// Scatter into the cell-sorted packed arrays. The position of a point inside its cell is its rank BY ORIGINAL INDEX among the
// cell's members (a stable counting sort), not the atomic arrival rank of k_count: the sorted copy, and with it the order of
// every floating-point accumulation over a neighbourhood (LRF covariance, FPFH sums), is the same from run to run.
template <bool COLOR>
__global__ __launch_bounds__(256) void k_scatter(const uint32_t* __restrict__ pt_off,
                                                 const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                 const float* __restrict__ nx, const float* __restrict__ ny, const float* __restrict__ nz,
                                                 const uint32_t* __restrict__ rgba,
                                                 const float* __restrict__ lut_srgb, const float* __restrict__ lut_sxyz,
                                                 const uint32_t* __restrict__ cell_start, const uint32_t* __restrict__ cell_of_pt,
                                                 const uint32_t* __restrict__ members,
                                                 float4* __restrict__ sp4, float4* __restrict__ sn4, float4* __restrict__ slab4) {
    const int o = blockIdx.y;
    const uint32_t b = pt_off[o], e = pt_off[o + 1];
    const uint32_t i = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e) return;
    const uint32_t c = cell_of_pt[i];
    if (c == 0xffffffffu) return;
    const uint32_t* cs = cell_start + (size_t)o * ISM_GRID_STRIDE;
    const uint32_t m0 = cs[c], m1 = cs[c + 1], me = i - b;
    uint32_t rank = 0;
    for (uint32_t t = m0; t < m1; ++t) rank += members[b + t] < me;
    const uint32_t d = b + m0 + rank;
    sp4[d] = make_float4(x[i], y[i], z[i], __uint_as_float(me));
    sn4[d] = make_float4(nx[i], ny[i], nz[i], 0.f);
    if (COLOR) {
        slab4[d] = rgba_to_lab4(rgba[i], lut_srgb, lut_sxyz);
    }
}

// ---- the whole grid build of one object in ONE workgroup -------------------------------------------------------------------
// Same results as k_bbox_meta + k_count + k_scan + k_members + k_scatter, bit for bit (GridMeta, cell_start, and the sorted copy in
// the order (cell id, original index)), with the object's cell table held in LDS: one launch instead of five, no global atomic per
// point, no cell / arrival-rank / member arrays written and read back, and no serial walk over a cell's members in global memory.
//   1. bounding box + centroid. The coordinate sums are FP64 and feed the centroid, so they are formed in k_bbox_meta's order: the
//      1024 threads stage 4096 points in LDS (the table's memory, not yet in use), then threads 0..255 play k_bbox_meta's 256
//      threads, each adding its points v, v + 256, v + 512, ... one after the other.
//   2. histogram of the cell ids (ds_add_u32), 3. exclusive scan in LDS, cell_start written once.
//   4. stable rank without a sort: the points are taken in index order, 1024 at a time. Inside a wave a point's rank among the lanes
//      of the same cell comes from one ballot per bit of the cell id (a fixed ~13 rounds, however many points share a cell); the
//      waves of a chunk then read and advance the table's cursor of their cells one wave after the other.
// An object with more than GRID_FUSED_LDS_CELLS - 1 cells runs the same code on its cell_start row in global memory (LDS = false):
// the cursor pass then leaves every cell's END in the row, which a last pass shifts back into the starts.
#define GRID_FUSED_THREADS 1024
#define GRID_FUSED_LDS_CELLS 15360            // table entries in LDS (60 KB: two workgroups per CU); an object needs ncell + 1
#define GRID_FUSED_STAGE 4096                 // points staged per round of step 1 (3 floats each, inside the table's memory)
#define GRID_FUSED_MAX_PTS 65536u             // larger objects are not one workgroup's work: the batch takes the five-kernel path

template <bool LDS>
__device__ __forceinline__ void fused_sync() {
    if (!LDS) __threadfence();                // the table is in global memory: atomics and plain accesses meet in L2
    __syncthreads();
}

template <bool COLOR, bool LDS>
__device__ __forceinline__ void fused_sort(uint32_t* __restrict__ T, uint32_t* __restrict__ s_wave, uint32_t* __restrict__ cs, const GridMeta& m, int ncell,
                                           uint32_t b, uint32_t n,
                                           const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                           const float* __restrict__ nx, const float* __restrict__ ny, const float* __restrict__ nz,
                                           const uint32_t* __restrict__ rgba, const float* __restrict__ lut_srgb, const float* __restrict__ lut_sxyz,
                                           float4* __restrict__ sp4, float4* __restrict__ sn4, float4* __restrict__ slab4) {
    const uint32_t t = threadIdx.x;
    const int lane = lane_id(), wave = (int)(t >> 6);
    auto cell_of = [&](float px, float py, float pz) -> uint32_t {
        if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return 0xffffffffu;
        const int cx = cell_coord(px, m.minv[0], m.inv_cell[0], m.dim[0]);
        const int cy = cell_coord(py, m.minv[1], m.inv_cell[1], m.dim[1]);
        const int cz = cell_coord(pz, m.minv[2], m.inv_cell[2], m.dim[2]);
        return (uint32_t)((cz * m.dim[1] + cy) * m.dim[0] + cx);
    };
    // 2. histogram
    for (int i = (int)t; i <= ncell; i += GRID_FUSED_THREADS) T[i] = 0u;
    fused_sync<LDS>();
#pragma unroll 4
    for (uint32_t i = t; i < n; i += GRID_FUSED_THREADS) {
        const uint32_t c = cell_of(x[b + i], y[b + i], z[b + i]);
        if (c != 0xffffffffu) atomicAdd(&T[c], 1u);
    }
    fused_sync<LDS>();
    // 3. exclusive scan in place, T[ncell] = total; every thread owns K consecutive entries
    {
        const int K = (ncell + GRID_FUSED_THREADS - 1) / GRID_FUSED_THREADS, i0 = (int)t * K;
        uint32_t sum = 0;
        for (int k = 0; k < K; ++k) if (i0 + k < ncell) sum += T[i0 + k];
        const uint32_t incl = wave_incl_scan_u32(sum);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (int k = 0; k < wave; ++k) run += s_wave[k];
        for (int k = 0; k < K; ++k)
            if (i0 + k < ncell) { const uint32_t v = T[i0 + k]; T[i0 + k] = run; run += v; }
        if (t == GRID_FUSED_THREADS - 1) T[ncell] = run;
        fused_sync<LDS>();
        if (LDS) {
            for (int i = (int)t; i <= ncell; i += GRID_FUSED_THREADS) cs[i] = T[i];
            __syncthreads();                      // step 4 advances T: every start has been copied out before
        }
    }
    // 4. T[c] is now the cursor of cell c: the sorted position of the cell's next point
    const int nbits = ncell > 1 ? 32 - __clz(ncell - 1) : 0;         // bits of a cell id
    for (uint32_t c0 = 0; c0 < n; c0 += GRID_FUSED_THREADS) {
        const uint32_t i = c0 + t;
        float px = 0.f, py = 0.f, pz = 0.f;
        uint32_t c = 0xffffffffu;
        if (i < n) { px = x[b + i]; py = y[b + i]; pz = z[b + i]; c = cell_of(px, py, pz); }
        const bool valid = c != 0xffffffffu;
        // the lanes of the wave with the same cell, from one ballot per bit of the cell id -> rank among them, their number, the lowest
        unsigned long long same = __ballot(valid);
        for (int k = 0; k < nbits; ++k) {
            const bool bit = (c >> k) & 1u;
            const unsigned long long bk = __ballot(bit);
            same &= bit ? bk : ~bk;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull)), grp = (uint32_t)__popcll(same);
        const int lead = valid ? __ffsll((long long)same) - 1 : lane;
        // the waves of the chunk advance the cursors one after the other, in index order
        const int nw = (int)((min(n - c0, (uint32_t)GRID_FUSED_THREADS) + 63u) >> 6);
        uint32_t base = 0;
        for (int w = 0; w < nw; ++w) {
            if (wave == w) {
                if (LDS) {                    // one wave's LDS accesses are carried out in program order: every lane reads before the leaders write
                    if (valid) { base = T[c]; if (lane == lead) T[c] = base + grp; }
                } else {
                    uint32_t old = 0;
                    if (valid && lane == lead) old = atomicAdd(&T[c], grp);
                    base = (uint32_t)__shfl((int)old, lead, 64);
                }
            }
            fused_sync<LDS>();
        }
        if (valid) {
            const uint32_t d = b + base + rank;
            sp4[d] = make_float4(px, py, pz, __uint_as_float(i));
            sn4[d] = make_float4(nx[b + i], ny[b + i], nz[b + i], 0.f);
            if (COLOR) slab4[d] = rgba_to_lab4(rgba[b + i], lut_srgb, lut_sxyz);
        }
    }
    if (!LDS) {
        // T[c] holds the end of cell c = the start of cell c + 1: shift by one entry, from the top so that nothing is read after it is written
        for (int hi = ncell; hi > 0; hi -= GRID_FUSED_THREADS) {
            const int i = hi - (int)t;                        // entries hi, hi - 1, ..., hi - 1023
            const uint32_t v = i >= 1 ? T[i - 1] : 0u;
            fused_sync<LDS>();
            if (i >= 1) T[i] = v;
            fused_sync<LDS>();
        }
        if (t == 0) T[0] = 0u;
    }
}

template <bool COLOR>
__global__ __launch_bounds__(GRID_FUSED_THREADS) void k_grid_fused(const uint32_t* __restrict__ pt_off, int n_obj_map,
                                                                   const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                                   const float* __restrict__ nx, const float* __restrict__ ny, const float* __restrict__ nz,
                                                                   const uint32_t* __restrict__ rgba, const float* __restrict__ lut_srgb, const float* __restrict__ lut_sxyz,
                                                                   float req_cell, float x_frac, GridMeta* __restrict__ meta, uint32_t* __restrict__ cell_start,
                                                                   float4* __restrict__ sp4, float4* __restrict__ sn4, float4* __restrict__ slab4) {
    __shared__ uint32_t s_tab[GRID_FUSED_LDS_CELLS];
    __shared__ float s_mn[4][3], s_mx[4][3];
    __shared__ double s_s[4][3];
    __shared__ uint32_t s_c[4], s_wave[GRID_FUSED_THREADS / 64];
    __shared__ GridMeta s_meta;
    __shared__ int s_ncell;
    int o, bx;
    if (!xcd_object_block(1, n_obj_map, o, bx)) return;
    const uint32_t b = pt_off[o], n = pt_off[o + 1] - b, t = threadIdx.x;
    // 1. bounding box, count and coordinate sums of the finite points, in k_bbox_meta's order of additions
    float* st = reinterpret_cast<float*>(s_tab);              // x | y | z of the staged points
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    double s[3] = {0, 0, 0};
    uint32_t cnt = 0;
    for (uint32_t r0 = 0; r0 < n; r0 += GRID_FUSED_STAGE) {
        const uint32_t rn = min(n - r0, (uint32_t)GRID_FUSED_STAGE);
#pragma unroll
        for (uint32_t q = 0; q < GRID_FUSED_STAGE / GRID_FUSED_THREADS; ++q) {
            const uint32_t j = q * GRID_FUSED_THREADS + t;
            if (j < rn) { st[j] = x[b + r0 + j]; st[GRID_FUSED_STAGE + j] = y[b + r0 + j]; st[2 * GRID_FUSED_STAGE + j] = z[b + r0 + j]; }
        }
        __syncthreads();
        if (t < 256)
            for (uint32_t j = t; j < rn; j += 256) {
                const float px = st[j], py = st[GRID_FUSED_STAGE + j], pz = st[2 * GRID_FUSED_STAGE + j];
                if (!(isfinite(px) && isfinite(py) && isfinite(pz))) continue;
                mn[0] = fminf(mn[0], px); mx[0] = fmaxf(mx[0], px);
                mn[1] = fminf(mn[1], py); mx[1] = fmaxf(mx[1], py);
                mn[2] = fminf(mn[2], pz); mx[2] = fmaxf(mx[2], pz);
                s[0] += px; s[1] += py; s[2] += pz; cnt++;
            }
        __syncthreads();
    }
    // Not common.h's block reductions: only waves 0 .. 3 of the 16 hold partials. block_*<16> over identities gives the same bits, but
    // the sixteen slots of ten reductions, all used by thread 0 alone, cost the kernel its second workgroup per CU (127 VGPRs).
    if (t < 256) {                                            // whole waves: the DPP reductions need all 64 lanes
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = wave_min_f(mn[a]); mx[a] = wave_max_f(mx[a]); s[a] = wave_sum_d(s[a]); }
        cnt = (uint32_t)wave_sum_i((int)cnt);
        if (lane_id() == 0) {
            const int w = (int)(t >> 6);
            for (int a = 0; a < 3; ++a) { s_mn[w][a] = mn[a]; s_mx[w][a] = mx[a]; s_s[w][a] = s[a]; }
            s_c[w] = cnt;
        }
    }
    __syncthreads();
    if (t == 0) {
        int ncell;
        uint32_t c = 0; double ss[3] = {0, 0, 0};             // left fold, as block_sum_d_left (k_bbox_meta)
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int k = 0; k < 4; ++k) {
            c += s_c[k];
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], s_mn[k][a]); hi[a] = fmaxf(hi[a], s_mx[k][a]); ss[a] += s_s[k][a]; }
        }
        const GridMeta m = make_grid_meta(c, ss, lo, hi, req_cell, x_frac, ncell);
        meta[o] = m; s_meta = m; s_ncell = ncell;
    }
    __syncthreads();
    const GridMeta m = s_meta;
    const int ncell = s_ncell;
    uint32_t* cs = cell_start + (size_t)o * ISM_GRID_STRIDE;
    if (ncell + 1 <= GRID_FUSED_LDS_CELLS)
        fused_sort<COLOR, true>(s_tab, s_wave, cs, m, ncell, b, n, x, y, z, nx, ny, nz, rgba, lut_srgb, lut_sxyz, sp4, sn4, slab4);
    else
        fused_sort<COLOR, false>(cs, s_wave, cs, m, ncell, b, n, x, y, z, nx, ny, nz, rgba, lut_srgb, lut_sxyz, sp4, sn4, slab4);
}

// ---- keypoints in cell order ------------------------------------------------------------------------------------------------
// perm[kp_off[o] + r] = object-local index of the keypoint of rank r in the order (cell id, index). One workgroup per object ranks
// its <= KP_ORDER_MAX keypoints by counting, all against all, on 32-bit keys (cell id << 12 | index) held in LDS.
#define KP_ORDER_MAX 4096
__global__ __launch_bounds__(256) void k_kp_order(const GridMeta* __restrict__ meta, const uint32_t* __restrict__ kp_off,
                                                  const float* __restrict__ kx, const float* __restrict__ ky, const float* __restrict__ kz,
                                                  uint32_t* __restrict__ perm) {
    __shared__ uint32_t s_key[KP_ORDER_MAX];
    const int o = blockIdx.x;
    const uint32_t kb = kp_off[o], n = min(kp_off[o + 1] - kb, (uint32_t)KP_ORDER_MAX);
    const GridMeta m = meta[o];
    for (uint32_t j = threadIdx.x; j < n; j += 256) {
        const float px = kx[kb + j], py = ky[kb + j], pz = kz[kb + j];
        uint32_t c = ISM_GRID_MAXCELLS - 1;
        if (isfinite(px) && isfinite(py) && isfinite(pz))
            c = (uint32_t)((cell_coord(pz, m.minv[2], m.inv_cell[2], m.dim[2]) * m.dim[1] + cell_coord(py, m.minv[1], m.inv_cell[1], m.dim[1])) * m.dim[0] +
                           cell_coord(px, m.minv[0], m.inv_cell[0], m.dim[0]));
        s_key[j] = (c << 12) | j;
    }
    const uint32_t n4 = (n + 3u) & ~3u;
    for (uint32_t j = n + threadIdx.x; j < n4; j += 256) s_key[j] = 0xffffffffu;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < n; j += 256) {
        const uint32_t kj = s_key[j];
        uint32_t rank = 0;
        for (uint32_t i = 0; i < n4; i += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4*>(&s_key[i]);
            rank += (k4.x < kj) + (k4.y < kj) + (k4.z < kj) + (k4.w < kj);
        }
        perm[kb + rank] = j;
    }
}

__global__ void k_centroids(const GridMeta* __restrict__ meta, int n_obj, float* __restrict__ out) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_obj) return;
    out[o * 3 + 0] = meta[o].centroid[0]; out[o * 3 + 1] = meta[o].centroid[1]; out[o * 3 + 2] = meta[o].centroid[2];
}

__global__ __launch_bounds__(256) void k_center_dist(const GridMeta* __restrict__ meta, const uint32_t* __restrict__ kp_off,
                                                     const float* __restrict__ kx, const float* __restrict__ ky,
                                                     const float* __restrict__ kz, float* __restrict__ out) {
    const int o = blockIdx.y;
    const uint32_t k = kp_off[o] + blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= kp_off[o + 1]) return;
    const float dx = kx[k] - meta[o].centroid[0], dy = ky[k] - meta[o].centroid[1], dz = kz[k] - meta[o].centroid[2];
    out[k] = sqrtf(dx * dx + dy * dy + dz * dz);
}

}  // namespace

uint32_t* ism_upload_offsets(ismhip_ctx* ctx, int slot, const uint32_t* off_h, int n) {
    uint32_t* d = (uint32_t*)ism_scratch(ctx, slot, (size_t)n * sizeof(uint32_t));
    if (!d) return nullptr;
    if (hipMemcpyAsync(d, off_h, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        ism_set_err(ctx, ISMHIP_ERR_HIP, "offset upload failed");
        return nullptr;
    }
    return d;
}

int ism_ragged_offsets(ismhip_ctx* ctx, const std::string& name, const uint32_t* off_h, int n, int slot, int flags, RaggedOffsets* r) {
    *r = RaggedOffsets{};
    for (int i = 0; i < n; ++i) {
        if (off_h[i + 1] < off_h[i]) return ism_set_err(ctx, ISMHIP_ERR_INVALID, name + ": offsets not monotone");
        r->max_run = std::max(r->max_run, off_h[i + 1] - off_h[i]);
    }
    if ((flags & RAGGED_START0) && off_h[0] != 0) return ism_set_err(ctx, ISMHIP_ERR_INVALID, name + ": offsets must start at 0");
    r->total = off_h[n];
    if (r->max_run == 0 && !(flags & RAGGED_EMPTY)) return ISMHIP_OK;
    r->dev = ism_upload_offsets(ctx, slot, off_h, n + 1);
    return r->dev ? ISMHIP_OK : ISMHIP_ERR_HIP;
}

int ism_offsets_from_counts(ismhip_ctx* ctx, int n, const uint32_t* cnt_d, uint32_t* off_h_out, uint32_t* max_run_out) {
    std::vector<uint32_t> cnt_h(n);
    ISM_HIP(ctx, hipMemcpyAsync(cnt_h.data(), cnt_d, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t max_run = 0;
    off_h_out[0] = 0;
    for (int i = 0; i < n; ++i) { off_h_out[i + 1] = off_h_out[i] + cnt_h[i]; max_run = std::max(max_run, cnt_h[i]); }
    if (max_run_out) *max_run_out = max_run;
    return ISMHIP_OK;
}

// The cell-order permutation of a keypoint set on this cloud (device pointer), built on the ctx stream when the cloud does not hold it
// already; nullptr = take the keypoints as they come (switched off, or an object with more than KP_ORDER_MAX keypoints). ko = the
// offsets on the device. The cache is keyed by the coordinate pointer and the offsets: a stale order is still a permutation of the
// same keypoints, so the results never depend on it.
const uint32_t* ism_kp_order(ismhip_ctx* ctx, const ismhip_cloud* cloud_c, const uint32_t* kp_offsets_h, const uint32_t* ko,
                             const float* kpx, const float* kpy, const float* kpz, uint32_t maxk) {
    ismhip_cloud* c = const_cast<ismhip_cloud*>(cloud_c);
    if (!ctx->kp_order || maxk > KP_ORDER_MAX || maxk < 8) return nullptr;
    const int n_obj = c->n_obj;
    if (c->kp_perm_key == kpx && c->kp_perm_off.size() == (size_t)n_obj + 1 && std::equal(c->kp_perm_off.begin(), c->kp_perm_off.end(), kp_offsets_h))
        return c->kp_perm;
    const size_t nkp = kp_offsets_h[n_obj];
    if (c->kp_perm_cap < nkp) {
        if (c->kp_perm) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(c->kp_perm); c->kp_perm = nullptr; c->kp_perm_cap = 0; }
        c->kp_perm_key = nullptr;
        if (hipMalloc((void**)&c->kp_perm, (nkp + nkp / 8) * 4) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        c->kp_perm_cap = nkp + nkp / 8;
    }
    hipLaunchKernelGGL(k_kp_order, dim3(n_obj), dim3(256), 0, ctx->stream, c->meta, ko, kpx, kpy, kpz, c->kp_perm);
    c->kp_perm_key = kpx;
    c->kp_perm_off.assign(kp_offsets_h, kp_offsets_h + n_obj + 1);
    return c->kp_perm;
}

extern "C" {

int ismhip_cloud_create(ismhip_ctx* ctx, int n_obj, const uint32_t* pt_offsets_h,
                        const float* x, const float* y, const float* z,
                        const float* nx, const float* ny, const float* nz,
                        const uint32_t* rgba, float cell_size, ismhip_cloud** out) {
    if (!ctx || !out || n_obj <= 0 || !pt_offsets_h || !x || !y || !z || !nx || !ny || !nz || !(cell_size > 0.f))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "cloud_create: bad argument");
    *out = nullptr;
    for (int o = 0; o < n_obj; ++o)
        if (pt_offsets_h[o + 1] < pt_offsets_h[o]) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "cloud_create: offsets not monotone");
    if (pt_offsets_h[0] != 0) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "cloud_create: offsets must start at 0");
    ISM_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t n_pts_new = pt_offsets_h[n_obj];
    const size_t np = n_pts_new ? n_pts_new : 1;
    // recycle a destroyed cloud whose allocations are large enough (steady-state batches never touch hipMalloc)
    ismhip_cloud* c = nullptr;
    for (size_t i = 0; i < ctx->cloud_pool.size(); ++i) {
        ismhip_cloud* p = ctx->cloud_pool[i];
        if (p->cap_pts >= np && p->cap_obj >= n_obj && (p->cap_color || !rgba)) { c = p; ctx->cloud_pool.erase(ctx->cloud_pool.begin() + i); break; }
    }
    const bool fresh = c == nullptr;
    if (fresh) c = new ismhip_cloud();
    c->n_obj = n_obj;
    c->pt_off_h.assign(pt_offsets_h, pt_offsets_h + n_obj + 1);
    c->n_pts = n_pts_new;
    c->max_pts = 0;
    for (int o = 0; o < n_obj; ++o) c->max_pts = std::max(c->max_pts, pt_offsets_h[o + 1] - pt_offsets_h[o]);
    c->x = x; c->y = y; c->z = z; c->nx = nx; c->ny = ny; c->nz = nz; c->rgba = rgba;
    c->requested_cell = cell_size;
    c->kp_perm_key = nullptr;
    c->cospair_code_valid = false;
    auto fail = [&](int code, const char* msg) { c->cap_pts = 0; ismhip_cloud_destroy(ctx, c); return ism_set_err(ctx, code, msg); };
    if (fresh) {
        const size_t capp = np + np / 8;
        const int n_arr = rgba ? 3 : 2;
        float4* block = nullptr;
        if (hipMalloc((void**)&block, capp * sizeof(float4) * n_arr) != hipSuccess) return fail(ISMHIP_ERR_NOMEM, "cloud_create: hipMalloc sorted arrays");
        c->sp4 = block; c->sn4 = block + capp;
        if (rgba) c->slab4 = block + 2 * capp;
        if (hipMalloc((void**)&c->pt_off, (size_t)(n_obj + 1) * 4) != hipSuccess ||
            hipMalloc((void**)&c->meta, (size_t)n_obj * sizeof(GridMeta)) != hipSuccess ||
            hipMalloc((void**)&c->cell_start, (size_t)n_obj * ISM_GRID_STRIDE * 4) != hipSuccess)
            return fail(ISMHIP_ERR_NOMEM, "cloud_create: hipMalloc grid");
        c->cap_pts = capp; c->cap_obj = n_obj; c->cap_color = rgba != nullptr;
    }
    if (hipMemcpyAsync(c->pt_off, c->pt_off_h.data(), (size_t)(n_obj + 1) * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return fail(ISMHIP_ERR_HIP, "cloud_create: offsets copy");
    // one workgroup per object builds the whole grid (k_grid_fused) unless an object is too large for that to be sensible
    const bool fused = ctx->grid_fused && c->max_pts <= GRID_FUSED_MAX_PTS;
    if (!fused && !c->members) {   // scratch of the five-kernel path only
        if (hipMalloc((void**)&c->members, c->cap_pts * 4) != hipSuccess || hipMalloc((void**)&c->cell_of_pt, c->cap_pts * 4) != hipSuccess ||
            hipMalloc((void**)&c->rank_of_pt, c->cap_pts * 4) != hipSuccess)
            return fail(ISMHIP_ERR_NOMEM, "cloud_create: hipMalloc grid scratch");
    }
    {
        TimerScope ts(ctx, "grid");
        // non-finite points are dropped: an object's sorted span holds its n_finite points first, the tail is never read
        const float x_frac = ctx->grid_xfrac > 0.f ? 1.0f / ctx->grid_xfrac : 1.0f / (float)ISM_GRID_XFRAC;
        if (fused) {
            const dim3 gf(ctx->xcd_map ? xcd_object_grid(1, n_obj) : (unsigned)n_obj);
            const int n_obj_map = ctx->xcd_map ? n_obj : 0;
            if (rgba)
                hipLaunchKernelGGL(k_grid_fused<true>, gf, dim3(GRID_FUSED_THREADS), 0, ctx->stream, c->pt_off, n_obj_map, x, y, z, nx, ny, nz, rgba,
                                   ctx->lut_srgb, ctx->lut_sxyz, cell_size, x_frac, c->meta, c->cell_start, c->sp4, c->sn4, c->slab4);
            else
                hipLaunchKernelGGL(k_grid_fused<false>, gf, dim3(GRID_FUSED_THREADS), 0, ctx->stream, c->pt_off, n_obj_map, x, y, z, nx, ny, nz, rgba,
                                   ctx->lut_srgb, ctx->lut_sxyz, cell_size, x_frac, c->meta, c->cell_start, c->sp4, c->sn4, c->slab4);
        } else {
            hipLaunchKernelGGL(k_bbox_meta, dim3(n_obj), dim3(256), 0, ctx->stream, c->pt_off, x, y, z, cell_size, x_frac, c->meta, c->cell_start);
            const dim3 g((c->max_pts + 255) / 256 ? (c->max_pts + 255) / 256 : 1, n_obj);
            hipLaunchKernelGGL(k_count, g, dim3(256), 0, ctx->stream, c->pt_off, x, y, z, c->meta, c->cell_start, c->cell_of_pt, c->rank_of_pt);
            hipLaunchKernelGGL(k_scan, dim3(n_obj), dim3(1024), 0, ctx->stream, c->meta, c->cell_start);
            hipLaunchKernelGGL(k_members, g, dim3(256), 0, ctx->stream, c->pt_off, c->cell_start, c->cell_of_pt, c->rank_of_pt, c->members);
            if (rgba)
                hipLaunchKernelGGL(k_scatter<true>, g, dim3(256), 0, ctx->stream, c->pt_off, x, y, z, nx, ny, nz, rgba, ctx->lut_srgb, ctx->lut_sxyz,
                                   c->cell_start, c->cell_of_pt, c->members, c->sp4, c->sn4, c->slab4);
            else
                hipLaunchKernelGGL(k_scatter<false>, g, dim3(256), 0, ctx->stream, c->pt_off, x, y, z, nx, ny, nz, rgba, ctx->lut_srgb, ctx->lut_sxyz,
                                   c->cell_start, c->cell_of_pt, c->members, c->sp4, c->sn4, c->slab4);
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ISMHIP_ERR_HIP, hipGetErrorString(e));
    *out = c;
    return ISMHIP_OK;
}

static void cloud_free(ismhip_cloud* c) {
    if (c->sp4) (void)hipFree(c->sp4);
    if (c->kp_perm) (void)hipFree(c->kp_perm);
    if (c->cospair_code) (void)hipFree(c->cospair_code);
    if (c->members) (void)hipFree(c->members);
    if (c->cell_of_pt) (void)hipFree(c->cell_of_pt);
    if (c->rank_of_pt) (void)hipFree(c->rank_of_pt);
    if (c->pt_off) (void)hipFree(c->pt_off);
    if (c->meta) (void)hipFree(c->meta);
    if (c->cell_start) (void)hipFree(c->cell_start);
    delete c;
}

int ismhip_cloud_destroy(ismhip_ctx* ctx, ismhip_cloud* c) {
    if (!c) return ISMHIP_ERR_INVALID;
    // stream order protects the buffers: a recycled cloud is only rewritten by later work on the same stream
    if (ctx && c->cap_pts > 0 && ctx->cloud_pool.size() < 4) { ctx->cloud_pool.push_back(c); return ISMHIP_OK; }
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    cloud_free(c);
    return ISMHIP_OK;
}

void ism_cloud_pool_release(ismhip_ctx* ctx) {
    for (ismhip_cloud* c : ctx->cloud_pool) cloud_free(c);
    ctx->cloud_pool.clear();
}

int ismhip_cloud_centroids(ismhip_ctx* ctx, const ismhip_cloud* cloud, float* centroid_out) {
    if (!ctx || !cloud || !centroid_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "cloud_centroids: bad argument");
    hipLaunchKernelGGL(k_centroids, dim3((cloud->n_obj + 63) / 64), dim3(64), 0, ctx->stream, cloud->meta, cloud->n_obj, centroid_out);
    ISM_CHECK_LAUNCH(ctx, "k_centroids");
    return ISMHIP_OK;
}

int ismhip_cloud_radii(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* centroid, float* radius_out) {
    if (!ctx || !cloud || !centroid || !radius_out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "cloud_radii: bad argument");
    hipLaunchKernelGGL(k_cloud_radii, dim3(cloud->n_obj), dim3(256), 0, ctx->stream, cloud->pt_off, cloud->x, cloud->y, cloud->z, centroid, radius_out);
    ISM_CHECK_LAUNCH(ctx, "k_cloud_radii");
    return ISMHIP_OK;
}

int ismhip_center_dist(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                       const float* kpx, const float* kpy, const float* kpz, float* out) {
    if (!ctx || !cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !out) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "center_dist: bad argument");
    uint32_t* ko = ism_upload_offsets(ctx, SCR_KP_OFF, kp_offsets_h, cloud->n_obj + 1);
    if (!ko) return ISMHIP_ERR_HIP;
    uint32_t maxk = 0;
    for (int o = 0; o < cloud->n_obj; ++o) maxk = std::max(maxk, kp_offsets_h[o + 1] - kp_offsets_h[o]);
    if (maxk == 0) return ISMHIP_OK;
    hipLaunchKernelGGL(k_center_dist, dim3((maxk + 255) / 256, cloud->n_obj), dim3(256), 0, ctx->stream, cloud->meta, ko, kpx, kpy, kpz, out);
    ISM_CHECK_LAUNCH(ctx, "k_center_dist");
    return ISMHIP_OK;
}

}  // extern "C"

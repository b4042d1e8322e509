// shot_wave.h — what the kernels of the SHOT family (shot.hip: k_shot; short_shot.hip: k_short_shot; short_cshot.hip: k_short_cshot),
// CoSPAIR (cospair.hip: k_cospair, which has no frame) and SpinImage (spin_image.hip: k_spin_image, an axis in place of the frame) have
// in common: one 64-lane wavefront per keypoint that sets itself up
// from the keypoint, its frame and the object's grid, streams the points inside the query ball through an LDS queue to a per-neighbour function, and a launcher that checks the caller's arrays,
// uploads the keypoint offsets and starts a quarter as many workgroups as the longest keypoint run. The kernels differ in their
// per-neighbour function, their histogram and their normalisation only; those stay in their units.
#pragma once
#include "common.h"

// The per-wave LDS histograms are kept in 64-bit FIXED POINT (2^-28 units) and updated with ds_add_u64.
// Measured on gfx950 (tools/lds_atomic_bench.hip): ds_add_f32 costs ~195 CU-cycles per wave-instruction whatever the
// addresses, ds_add_u64 17-24, ds_add_u32 15 — with float atomics the kernel spent 64 % of its wave cycles in
// SQ_WAIT_INST_LDS. Every deposit is a non-negative interpolation weight < 8 (Short SHOT: a sum of shares in [0, 4]), so
// round(v * 2^28) fits 32 bits and a bin (<= 4 * 2^14 neighbours) needs 46 bits. Integer adds are associative: the histogram no
// longer depends on the order in which neighbours arrive (bitwise reproducible), and its error (<= 2^-29 per deposit) is far
// below the float accumulation error of the reference itself.
#define SHOT_FIX_SCALE 268435456.0f          /* 2^28 */
#define SHOT_FIX_INV   3.7252902984619140625e-09 /* 2^-28 */
typedef unsigned long long shot_bin_t;

#ifdef __HIPCC__
// What a wave knows once it is set up: its place, its keypoint k with row `row` of the output, the keypoint's centre and frame, the
// object's grid and the cell range of the query ball.
struct ShotWave {
    int o, wv, lane;
    uint32_t k;
    float* row;
    float cx, cy, cz, fx[3], fy[3], fz[3];
    GridMeta m;
    CellRange cr;
};

// The place of one wave, from any of the family's argument structs (the common fields carry the same names), for rows of D floats: the
// XCD block map, the keypoint of this wave in cell order, its row, its centre and the object's grid. False when the wave has no row to
// build: past the object's keypoint run (wave-uniform; no block-level barrier may follow).
template <class Args>
__device__ __forceinline__ bool shot_wave_place(const Args& a, int D, ShotWave& w) {
    int bx;
    if (!xcd_object_block(a.nbx, a.n_obj, w.o, bx)) return false;
    w.wv = threadIdx.x >> 6;
    w.lane = lane_id();
    if (a.kp_off[w.o] + bx * 4 + w.wv >= a.kp_off[w.o + 1]) return false;
    w.k = ordered_keypoint(a.kp_perm, a.kp_off[w.o], (uint32_t)(bx * 4 + w.wv));
    w.row = a.desc + (size_t)w.k * D;
    w.cx = a.kx[w.k]; w.cy = a.ky[w.k]; w.cz = a.kz[w.k];
    w.m = a.meta[w.o];
    return true;
}

// The cell range of the wave's ball, given `ok` = whatever else the descriptor needs to be finite. False -- THE rule that compact.hip's
// k_keep_rows relies on when it judges a row by its element 0 -- when ok fails, the centre is not finite or the ball misses the grid:
// the WHOLE row NaN, count 0.
template <class Args>
__device__ __forceinline__ bool shot_wave_ball(const Args& a, int D, ShotWave& w, bool ok) {
    ok = ok && isfinite(w.cx) && isfinite(w.cy) && isfinite(w.cz);
    if (!ok || !ball_cells(w.m, w.cx, w.cy, w.cz, a.radius, w.cr)) {
        for (int i = w.lane; i < D; i += 64) w.row[i] = __builtin_nanf("");
        if (a.count && w.lane == 0) a.count[w.k] = 0;
        return false;
    }
    return true;
}

// Set-up of one wave of a descriptor that reads a frame: its place, the frame, the ball. False as the two steps say.
template <class Args>
__device__ __forceinline__ bool shot_wave_setup(const Args& a, int D, ShotWave& w) {
    if (!shot_wave_place(a, D, w)) return false;
    const float* f = a.lrf + (size_t)w.k * 9;
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.fx[i] = f[i]; w.fy[i] = f[3 + i]; w.fz[i] = f[6 + i]; }
    return shot_wave_ball(a, D, w, isfinite(w.fx[0]) && isfinite(w.fy[0]) && isfinite(w.fz[0]));
}

// The neighbours of the wave's keypoint: streams the candidate x-runs of the query ball (coalesced loads of the cell-sorted sp4) in NG
// segments; lanes whose point is inside the ball are COMPACTED with a ballot + prefix popcount into a 128-entry circular LDS queue
// (qd: dx, dy, dz, d2; qi, with INDEX: the sorted point index -- without, qi is not touched and may be null); whenever 64 are queued,
// all 64 lanes run nb(true, gi, dx, dy, dz, d2) on a full wave (no divergence on the radius test), and the tail runs
// nb(act, gi, ...) once with act marking the lanes that hold a neighbour (gi = 0 on the others, and everywhere without INDEX).
// Correct only because the LDS traffic of one wave is ordered: no barrier is used. Writes the neighbour total to count[k], returns it.
template <int NG, bool INDEX, class Args, class NB>
__device__ __forceinline__ uint32_t shot_wave_neighbours(const Args& a, const ShotWave& w, float4* qd, uint32_t* qi, WaveRows& rows, NB&& nb) {
    const int lane = w.lane;
    const float cx = w.cx, cy = w.cy, cz = w.cz;
    const uint32_t* cs = a.cell_start + (size_t)w.o * ISM_GRID_STRIDE;
    const uint32_t base = a.pt_off[w.o];
    uint32_t qn = 0, qh = 0, total = 0;
    ball_for_each<NG, true>(w.m, cs, w.cr, cx, cy, cz, a.radius, lane, rows,
                  [&](uint32_t i, bool) { return a.sp4[base + i]; },      // invalid lanes carry index 0 (common.h): no branch, no zero fill
                  [&](const float4& p, uint32_t i, bool v) {
        bool pass = false; float dx = 0, dy = 0, dz = 0, d2 = 0;
        if (v) {
            const float px = p.x, py = p.y, pz = p.z;
            d2 = sqdist3(px, py, pz, cx, cy, cz);
            dx = px - cx; dy = py - cy; dz = pz - cz;
            pass = d2 < a.r2;
        }
        const unsigned long long mask = __ballot(pass);
        if (pass) {
            const uint32_t pos = (qh + qn + __popcll(mask & ((1ull << lane) - 1ull))) & 127u;
            qd[pos] = make_float4(dx, dy, dz, d2);
            if (INDEX) qi[pos] = base + i;
        }
        const uint32_t c = __popcll(mask);
        qn += c; total += c;
        if (qn >= 64) {
            const uint32_t at = (qh + lane) & 127u;
            const float4 e = qd[at];
            nb(true, INDEX ? qi[at] : 0u, e.x, e.y, e.z, e.w);
            qh = (qh + 64) & 127u; qn -= 64;
        }
    });
    if (qn > 0) {
        const bool act = (uint32_t)lane < qn;
        const uint32_t at = (qh + lane) & 127u;
        const float4 e = qd[at];
        nb(act, INDEX && act ? qi[at] : 0u, e.x, e.y, e.z, e.w);
    }
    if (a.count && lane == 0) a.count[w.k] = total;
    return total;
}
#endif

// ---- the launchers ------------------------------------------------------------------------------------------------------------
// What every entry point of the family is called with (kp_rgba: the colour descriptors only)
struct ShotCall {
    ismhip_ctx* ctx; const ismhip_cloud* cloud; const uint32_t* kp_offsets_h;
    const float *kpx, *kpy, *kpz; const uint32_t* kp_rgba; const float* lrf9;
    float radius; float* desc_out; uint32_t* count_out; const char* name;
};

// The argument checks: "<name>: bad argument" unless every array is there, the radius positive and `also` holds (what else the entry
// point asks of its scalars), then "<name>: colour arrays missing" for a colour descriptor without them.
static inline int shot_check_call(const ShotCall& c, bool also, bool colour) {
    if (!c.ctx || !c.cloud || !c.kp_offsets_h || !c.kpx || !c.kpy || !c.kpz || !c.lrf9 || !c.desc_out || !(c.radius > 0.f) || !also)
        return ism_set_err(c.ctx, ISMHIP_ERR_INVALID, std::string(c.name) + ": bad argument");
    if (colour && (!c.cloud->rgba || !c.kp_rgba)) return ism_set_err(c.ctx, ISMHIP_ERR_INVALID, std::string(c.name) + ": colour arrays missing");
    return ISMHIP_OK;
}

// Checks and uploads the keypoint offsets and fills the fields that the three argument structs share. maxk = the longest keypoint run;
// 0: nothing to describe, the entry point returns.
template <class Args>
int shot_common_args(const ShotCall& c, Args& a, uint32_t& maxk) {
    const int n_obj = c.cloud->n_obj;
    RaggedOffsets kp;
    maxk = 0;
    int rc = ism_ragged_offsets(c.ctx, c.name, c.kp_offsets_h, n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK) return rc;
    maxk = kp.max_run;
    a.pt_off = c.cloud->pt_off; a.meta = c.cloud->meta; a.cell_start = c.cloud->cell_start; a.sp4 = c.cloud->sp4;
    a.kp_off = kp.dev; a.kx = c.kpx; a.ky = c.kpy; a.kz = c.kpz; a.lrf = c.lrf9;
    a.radius = c.radius; a.r2 = (float)((double)c.radius * (double)c.radius);
    a.desc = c.desc_out; a.count = c.count_out;
    a.n_obj = c.ctx->xcd_map ? n_obj : 0; a.nbx = (int)((maxk + 3) / 4);
    return ISMHIP_OK;
}

// Under the entry point's timer: the keypoints in cell order, then four waves per workgroup on the XCD block map with `lds` bytes of
// dynamic LDS.
template <class Args>
int shot_launch(const ShotCall& c, Args& a, uint32_t maxk, void (*kernel)(Args), size_t lds) {
    TimerScope ts(c.ctx, c.name);
    a.kp_perm = ism_kp_order(c.ctx, c.cloud, c.kp_offsets_h, a.kp_off, c.kpx, c.kpy, c.kpz, maxk);
    const dim3 grid(c.ctx->xcd_map ? xcd_object_grid((unsigned)a.nbx, c.cloud->n_obj) : (unsigned)a.nbx * (unsigned)c.cloud->n_obj);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, c.ctx->stream, a);
    ISM_CHECK_LAUNCH(c.ctx, c.name);
    return ISMHIP_OK;
}

// short_cshot.hip — the Short SHOT with its colour histogram (Features type "SHORT_CSHOT"), one 64-lane wavefront per keypoint.
// Reference seam: FeaturesSHORTCSHOT::compute_descriptor / compute_shape_descriptor / compute_color_descriptor / linear_interpolation /
// correct_bin (features/features_short_cshot.cpp:103-507). The row is the SHORT_SHOT histogram of Ds = r e a bins on the shape grid,
// followed by Dc H bins: a histogram of H colour-distance bins in every cell of a SECOND spherical grid of Dc = rc ec ac cells; the
// two parts are L2-normalised together. A neighbour therefore takes two independent sets of hard decisions on its raw r / theta / phi
// values (one per grid) and one on raw_c = colour distance * H.
//
// Gather model: algorithmic bytes per keypoint = M_k * 32 + 12 + 36 + 4 + 4 * D (M_k = radius neighbours, D = Ds + Dc H <= 1344): the
// 16-byte point record of k_short_shot plus the neighbour's 16-byte normalised CIELab record (slab4, gathered by the queued index as
// k_shot<true> does), the keypoint, its frame and colour, the row.
//
// Structure per wave: that of k_short_shot (the XCD block map, ball_for_each<16, true> over sp4, the ballot-compacted 128-entry queue,
// full waves of neighbours, 2^-28 fixed-point ds_add_u64 deposits); the steps a neighbour takes are those of short_common.h. The
// geometry is ESTIMATED once in float (r, theta, phi) and scaled per grid; where a raw value of EITHER grid comes within eps of a
// decision the reference's FP64 sequence is taken for both. The colour side needs no estimate: float subtractions, fabsf, one
// multiplication by 0.5, two additions, an IEEE division by 3, the clamp and the product with (float)H are each exactly the
// reference's operation (the product is the reference's double product rounded once: a 24-bit by <= 11-bit product is exact in double).
// Deviation: the colour distance is taken in float as in PCL's cshot.hpp, from which the reference says it copied the
// block, and as in k_shot<true>; the reference's unqualified fabs does not pin float against double.
//
// Increments: every share is a float in [0.5, 1] (a hair below 0.5 only for phi = -180 degrees) and a multiple of 2^-24, so a sum of
// four is exact in float whatever the order, lies in [1, 4], and round(v * 2^28) <= 2^30 fits 32 bits. The secondary COLOUR bin
// receives (1 - f_c) + (1 - f_r) + f_theta + f_phi exactly as the reference writes it (:424) -- with 1 - f_r, not f_r: bug-compatible.
//
// The per-wave histogram lives in dynamic LDS, sized by the launch (D 64-bit slots per wave): 30 KiB per workgroup at the default 512
// bins (5 workgroups per CU by LDS), 56 KiB at the 1344 cap (2 per CU). No histogram copies for short rows: the default row spreads a
// wave's deposits over 15 colour bins per cell already.
#include "short_common.h"

namespace {

struct ShortCshotArgs {
    const uint32_t* pt_off; const GridMeta* meta; const uint32_t* cell_start;
    const float4 *sp4, *slab4;
    const uint32_t* kp_off; const float *kx, *ky, *kz; const uint32_t* kp_rgba;
    const float* lrf; float radius, r2;
    double radius_d, min_radius, ln_rmin, ln_rmax_rmin;
    SshotScale gs, gc;                         // the float estimate's scales and eps on the shape grid and on the colour grid
    float min_radius_f, hist_size_f;
    int log_radius, r_bins, e_bins, a_bins, rc_bins, ec_bins, ac_bins, hist_size, same_grid;
    const float *lut_srgb, *lut_sxyz;
    float* desc; uint32_t* count;
    int n_obj, nbx;
    const uint32_t* kp_perm;   // keypoints in cell order (nullptr: as they come)
};

struct ShortCshotSmem {
    float4 qd[4][128];       // dx, dy, dz, d2 of queued neighbours
    uint32_t qi[4][128];     // sorted index of queued neighbours (their Lab record is gathered when they are processed)
    WaveRows rows[4];
};

// compute_color_descriptor (:312-429) from the float raw values on: up to five deposits into hist[ds .. dim)
__device__ __forceinline__ void scshot_color_deposits(sshot_bin_t* hist, int dim, int ds, int rb, int eb, int ab, int hs,
                                                      float raw_r, float raw_theta, float raw_phi, float raw_c) {
    const SshotAxis r = sshot_axis<true, false>(raw_r, rb), t = sshot_axis<false, false>(raw_theta, eb), p = sshot_axis<false, true>(raw_phi, ab);
    const SshotAxis c = sshot_axis<false, false>(raw_c, hs);
    const int hr = hs * rb, hre = hr * eb;
    hist += ds; dim -= ds;
    sshot_dep(hist, dim, c.bin + r.bin * hs + t.bin * hr + p.bin * hre, ((c.f + r.f) + t.f) + p.f);
    if (ab > 1 && p.bin2 != p.bin) sshot_dep(hist, dim, c.bin + r.bin * hs + t.bin * hr + p.bin2 * hre, ((c.f + r.f) + t.f) + (1.0f - p.f));
    if (eb > 1 && t.bin2 != t.bin) sshot_dep(hist, dim, c.bin + r.bin * hs + t.bin2 * hr + p.bin * hre, ((c.f + r.f) + (1.0f - t.f)) + p.f);
    if (rb > 1 && r.bin2 != r.bin) sshot_dep(hist, dim, c.bin + r.bin2 * hs + t.bin * hr + p.bin * hre, ((c.f + (1.0f - r.f)) + t.f) + p.f);
    if (hs > 1 && c.bin2 != c.bin) sshot_dep(hist, dim, c.bin2 + r.bin * hs + t.bin * hr + p.bin * hre, (((1.0f - c.f) + (1.0f - r.f)) + t.f) + p.f);   // :424 as written
}

// Per-neighbour update (:167-202). All 64 lanes call it; 'act' marks lanes that hold a neighbour, gi its sorted point index.
__device__ __forceinline__ void scshot_neighbour(const ShortCshotArgs& a, sshot_bin_t* hist, int dim, int ds, bool act, uint32_t gi,
                                                 float dx, float dy, float dz, float d2,
                                                 const float fx[3], const float fy[3], const float fz[3], float LRef, float aRef, float bRef) {
    if (!act) return;
    if (d2 <= 1e-15f) return;                                                     // distances[j] > 1E-15 on the SQUARED distance (:169)
    const float4 lab = a.slab4[gi];
    const float xf = (dx * fx[0] + dy * fx[1]) + dz * fx[2];                      // float products, unfused, in this order
    const float yf = (dx * fy[0] + dy * fy[1]) + dz * fy[2];
    const float zf = (dx * fz[0] + dy * fz[1]) + dz * fz[2];
    float r, theta, phi, sr, st, sp, cr, ct, cp;
    bool below_min;
    sshot_polar(xf, yf, zf, r, theta, phi);
    const bool s_clear = sshot_scaled(a.gs, r, theta, phi, sr, st, sp);
    const bool c_clear = sshot_scaled(a.gc, r, theta, phi, cr, ct, cp);
    const bool min_clear = sshot_min_clear(r, a.min_radius_f, below_min);
    if (a.log_radius || !min_clear || !s_clear || !c_clear) {
        const float4 e = sshot_exact(xf, yf, zf, a.radius_d, a.min_radius, a.ln_rmin, a.ln_rmax_rmin, a.log_radius, a.r_bins, a.e_bins, a.a_bins);
        sr = e.x; st = e.y; sp = e.z; below_min = e.w != 0.f;
        cr = sr; ct = st; cp = sp;
        if (!a.same_grid) {
            const float4 g = sshot_exact(xf, yf, zf, a.radius_d, a.min_radius, a.ln_rmin, a.ln_rmax_rmin, a.log_radius, a.rc_bins, a.ec_bins, a.ac_bins);
            cr = g.x; ct = g.y; cp = g.z;
        }
    }
    if (below_min) return;
    sshot_shape_deposits(hist, ds, a.r_bins, a.e_bins, a.a_bins, sr, st, sp);
    float cd = (fabsf(LRef - lab.x) + ((fabsf(aRef - lab.y) + fabsf(bRef - lab.z)) * 0.5f)) / 3.0f;   // feeds a hard bin: exact division (:194)
    cd = fminf(1.0f, fmaxf(0.0f, cd));
    scshot_color_deposits(hist, dim, ds, a.rc_bins, a.ec_bins, a.ac_bins, a.hist_size, cr, ct, cp, cd * a.hist_size_f);
}

// 123 VGPRs (52 scalar registers kept in vector-register lanes), no scratch, 14 KiB static + 32 D bytes dynamic LDS per workgroup: 4 waves
// per SIMD by registers (the compiler's resource report)
__global__ __launch_bounds__(256, 4) void k_short_cshot(ShortCshotArgs a) {
    __shared__ ShortCshotSmem sm;
    extern __shared__ sshot_bin_t scshot_hist[];                        // [4][D]
    int o, bx;
    if (!xcd_object_block(a.nbx, a.n_obj, o, bx)) return;
    const int wv = threadIdx.x >> 6;
    const int lane = lane_id();
    if (a.kp_off[o] + bx * 4 + wv >= a.kp_off[o + 1]) return;          // wave-uniform; no block-level barrier below
    const uint32_t k = ordered_keypoint(a.kp_perm, a.kp_off[o], (uint32_t)(bx * 4 + wv));
    const int Ds = a.r_bins * a.e_bins * a.a_bins;                      // 1 .. 256
    const int D = Ds + a.rc_bins * a.ec_bins * a.ac_bins * a.hist_size; // .. 1344 (both checked by the launcher, which sizes the LDS by D)
    float* out = a.desc + (size_t)k * D;
    const float cx = a.kx[k], cy = a.ky[k], cz = a.kz[k];
    const float* f = a.lrf + (size_t)k * 9;
    const float fx[3] = {f[0], f[1], f[2]}, fy[3] = {f[3], f[4], f[5]}, fz[3] = {f[6], f[7], f[8]};
    const GridMeta m = a.meta[o];
    CellRange cr;
    const bool ok = isfinite(fx[0]) && isfinite(fy[0]) && isfinite(fz[0]) && isfinite(cx) && isfinite(cy) && isfinite(cz);
    if (!ok || !ball_cells(m, cx, cy, cz, a.radius, cr)) {
        for (int i = lane; i < D; i += 64) out[i] = __builtin_nanf("");
        if (a.count && lane == 0) a.count[k] = 0;
        return;
    }
    sshot_bin_t* hist = scshot_hist + (size_t)wv * D;
    for (int i = lane; i < D; i += 64) hist[i] = 0ull;
    float LRef, aRef, bRef;
    rgb2lab_norm(a.lut_srgb, a.lut_sxyz, a.kp_rgba[k], LRef, aRef, bRef);   // the keypoint's own colour is the reference colour (:148-155)
    const uint32_t* cs = a.cell_start + (size_t)o * ISM_GRID_STRIDE;
    const uint32_t base = a.pt_off[o];
    uint32_t qn = 0, qh = 0, total = 0;
    ball_for_each<16, true>(m, cs, cr, cx, cy, cz, a.radius, lane, sm.rows[wv],
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
            const uint32_t pos = (qh + qn + __popcll(mask & ((1ull << lane) - 1ull))) & 127u;      // 128-entry circular queue
            sm.qd[wv][pos] = make_float4(dx, dy, dz, d2); sm.qi[wv][pos] = base + i;
        }
        const uint32_t c = __popcll(mask);
        qn += c; total += c;
        if (qn >= 64) {
            // a full wave of neighbours (LDS traffic of one wave is ordered; no barrier needed)
            const uint32_t at = (qh + lane) & 127u;
            const float4 e = sm.qd[wv][at];
            scshot_neighbour(a, hist, D, Ds, true, sm.qi[wv][at], e.x, e.y, e.z, e.w, fx, fy, fz, LRef, aRef, bRef);
            qh = (qh + 64) & 127u; qn -= 64;
        }
    });
    if (qn > 0) {
        const bool act = (uint32_t)lane < qn;
        const uint32_t at = (qh + lane) & 127u;
        const float4 e = sm.qd[wv][at];
        scshot_neighbour(a, hist, D, Ds, act, act ? sm.qi[wv][at] : 0u, e.x, e.y, e.z, e.w, fx, fy, fz, LRef, aRef, bRef);
    }
    if (a.count && lane == 0) a.count[k] = total;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");             // the deposits of the other lanes are read below
    // L2 norm of the fused row (:204-220): double sum of squares, sqrt, double division, cast to float. No contributing neighbour:
    // 0 / 0, a NaN row. The bins are integers: reading them twice gives the same values.
    double acc = 0.0;
    for (int i = lane; i < D; i += 64) { const double v = (double)hist[i] * SSHOT_FIX_INV; acc += v * v; }
    const double norm = sqrt(wave_sum_d(acc));
    for (int i = lane; i < D; i += 64) out[i] = (float)(((double)hist[i] * SSHOT_FIX_INV) / norm);
}

}  // namespace

extern "C" {

int ismhip_short_cshot(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                       const float* kpx, const float* kpy, const float* kpz, const uint32_t* kp_rgba, const float* lrf9,
                       float radius, float min_radius, int log_radius, int r_bins, int e_bins, int a_bins,
                       int rc_bins, int ec_bins, int ac_bins, int hist_size, float* desc_out, uint32_t* neighbour_count_out) {
    const char* name = "short_cshot";
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (r_bins < 1 || e_bins < 1 || a_bins < 1 || rc_bins < 1 || ec_bins < 1 || ac_bins < 1)
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_cshot: fewer than one bin on an axis");
    if (hist_size < 1) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_cshot: colour histogram of fewer than one bin");
    const long long ds = (long long)r_bins * e_bins * a_bins;
    if (ds > ISMHIP_SHORT_SHOT_MAX_DIM) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "short_cshot: more than 256 shape bins");
    // a factor at a time, stopping above the cap: the product of four ints cannot overflow
    long long dc = (long long)rc_bins * ec_bins;
    if (dc <= ISMHIP_SHORT_CSHOT_MAX_DIM) dc *= ac_bins;
    if (dc <= ISMHIP_SHORT_CSHOT_MAX_DIM) dc *= hist_size;
    if (ds + dc > ISMHIP_SHORT_CSHOT_MAX_DIM) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "short_cshot: row longer than 1344 bins");
    if (!cloud || !kp_offsets_h || !kpx || !kpy || !kpz || !lrf9 || !desc_out || !(radius > 0.f) || !(min_radius >= 0.f) || !std::isfinite(min_radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_cshot: bad argument");
    if (!cloud->rgba || !kp_rgba) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_cshot: colour arrays missing");
    // the reference divides by log(Radius / min_radius): 0 for min_radius == 0 (and NaN -> int); refused, never altered
    if (log_radius && !(min_radius > 0.f && min_radius < radius))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "short_cshot: logarithmic radius needs 0 < min_radius < radius");
    const int n_obj = cloud->n_obj;
    RaggedOffsets kp;
    int rc = ism_ragged_offsets(ctx, name, kp_offsets_h, n_obj, SCR_KP_OFF, 0, &kp);
    if (rc != ISMHIP_OK) return rc;
    const uint32_t maxk = kp.max_run;
    if (maxk == 0) return ISMHIP_OK;
    ShortCshotArgs a;
    a.pt_off = cloud->pt_off; a.meta = cloud->meta; a.cell_start = cloud->cell_start; a.sp4 = cloud->sp4; a.slab4 = cloud->slab4;
    a.kp_off = kp.dev; a.kx = kpx; a.ky = kpy; a.kz = kpz; a.kp_rgba = kp_rgba; a.lrf = lrf9;
    a.radius = radius; a.r2 = (float)((double)radius * (double)radius);
    a.radius_d = (double)radius; a.min_radius = (double)min_radius;
    a.ln_rmin = min_radius == 0.f ? 0.0 : log((double)min_radius);
    a.ln_rmax_rmin = min_radius == 0.f ? 0.0 : log((double)radius / (double)min_radius);
    a.log_radius = log_radius ? 1 : 0; a.r_bins = r_bins; a.e_bins = e_bins; a.a_bins = a_bins;
    a.rc_bins = rc_bins; a.ec_bins = ec_bins; a.ac_bins = ac_bins; a.hist_size = hist_size; a.hist_size_f = (float)hist_size;
    a.same_grid = (r_bins == rc_bins && e_bins == ec_bins && a_bins == ac_bins) ? 1 : 0;
    a.gs = sshot_scale_of(r_bins, e_bins, a_bins, radius);
    a.gc = sshot_scale_of(rc_bins, ec_bins, ac_bins, radius);
    a.min_radius_f = min_radius;
    a.lut_srgb = ctx->lut_srgb; a.lut_sxyz = ctx->lut_sxyz;
    a.desc = desc_out; a.count = neighbour_count_out;
    a.n_obj = ctx->xcd_map ? n_obj : 0; a.nbx = (int)((maxk + 3) / 4);
    TimerScope ts(ctx, name);
    a.kp_perm = ism_kp_order(ctx, cloud, kp_offsets_h, kp.dev, kpx, kpy, kpz, maxk);
    const dim3 grid(ctx->xcd_map ? xcd_object_grid((unsigned)a.nbx, n_obj) : (unsigned)a.nbx * (unsigned)n_obj);
    const size_t lds = (size_t)4 * (size_t)(ds + dc) * sizeof(sshot_bin_t);          // <= 43 008 bytes: with the 14 KiB static part inside the 64 KiB default
    hipLaunchKernelGGL(k_short_cshot, grid, dim3(256), lds, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, name);
    return ISMHIP_OK;
}

}  // extern "C"

// knn.hip — exact k-nearest-codeword search (codebook activation).
// Reference seam: ActivationStrategyKNN::activateKNN (activation_strategy/activation_strategy_knn.h:41-126) with
// FLANNExactMatch semantics (flann::SearchParams(-1)); distance functors utils/distance.h:45,65 (FLANN L2 = squared
// Euclidean, ChiSquareDistance), SURVEY Appendix A.6.
//
// Three stages, one unit per phase and heavy kernel family; every kernel is defined in the unit that launches it,
// and the units call each other through the host functions declared in knn_internal.h:
//  1. candidate generation (the dominant kernel of the whole path). Score(c,q) = |c|^2 - 2 c.q as a dense [codewords x queries]
//     contraction on the matrix cores; codewords are the MFMA ROWS and queries the COLUMNS, so a lane holds 16 codeword scores of
//     ONE query per accumulator tile: the running top-T per query lives in registers with no cross-lane traffic and the Nq x Nc
//     matrix is never materialised. Every kernel keeps, per lane slot, the T best candidates AND the value of the best candidate
//     it dropped (the slot's bound).
//       knn_ring16.hip   k_knn_l2_ring16  f16 MFMA, 256x256 tile, LDS-DMA ring         default for launches >= 4096 queries x 4096 codewords
//                                         (its tile epilogue: at the kernel in that unit, and DESIGN.md §4.1 "Hit path")
//       knn_mfma16.hip   k_knn_l2_mfma16  f16 (or bf16x3) MFMA, register-staged tiles  smaller launches; bf16x3 for A/B runs; EMIT variant
//       knn_cand.hip     k_knn_l2_mfma    f32 MFMA (exact fma chain)                   ISMHIP_KNN_MODE=f32: the independent route used by the tests
//                        k_knn_chi2       VALU 64x64 tile, v_rcp_f32                   chi-square is not a contraction
//  2. knn_rerank.hip: exact functor values of the candidates that matter, the k best, a proof slot by slot; what it cannot prove is queued for
//  3. knn_scan.hip: k_knn_fallback / k_knn_fallback_merge — exact scan of the queued slots' rows. Rare for descriptor data, the rule for
//     adversarial inputs (un-normalised magnitudes, hundreds of near-duplicates): it keeps the answer exact in every case.
//  This file: the query / codebook images the candidate kernels read (the f16 scale rule and the tiled layout: knn_internal.h), knn_plan
//  and run_knn -- one search is knn_carve_scratch, knn_query_images, knn_launch_candidates, knn_rerank_prove, knn_scan_queue on one
//  stream -- and the entry points ismhip_knn, _ratio, _rule. Above it, knn_two_stage.hip: run_knn_two_stage (squared L2: stage 1 with
//  T = 2 on the rotated image, then a seeded stage 2 on the rows of the stage-1 splits whose proof failed, or on the whole codebook) and
//  run_knn_chi2_hellinger (chi-square: Hellinger candidates on the matrix cores, an EMIT sweep for what they leave open);
//  knn_threshold.hip (radius search) and knn_large_k.hip (any K up to 1024).
#include "knn_internal.h"

namespace {

__device__ __forceinline__ u16 f32_to_bf16_rn(float x) {
    const unsigned u = __float_as_uint(x);
    return (u16)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// rows beyond n and columns beyond dim are zero; hi = RN_bf16(x), lo = RN_bf16(x - hi)
__global__ void k_split_bf16(const float* __restrict__ src, int n, int dim, int ld, int n_pad, int dim_pad,
                             u16* __restrict__ hi, u16* __restrict__ lo) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_pad * dim_pad) return;
    const int row = (int)(i / dim_pad), col = (int)(i % dim_pad);
    float x = 0.f;
    if (row < n && col < dim) x = src[(size_t)row * ld + col];
    const u16 h = f32_to_bf16_rn(x);
    const float hf = __uint_as_float((unsigned)h << 16);
    hi[i] = h; lo[i] = f32_to_bf16_rn(x - hf);
}

// ---- f16 image (NTERM = 1; scale rule and layout: knn_internal.h). absmax is kept as float bits (non-negative floats order like
// uints; NaN/inf sort last and select s = 1, the affected scores become NaN/inf and those queries take the exact path).
__global__ void k_absmax(const float* __restrict__ src, int n, int dim, int ld, uint32_t* __restrict__ out_bits) {
    uint32_t m = 0u;
    const size_t tot = (size_t)n * dim;
    if (ld == dim) {                                   // contiguous rows: a flat, 16-byte-wide sweep
        const size_t n4 = tot >> 2;
        const uint4* s4 = (const uint4*)src;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
            const uint4 v = s4[i];
            const uint32_t a = max(max(v.x & 0x7fffffffu, v.y & 0x7fffffffu), max(v.z & 0x7fffffffu, v.w & 0x7fffffffu));
            m = a > m ? a : m;
        }
        for (size_t i = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
            const uint32_t b = __float_as_uint(src[i]) & 0x7fffffffu; m = b > m ? b : m;
        }
    } else
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / dim), col = (int)(i % dim);
        const uint32_t b = __float_as_uint(src[(size_t)row * ld + col]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    __shared__ uint32_t s_m[4];                        // one atomic per workgroup: thousands of same-address atomics serialise
    m = block_max_u32(m, s_m);
    if (threadIdx.x == 0 && m) atomicMax(out_bits, m);
}
// sc[0] = absmax bits (in), sc[1] = -2 / (s * other_scale) (out), sc[2] = 2^-14 / s (out: worst-case absolute element error);
// returns s. Thread 0 of the grid writes the two.
__device__ __forceinline__ float f16_image_scalars(uint32_t* __restrict__ sc, float other_scale, size_t i) {
    const float s = f16_scale_for(sc[0]);
    if (i == 0) {
        ((float*)sc)[1] = -2.0f / (s * other_scale);
        ((float*)sc)[2] = (sc[0] >> 23) == 255u ? __builtin_inff() : F16_FLUSH / s;     // inf/NaN in the batch: nothing is provable
    }
    return s;
}
// element (row, col) of the image: zero beyond n rows / dim columns
__device__ __forceinline__ u16 f16_image_element(const float* __restrict__ src, int n, int dim, int ld, size_t row, int col, float s) {
    float x = 0.f;
    if (row < (size_t)n && col < dim) x = src[row * ld + col];
    const _Float16 hx = (_Float16)(x * s);            // v_cvt_f16_f32, round to nearest even
    return __builtin_bit_cast(u16, hx);
}
__global__ void k_to_f16(const float* __restrict__ src, int n, int dim, int ld, int n_pad, int dim_pad,
                         uint32_t* __restrict__ sc, float other_scale, u16* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float s = f16_image_scalars(sc, other_scale, i);
    if (i >= (size_t)n_pad * dim_pad) return;
    dst[i] = f16_image_element(src, n, dim, ld, i / dim_pad, (int)(i % dim_pad), s);
}
// The same conversion into the tiled layout k_knn_l2_ring16 streams (knn_internal.h): thread i writes half i of the image
__global__ void k_to_f16_tiled(const float* __restrict__ src, int n, int dim, int ld, int n_tiles, int nk,
                               uint32_t* __restrict__ sc, float other_scale, u16* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float s = f16_image_scalars(sc, other_scale, i);
    if (i >= f16t_halves(n_tiles, nk)) return;
    const int e = (int)(i & 7), p = (int)((i >> 3) & 3), r = (int)((i / F16T_KB) % F16T_ROWS);
    const size_t blk = i / F16T_BLOCK;
    const int col = (int)(blk % nk) * F16T_KB + ((p ^ f16t_swizzle(r)) << 3) + e;          // the swizzle is its own inverse
    dst[i] = f16_image_element(src, n, dim, ld, blk / nk * F16T_ROWS + r, col, s);
}

// |c|^2 / out_scale for every codebook row (out_scale is known on the device only: it holds the batch's query scale)
__global__ void k_scale_norms(const float* __restrict__ norm, int n, const float* __restrict__ out_scale, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = norm[i] * (1.0f / out_scale[0]);
}
__global__ void k_pad_rows(const float* __restrict__ src, int n, int dim, float* __restrict__ dst, int dim_pad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * dim_pad) return;
    const int row = (int)(i / dim_pad), col = (int)(i % dim_pad);
    dst[i] = col < dim ? src[(size_t)row * dim + col] : 0.f;
}

// sqrt of every element (rows padded to dim_pad with zeros); flag[0] |= 1 when an element is negative or NaN
__global__ void k_sqrt_rows(const float* __restrict__ src, int n, int dim, int ld, int dim_pad, float* __restrict__ dst, uint32_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < (size_t)n * dim_pad) {
        const int row = (int)(i / dim_pad), col = (int)(i % dim_pad);
        float v = 0.f;
        if (col < dim) { v = src[(size_t)row * ld + col]; bad = !(v >= 0.f); }
        dst[i] = sqrtf(v);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

__global__ void k_ratio(int nq, float thr, const int32_t* __restrict__ idx2, const float* __restrict__ d2,
                        int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    int id = idx2[i * 2]; const float a = d2[i * 2], b = d2[i * 2 + 1];
    if (idx2[i * 2 + 1] >= 0 && a / b > thr) id = -1;        // activation_strategy_knn.h:77-84
    idx_out[i] = id; dist_out[i] = a;
}

// ActivationStrategyKnnRule::activateKNN, detection branch (activation_strategy_knn_rule.h:79-118)
__global__ void k_rule(int nq, float thr, const int32_t* __restrict__ idx3, const float* __restrict__ d3, const uint32_t* __restrict__ word_class,
                       int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int i0 = idx3[i * 3], i1 = idx3[i * 3 + 1], i2 = idx3[i * 3 + 2];
    const float a = d3[i * 3], b = d3[i * 3 + 1], c = d3[i * 3 + 2];
    int id = -1; float dd = __builtin_nanf("");
    if (i2 < 0) {                       // fewer than 4 codewords: the reference returns all of them; report the nearest
        if (i0 >= 0) { id = i0; dd = a; }
    } else {
        const uint32_t c0 = word_class[i0], c1 = word_class[i1], c2 = word_class[i2];
        if (c0 == c1 && c0 == c2) { id = i0; dd = a; }
        else if (c0 == c1 && c0 != c2) { if (a / c < thr) { id = i0; dd = a; } }
        else if (c0 != c1 && c1 == c2) { if (a / b >= thr) { id = i1; dd = b; } }
        else if (c0 != c1 && c1 != c2) { if (a / b < thr) { id = i0; dd = a; } }
    }
    idx_out[i] = id; dist_out[i] = dd;
}

// candidate lists | slot bounds (| the folded slot of a merge); candidate rows; counter block | the search's own queue (knn_scan.hip)
int knn_carve_scratch(KnnRun& r) {
    const KnnPlan& p = r.p; const size_t nq = (size_t)r.nq, q_items = nq * p.n_bound;
    r.n_cand = p.n_cand; r.n_bound = p.n_bound;
    r.cand_val = (float*)ism_scratch(r.ctx, SCR_KNN_CAND_VAL, nq * (p.n_cand + p.n_bound + (p.merged ? KNN_MERGE_KEEP + 1 : 0)) * sizeof(float));
    r.cand_idx = (int*)ism_scratch(r.ctx, SCR_KNN_CAND_IDX, nq * (p.n_cand + (p.merged ? KNN_MERGE_KEEP : 0)) * sizeof(int));
    r.counters = (uint32_t*)ism_scratch(r.ctx, SCR_KNN_FLAGS, knn_queue_bytes(nq, q_items, r.k));
    if (!r.cand_val || !r.cand_idx || !r.counters) return ISMHIP_ERR_NOMEM;
    r.cand_bound = r.cand_val + nq * p.n_cand; r.qsc = r.counters + KNN_CNT_QSC;
    ISM_HIP(r.ctx, hipMemsetAsync(r.counters, 0, KNN_CNT_WORDS * sizeof(uint32_t), r.ctx->stream));
    r.queue = r.rq->ranged ? *r.rq->ranged->queue : knn_queue_carve(r.counters, nq, q_items);
    return ISMHIP_OK;
}

// the 16-bit images of the query batch (none for the f32 and chi-square candidates)
int knn_query_images(KnnRun& r) {
    ismhip_ctx* ctx = r.ctx; const ismhip_codebook* cb = r.cb; const KnnPlan& p = r.p; const int nq = r.nq;
    if (p.mode != 0 && p.mode != 1) return ISMHIP_OK;
    const bool ring = p.cand == KNN_CAND_RING16;
    const int nq_pad = ring ? (nq + F16T_ROWS - 1) / F16T_ROWS * F16T_ROWS : (nq + p.BN - 1) / p.BN * p.BN;
    const size_t tot = ring ? f16t_halves(nq_pad / F16T_ROWS, p.ring_nk) : (size_t)nq_pad * cb->ld16;
    r.q_hi = (u16*)ism_scratch(ctx, SCR_KNN_QSPLIT, tot * 2 * sizeof(u16));
    if (!r.q_hi) return ISMHIP_ERR_NOMEM;
    r.q_lo = r.q_hi + tot;
    if (p.pca) {
        TimerScope tr(ctx, "knn_rotate");
        float* norms = (float*)r.q_lo;                                    // (no second image on this route: nq_pad * 2 floats fit in its place)
        const int rc = ism_pca_rotate_queries(ctx, cb, r.PI, r.qq, nq, r.ldq, r.q_hi, norms, norms + nq_pad);
        if (rc != ISMHIP_OK) return rc;
        if (ism_pca_split_queries(ctx, r.PI)) { r.qn2 = norms; r.qn2h = norms + nq_pad; }
        ++ctx->knn_pca_launches;
    } else if (p.mode == 0) {
        const float* cq = p.hell ? r.rq->hell_q : r.qq; const int cldq = p.hell ? cb->dim_pad : r.ldq;     // Hellinger: the images are made from sqrt(q)
        hipLaunchKernelGGL(k_absmax, dim3(512), dim3(256), 0, ctx->stream, cq, nq, cb->dim, cldq, r.qsc);
        ISM_CHECK_LAUNCH(ctx, "k_absmax");
        if (ring) hipLaunchKernelGGL(k_to_f16_tiled, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, cq, nq, cb->dim, cldq, nq_pad / F16T_ROWS, p.ring_nk, r.qsc, r.xb->f16_scale, r.q_hi);
        else hipLaunchKernelGGL(k_to_f16, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, cq, nq, cb->dim, cldq, nq_pad, cb->ld16, r.qsc, r.xb->f16_scale, r.q_hi);
        ISM_CHECK_LAUNCH(ctx, "k_to_f16");
    } else {
        hipLaunchKernelGGL(k_split_bf16, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, r.qq, nq, cb->dim, r.ldq, nq_pad, cb->ld16, r.q_hi, r.q_lo);
        ISM_CHECK_LAUNCH(ctx, "k_split_bf16");
    }
    return ISMHIP_OK;
}

// the candidate kernel of the plan
int knn_launch_candidates(KnnRun& r) {
    ismhip_ctx* ctx = r.ctx; const ismhip_codebook *cb = r.cb, *xb = r.xb; const KnnPlan& p = r.p; const PcaImage& PI = *r.PI; const int nq = r.nq;
    {
        TimerScope ts(ctx, r.rq->tname ? r.rq->tname : (r.metric == ISMHIP_METRIC_L2SQ ? "knn_l2_mfma" : "knn_chi2"));      // chi-square: whichever kernel makes its candidates
        const unsigned grid = 8 * ((p.n_qt + 7) / 8) * p.n_splits;
        KnnCandArgs a{};                                                     // the 16-bit kernels; f32 and chi-square read the codebook itself
        a.n_tiles_m = cb->n_words_pad / p.BM; a.ld = cb->ld16; a.k_steps = p.pca ? PI.m / 16 : (cb->dim + 15) / 16;
        a.qh = r.q_hi; a.ql = r.q_lo; a.nq = nq; a.out_scale = (const float*)(r.qsc + 1);
        a.tiles_per_split = p.tiles_per_split; a.n_splits = p.n_splits;
        a.cand_val = r.cand_val; a.cand_idx = r.cand_idx; a.cand_stride = r.n_cand; a.cand_bound = r.cand_bound; a.bound_stride = r.n_bound;
        a.qrange = p.ranged ? r.rq->ranged->qrange : nullptr;
        a.split_major = p.split_major;
        int rc = ISMHIP_OK;
        if (p.cand == KNN_CAND_RING16) {
            rc = ism_lds_cap(ctx, p.kern, p.lds_cap);
            if (rc != ISMHIP_OK) return rc;
            a.wh = xb->words_f16t;
            if (p.pca) { a.wh = PI.f16t; a.out_scale = PI.osc; a.word_norm = PI.cn_scaled; }      // scales fixed per codebook: the C operand is precomputed
            else {
                float* cn_scaled = (float*)ism_scratch(ctx, SCR_QNORM2, ((size_t)cb->n_words_pad + 256) * sizeof(float));   // the |c|^2 DMA of a 128-row tile reads 256 floats
                if (!cn_scaled) return ISMHIP_ERR_NOMEM;
                hipLaunchKernelGGL(k_scale_norms, dim3((cb->n_words_pad + 255) / 256), dim3(256), 0, ctx->stream, xb->word_norm, cb->n_words_pad, a.out_scale, cn_scaled);
                ISM_CHECK_LAUNCH(ctx, "k_scale_norms");
                a.word_norm = cn_scaled;
            }
            unsigned int* clock = nullptr;                                   // joined codeword streams, one clock per (XCD, split)
            if (p.join) {
                clock = (unsigned int*)ism_scratch(ctx, SCR_KNN_CLOCK, 8 * 64 * sizeof(unsigned int));
                if (!clock) return ISMHIP_ERR_NOMEM;
                ISM_HIP(ctx, hipMemsetAsync(clock, 0, 8 * 64 * sizeof(unsigned int), ctx->stream));
            }
            float* thr0 = nullptr;                                           // the pre-pass leaves the start thresholds here
            float relax = 0.f;
            if (p.prepass || p.seeded) {
                thr0 = (float*)ism_scratch(ctx, SCR_KNN_THR0, (size_t)((nq + 255) / 256 * 256) * sizeof(float));
                if (!thr0) return ISMHIP_ERR_NOMEM;
                // relaxation: gamma x the second moment the truncation leaves out (codeword + query side, taken as equal), in
                // accumulator units (score / out_scale); the original image truncates nothing
                if (p.pca) relax = -ctx->knn_pre_gamma * 2.0f * PI.resid2 * (PI.sq * PI.sc * 0.5f);
            }
            if (p.seeded && (rc = knn_seed_thresholds(r, a.out_scale, thr0)) != ISMHIP_OK) return rc;
            rc = knn_ring16_launch(ctx, r.T, p.kern, grid, p.threads, p.lds, a, clock, thr0, p.prepass ? ctx->knn_pre_step : 0, relax);
        } else if (p.cand == KNN_CAND_MFMA16) {
            rc = ism_lds_cap(ctx, p.kern, p.lds_cap);
            if (rc != ISMHIP_OK) return rc;
            a.wh = p.mode == 0 ? xb->words_f16 : xb->words_bf16_hi;
            a.wl = p.mode == 0 ? nullptr : xb->words_bf16_lo;
            a.word_norm = xb->word_norm;
            rc = knn_mfma16_launch(ctx, p.kern, grid, p.threads, p.lds, a, nullptr, nullptr, nullptr, 0);
        } else if (p.cand == KNN_CAND_F32) {
            rc = knn_l2_f32_launch(ctx, r.T, grid, cb, r.qq, nq, r.ldq, p.tiles_per_split, p.n_splits, r.cand_val, r.cand_idx, r.n_cand, r.cand_bound, r.n_bound);
        } else {
            rc = knn_chi2_launch(ctx, r.T, p.n_qt, cb, r.qq, nq, r.ldq, r.counters + KNN_CNT_NEGATIVE, p.tiles_per_split, p.n_splits, r.cand_val, r.cand_idx, r.n_cand, r.cand_bound, r.n_bound);
        }
        if (rc != ISMHIP_OK) return rc;
    }
    return ISMHIP_OK;
}

KnnSlotRows knn_fb_desc(const KnnPlan& p, const ismhip_codebook* cb) { return KnnSlotRows{p.fb_tiles_per_split, cb->n_words_pad / p.BM, p.BM, (int)p.fb_layout, p.n_splits}; }
}  // namespace

KnnPlan knn_plan(const ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, int k, int T, const KnnRequest& rq) {
    KnnPlan p{};
    // hell_q != nullptr (chi-square only): candidates come from the squared-L2 kernels run on the SQUARE-ROOT images (Hellinger lower
    // bound, see k_knn_rerank_hell): xb = the shadow codebook that owns those images
    p.hell = rq.hell_q != nullptr && metric == ISMHIP_METRIC_CHI2 && cb->chi_shadow;
    const ismhip_codebook* xb = p.hell ? cb->chi_shadow : cb;
    const bool l2 = p.hell || metric == ISMHIP_METRIC_L2SQ;
    // candidate kernel for squared L2: f16 (default), bf16x3 (ISMHIP_KNN_MODE=bf16x3) or the exact-f32 MFMA contraction
    // (ISMHIP_KNN_MODE=f32); the last two are kept for A/B runs and as the reference points of the error model tests
    // short descriptors (FPFH-33: values up to 100, |q||c| ~ 1e4): the f16 error bound is of the order of the neighbour distances, most
    // proofs fail and the exact scan takes over (measured: 135 ms of scan per 524288 queries). The exact-f32 MFMA contraction costs
    // 2 Nq Nc D flop at ~125 TFLOP/s, which for D <= 64 is cheaper than the 16-bit kernels' fixed overheads -- and it proves everything.
    const PcaImage& PI = rq.use_pca == 2 ? cb->pca2 : cb->pca;
    const bool short_dim = cb->dim <= 64 && ctx->knn_mode == 0 && !(rq.use_pca && PI.m > 0);     // (stage 1 of a short-descriptor codebook with an f16 stage-1 image: pca.hip)
    p.mode = !l2 ? -1 : (p.hell ? 0 : (short_dim ? 2 : (ctx->knn_mode == 0 && cb->words_f16 ? 0 : (ctx->knn_mode <= 1 && cb->words_bf16_hi ? 1 : 2))));
    const bool use_lp = p.mode == 0 || p.mode == 1;
    p.big_tile = use_lp && nq >= 4096 && cb->n_words_pad >= 4096;       // 256x256 tile, 8 waves
    // (the ring kernel prefetches four slices ahead and keeps the |c|^2 rows of four tiles: a tile must have at least two slices)
    const bool ring = p.big_tile && p.mode == 0 && xb->words_f16t && (cb->dim + 15) / 16 > 2;
    p.half = ring && (rq.half || ctx->knn_half);                       // 128 x 256 tile, two workgroups per CU (k_knn_l2_ring16<T, 1>)
    // 256 x 256 tile with the whole query panel resident (k_knn_l2_ring16<T, 2, 2>): stage 1 on a rotated image of <= 160 coordinates
    p.qpanel2 = ring && !p.half && ctx->knn_qpanel2 && rq.use_pca && PI.m > 0 && PI.m <= 160 && !rq.ranged;
    // stage 1 of the two-stage search on the rotated, truncated image (pca.hip): same kernel, pca_m / 32 slices instead of dim / 32
    p.pca = rq.use_pca && ring && PI.m > 0;
    p.ring_nk = p.pca ? PI.m / 32 : ((cb->dim + 15) / 16 + 1) / 2;     // 32-k slices per row in the tiled images
    p.merged = rq.many_splits && l2 && use_lp && !p.big_tile;
    p.join = ring && ctx->knn_join;
    p.BM = !l2 ? CHI_B : (p.half ? 128 : (p.big_tile ? 256 : KNN_BM));
    p.BN = !l2 ? CHI_B : (p.big_tile ? 256 : KNN_BN);
    p.slots = ring && !p.half ? 8 : 4;                                 // 16x16x32 MFMA shape: 8 lane slots per query and split
    p.n_qt = (nq + p.BN - 1) / p.BN;
    // The ring kernel's block -> (query tile, split) map: with the split as the SLOW index of an XCD's queue the workgroups resident on
    // the XCD sweep one split, 32 on one joined codeword stream instead of 32 / n_splits on each of n_splits streams, and a codeword
    // tile comes from beyond the L2 once for all of them. Only where the query panel is resident in LDS: the other ring kernels re-read
    // their query tile from the L2 for every codeword tile and want FEW query tiles per XCD, which is what the split as the fast index
    // gives them (measured with the map forced on everywhere, bench configuration 4: stage 1 117.9 -> 118.1 ms, its ranged stage 2 13.27 -> 13.63).
    // Bench launch, two splits: stage 1 23.97 -> 23.23 ms; four splits: 25.51 -> 23.96.
    p.split_major = ctx->knn_split_major >= 0 ? ctx->knn_split_major != 0 : p.qpanel2;
    // (a ranged search plans for its longest range, and keeps a tile for every split of its shortest)
    p.ranged = rq.ranged && l2 && use_lp;
    const int n_mt = (p.ranged ? rq.ranged->rows_max : cb->n_words_pad) / p.BM;
    if (l2) {
        const int max_s = (p.hell ? 64 * KNN_HELL_CPL : 64) / (p.slots * T);
        // at least three codebook splits (two when the candidate slots allow no more): with one, the 32 workgroups of an XCD hold 32
        // different query tiles (6 MB of f16 queries re-read per codeword tile) and fall out of its 4 MB L2; two splits halve that
        // working set (measured 21.0 -> 19.9 ms at 262144 queries), three cost the same time as two and fetch a fifth less from
        // beyond the L2 (joined streams); four are 1.5 % slower
        // (stage 1 on the rotated image: two -- with 4-6 slices per tile the epilogue is a larger share of the kernel, and every split
        // is another eight candidate lists per query to fill: 29.8 -> 28.1 ms per bench launch)
        int want = std::max(p.pca ? 2 : 3, (1024 + p.n_qt - 1) / p.n_qt);
        // (... on the split-major map (above): FOUR wherever filling the chip asks for more than two. A proof fails per split, so stage 2
        // searches a quarter of the rows per failed entry and fewer queries fail at all. 114-object shard of the bench, 454 query
        // tiles, ms per step: three splits 6.91 / 6.97, four 6.87 / 6.85, two 7.78 / 7.71. Not the full launch of 3 632 query tiles: two
        // splits 44.56 / 44.57, three 44.94 / 44.78, four 44.62 / 44.51 -- stage 2 and the scan give back 0.85 ms, the second set of
        // workgroup prologues, candidate lists and re-rank candidates takes 0.85: it stays at two. DESIGN §5 "Stage 1 on four splits")
        if (p.pca && p.split_major && want > 2) want = 4;
        p.n_splits = std::max(1, std::min(std::min(max_s, n_mt), want));
        // ... as long as a workgroup still has a few dozen tiles to amortise its prologue over (10 k-word codebook, 40 tiles: 1 / 2 / 3
        // splits = 3.81 / 4.18 / 4.51 ms) and the launch fills the chip without them
        if (p.big_tile && p.n_qt >= 512) p.n_splits = std::min(p.n_splits, std::max(1, n_mt / 32));
        // Hellinger candidates for chi-square: as many splits as the candidate slots allow (up to eight, at least four tiles each) --
        // the bound of a proof has to lie beyond EVERY row whose Hellinger distance is below the best chi-square value, and
        // those are dozens to hundreds (CSHOT-1344, 10 k words, measured: median 28, 90th percentile 131, 99th 352)
        if (p.hell) p.n_splits = std::max(1, std::min(std::min(max_s, 8), n_mt / 4));
        if (ctx->knn_splits > 0) p.n_splits = std::max(1, std::min(std::min(max_s, n_mt), ctx->knn_splits));
        // few queries (stage 2 of the two-stage search): cut the codebook into as many splits as it takes to fill the chip; the
        // candidates of all splits are then folded into one slot of KNN_MERGE_KEEP by k_knn_merge_splits
        if (p.merged) p.n_splits = std::max(1, std::min(n_mt, (1024 + 8 * ((p.n_qt + 7) / 8) - 1) / (8 * ((p.n_qt + 7) / 8))));
        p.cand_per_split = p.slots * T;
    } else {
        const int max_s = 64 / T;
        p.n_splits = std::max(1, std::min(std::min(max_s, n_mt), (2048 + p.n_qt - 1) / p.n_qt));
        if (k > T) p.n_splits = std::max(p.n_splits, std::min(std::min(max_s, n_mt), (2 * k + T - 1) / T));    // at least 2k candidates to re-rank
        p.cand_per_split = T;
    }
    if (p.ranged) p.n_splits = std::max(1, std::min(p.n_splits, rq.ranged->rows_min / p.BM));
    p.tiles_per_split = (n_mt + p.n_splits - 1) / p.n_splits;
    if (!p.ranged) p.n_splits = (n_mt + p.tiles_per_split - 1) / p.tiles_per_split;      // (a range is dealt evenly: knn_range_split)
    p.n_cand = p.n_splits * p.cand_per_split;
    p.n_bound = l2 ? p.n_splits * p.slots : p.n_splits;
    // sampling pre-pass (stage 1 of the two-stage search on the 256 x 256 kernel, codebooks of >= 128 tiles): the best score
    // every query meets in every 16th codeword tile becomes the start threshold of all its lane slots (see the kernel)
    // (not for an untruncated stage-1 image: with nothing left out there is no scale to relax the start value by, and the
    // unrelaxed best of the sample is the nearest neighbour itself too often)
    p.prepass = rq.stage1 && ring && !p.half && ctx->knn_prepass && n_mt >= 128 && !(p.pca && PI.resid2 <= 0.f);
    p.seeded = rq.seed_dk && ring && !p.prepass;
    p.fb_tiles_per_split = p.merged ? n_mt : p.tiles_per_split;
    p.fb_layout = p.merged ? KNN_FB_ALL : (p.half ? KNN_FB_RING_HALF : (ring ? KNN_FB_RING : (p.big_tile ? KNN_FB_TILE256 : KNN_FB_TILE128)));
    p.threads = 256;
    if (!l2) p.cand = KNN_CAND_CHI2;
    else if (!use_lp) p.cand = KNN_CAND_F32;
    else if (ring) {
        p.cand = KNN_CAND_RING16;
        p.threads = p.half ? 256 : 512;
        if (p.half) { p.kern = knn_ring16_kernel(T, 1, 0, 0, p.ranged); p.lds = p.lds_cap = Ring16Lds<1, 0>::total(0); }
        else if (p.qpanel2) { p.kern = knn_ring16_kernel(T, 2, 2); p.lds = Ring16Lds<2, 2>::total(p.ring_nk); p.lds_cap = Ring16Lds<2, 2>::total(160 / 32); }
        else { p.kern = knn_ring16_kernel(T, 2, 0, 0, p.ranged); p.lds = p.lds_cap = Ring16Lds<2, 0>::total(0); }
    } else {
        p.cand = KNN_CAND_MFMA16;
        p.threads = p.big_tile ? 512 : 256;
        p.kern = knn_mfma16_kernel(T, p.mode, p.big_tile);
        p.lds = p.lds_cap = knn_mfma16_lds(p.BM, p.BN, p.mode == 1 ? 32 : 64, p.mode == 1 ? 3 : 1);
    }
    return p;
}

int run_knn(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, int k, int T, int32_t* idx_out, float* dist_out, const KnnRequest& rq) {
    if (cb->dim_pad / 16 > KNN_FB_MAXJ) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn: descriptor longer than 1344 not built");
    KnnRun r{};
    r.ctx = ctx; r.cb = cb; r.rq = &rq; r.metric = metric; r.nq = nq; r.k = k; r.T = T;
    r.p = knn_plan(ctx, cb, metric, nq, k, T, rq);
    if (r.p.cand == KNN_CAND_MFMA16 && !r.p.kern) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn: f16 256x256 tile without the ring not built");
    if (r.p.cand == KNN_CAND_RING16 && !r.p.kern) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn: ranged ring instance not built for this T");
    r.xb = r.p.hell ? cb->chi_shadow : cb;
    r.PI = rq.use_pca == 2 ? &cb->pca2 : &cb->pca;
    r.qq = q; r.ldq = rq.q_ld ? rq.q_ld : cb->dim;
    if (cb->dim_pad != r.ldq) {
        float* qpad = (float*)ism_scratch(ctx, SCR_QPAD, (size_t)nq * cb->dim_pad * sizeof(float));
        if (!qpad) return ISMHIP_ERR_NOMEM;
        const size_t tot = (size_t)nq * cb->dim_pad;
        hipLaunchKernelGGL(k_pad_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, q, nq, cb->dim, qpad, cb->dim_pad);
        ISM_CHECK_LAUNCH(ctx, "k_pad_rows");
        r.qq = qpad; r.ldq = cb->dim_pad;
    }
    int rc = knn_carve_scratch(r);
    if (rc == ISMHIP_OK) rc = knn_query_images(r);
    if (rc == ISMHIP_OK) rc = knn_launch_candidates(r);
    if (rc == ISMHIP_OK) rc = knn_rerank_prove(r, idx_out, dist_out);
    if (rc != ISMHIP_OK) return rc;
    if (rq.stage1) { *rq.stage1 = KnnStage1{r.queue, r.p.n_splits, r.p.slots, r.p.tiles_per_split * r.p.BM}; return ISMHIP_OK; }
    if (rq.ranged) { rq.ranged->queue->desc[rq.ranged->chunk] = knn_fb_desc(r.p, cb); return ISMHIP_OK; }      // the caller scans the queue once, after its last search
    r.queue.desc[0] = knn_fb_desc(r.p, cb);
    rc = knn_scan_queue(ctx, cb, metric, k, r.qq, r.ldq, r.queue, nullptr, idx_out, dist_out);
    if (rc != ISMHIP_OK) return rc;
    if (ctx->timers_on) ISM_HIP(ctx, hipMemcpyAsync(ctx->knn_stats, r.counters, 8, hipMemcpyDeviceToHost, ctx->stream));   // read back after a sync
    return ISMHIP_OK;
}

int knn_sqrt_queries(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, float* sq, bool& negative) {
    uint32_t* flag = (uint32_t*)(sq + (size_t)nq * cb->dim_pad);
    ISM_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
    const size_t tot = (size_t)nq * cb->dim_pad;
    hipLaunchKernelGGL(k_sqrt_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, q, nq, cb->dim, cb->dim, cb->dim_pad, sq, flag);
    ISM_CHECK_LAUNCH(ctx, "k_sqrt_rows");
    uint32_t neg = 0;
    ISM_HIP(ctx, hipMemcpyAsync(&neg, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    negative = neg != 0;
    return ISMHIP_OK;
}

int knn_f16_emit_image(ismhip_ctx* ctx, const ismhip_codebook* cb, const ismhip_codebook* xb, const float* qv, int n, int ldv, int n_pad,
                       uint32_t* sc, u16* qimg) {
    hipLaunchKernelGGL(k_absmax, dim3(512), dim3(256), 0, ctx->stream, qv, n, cb->dim, ldv, sc);
    ISM_CHECK_LAUNCH(ctx, "k_absmax");
    const size_t tot = (size_t)n_pad * cb->ld16;
    hipLaunchKernelGGL(k_to_f16, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, qv, n, cb->dim, ldv, n_pad, cb->ld16, sc, xb->f16_scale, qimg);
    ISM_CHECK_LAUNCH(ctx, "k_to_f16");
    return ISMHIP_OK;
}

// bf16 hi/lo and scaled-f16 images of the codebook for k_knn_l2_mfma16 (called once from ismhip_codebook_create)
int ism_codebook_split_bf16(ismhip_ctx* ctx, ismhip_codebook* cb, uint32_t absmax_bits) {
    cb->ld16 = (cb->dim + 63) / 64 * 64;
    const size_t tot = (size_t)cb->n_words_pad * cb->ld16;
    if (hipMalloc((void**)&cb->words_bf16_hi, tot * 3 * sizeof(u16) + 16) != hipSuccess) return ism_set_err(ctx, ISMHIP_ERR_NOMEM, "codebook bf16/f16 images");
    cb->words_bf16_lo = cb->words_bf16_hi + tot;
    cb->words_f16 = cb->words_bf16_lo + tot;
    uint32_t* sc = (uint32_t*)(cb->words_f16 + tot);
    hipLaunchKernelGGL(k_split_bf16, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, cb->words, cb->n_words_pad, cb->dim_pad, cb->dim_pad,
                       cb->n_words_pad, cb->ld16, cb->words_bf16_hi, cb->words_bf16_lo);
    ISM_CHECK_LAUNCH(ctx, "k_split_bf16");
    cb->f16_scale = f16_scale_for(absmax_bits);
    ISM_HIP(ctx, hipMemcpyAsync(sc, &absmax_bits, 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_to_f16, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, cb->words, cb->n_words_pad, cb->dim_pad, cb->dim_pad,
                       cb->n_words_pad, cb->ld16, sc, 1.0f, cb->words_f16);
    ISM_CHECK_LAUNCH(ctx, "k_to_f16");
    {
        const int nk = ((cb->dim + 15) / 16 + 1) / 2, n_tiles = cb->n_words_pad / F16T_ROWS;
        const size_t tt = f16t_halves(n_tiles, nk);
        if (hipMalloc((void**)&cb->words_f16t, tt * sizeof(u16)) != hipSuccess) return ism_set_err(ctx, ISMHIP_ERR_NOMEM, "codebook tiled f16 image");
        hipLaunchKernelGGL(k_to_f16_tiled, dim3((unsigned)((tt + 255) / 256)), dim3(256), 0, ctx->stream, cb->words, cb->n_words_pad, cb->dim_pad, cb->dim_pad,
                           n_tiles, nk, sc, 1.0f, cb->words_f16t);
        ISM_CHECK_LAUNCH(ctx, "k_to_f16_tiled");
    }
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));       // absmax_bits is a stack variable of the caller's frame
    return ISMHIP_OK;
}

extern "C" {

int ismhip_knn(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, int k,
               int32_t* idx_out, float* dist_out) {
    if (!ctx || !cb || !q || !idx_out || !dist_out || nq < 0 || k <= 0 || (metric != ISMHIP_METRIC_L2SQ && metric != ISMHIP_METRIC_CHI2))
        return ism_set_err(ctx, ISMHIP_ERR_INVALID, "knn: bad argument");
    // k <= 4 is what the candidate slots (T <= 4 per slot) are sized for. Up to KNN_MAX_K the same kernels serve: the re-rank takes
    // the k best of the <= 64 candidates, the proof asks every slot's dropped-score bound to clear the k-th exact distance -- which
    // fails whenever one slot held more than T of the true k best -- and the exact scan of those slots finishes the query.
    if (k > KNN_MAX_K) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn: k > 16 not built");
    if (nq == 0) return ISMHIP_OK;
    TimerScope ts(ctx, "knn");
    // rows of 1345 .. ISMHIP_KNN_MAX_DIM floats (USC): the exact scan of knn_wide.hip, which needs none of the images
    if (cb->dim_pad / 16 > KNN_FB_MAXJ) return run_knn_wide(ctx, cb, metric, nq, q, k, idx_out, dist_out);
    // T = candidates kept per slot. The bf16x3 candidate scores carry a larger error bound, so more are kept (T = 4): the proof
    // then compares against the 5th best of every slot and almost never fails.
    // (short descriptors take the exact-f32 contraction, whose scores are as good as exact: two candidates per slot are plenty)
    const bool wide = k > 2 || (metric == ISMHIP_METRIC_L2SQ && cb->words_bf16_hi && ctx->knn_mode <= 1 && !(cb->dim <= 64 && ctx->knn_mode == 0));
    // default for big squared-L2 launches with k <= 2 (every shipped configuration): the two-stage search (see run_knn_two_stage)
    if (metric == ISMHIP_METRIC_L2SQ && k <= 2 && ctx->knn_t == 0 && ctx->knn_mode == 0 && ctx->knn_two_stage && cb->words_f16t && nq >= 4096 &&
        cb->n_words_pad >= 4096 && (cb->dim > 64 || cb->pca.m > 0))
        return run_knn_two_stage(ctx, cb, nq, q, k, idx_out, dist_out);
    // chi-square on histogram data: Hellinger candidates on the matrix cores (run_knn_chi2_hellinger); a batch with a negative element
    // keeps the VALU kernel
    if (metric == ISMHIP_METRIC_CHI2 && cb->chi_shadow && ctx->knn_hellinger && knn_matrix_gate(ctx, cb, nq)) {
        bool taken = false;
        const int rc = run_knn_chi2_hellinger(ctx, cb, nq, q, k, idx_out, dist_out, taken);
        if (rc != ISMHIP_OK || taken) return rc;
    }
    const bool forced = ctx->knn_t >= 1 && ctx->knn_t <= 3 && k <= ctx->knn_t;      // ISMHIP_KNN_T, where it can hold k neighbours
    return run_knn(ctx, cb, metric, nq, q, k, forced ? ctx->knn_t : (wide ? 4 : 2), idx_out, dist_out);
}

int ismhip_knn_ratio(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q,
                     float ratio_threshold, int32_t* idx_out, float* dist_out) {
    if (!ctx || !cb || !q || !idx_out || !dist_out || nq < 0) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "knn_ratio: bad argument");
    if (nq == 0) return ISMHIP_OK;
    int32_t* idx2 = (int32_t*)ism_scratch(ctx, SCR_QNORM, (size_t)nq * 2 * (sizeof(int32_t) + sizeof(float)));
    if (!idx2) return ISMHIP_ERR_NOMEM;
    float* d2 = (float*)(idx2 + (size_t)nq * 2);
    int rc = ismhip_knn(ctx, cb, metric, nq, q, 2, idx2, d2);
    if (rc != ISMHIP_OK) return rc;
    hipLaunchKernelGGL(k_ratio, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, nq, ratio_threshold, idx2, d2, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_ratio");
    return ISMHIP_OK;
}

int ismhip_knn_rule(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q,
                    float ratio_threshold, int32_t* idx_out, float* dist_out) {
    if (!ctx || !cb || !q || !idx_out || !dist_out || nq < 0) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "knn_rule: bad argument");
    if (nq == 0) return ISMHIP_OK;
    int32_t* idx3 = (int32_t*)ism_scratch(ctx, SCR_QNORM, (size_t)nq * 3 * (sizeof(int32_t) + sizeof(float)));
    if (!idx3) return ISMHIP_ERR_NOMEM;
    float* d3 = (float*)(idx3 + (size_t)nq * 3);
    int rc = ismhip_knn(ctx, cb, metric, nq, q, 3, idx3, d3);
    if (rc != ISMHIP_OK) return rc;
    hipLaunchKernelGGL(k_rule, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, nq, ratio_threshold, idx3, d3, cb->word_class, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_rule");
    return ISMHIP_OK;
}

}  // extern "C"

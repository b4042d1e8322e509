// knn.hip — exact k-nearest-codeword search (codebook activation).
// Reference seam: ActivationStrategyKNN::activateKNN (activation_strategy/activation_strategy_knn.h:41-126) with
// FLANNExactMatch semantics (flann::SearchParams(-1)); distance functors utils/distance.h:45,65 (FLANN L2 = squared
// Euclidean, ChiSquareDistance), SURVEY Appendix A.6.
//
// Three stages, one unit per stage and heavy kernel family; every kernel is defined in the unit that launches it,
// and the units call each other through the host functions declared in knn_internal.h:
//  1. candidate generation (the dominant kernel of the whole path). Score(c,q) = |c|^2 - 2 c.q as a dense [codewords x queries]
//     contraction on the matrix cores; codewords are the MFMA ROWS and queries the COLUMNS, so a lane holds 16 codeword scores of
//     ONE query per accumulator tile: the running top-T per query lives in registers with no cross-lane traffic and the Nq x Nc
//     matrix is never materialised. Every kernel keeps, per lane slot, the T best candidates AND the value of the best candidate
//     it dropped (the slot's bound).
//       knn_ring16.hip   k_knn_l2_ring16  f16 MFMA, 256x256 tile, LDS-DMA ring         default for launches >= 4096 queries x 4096 codewords
//                                         (its tile epilogue: a scan that leaves the maximum of every 4-row group, one branch per tile, a walk of
//                                         the flagged columns that starts from those maxima, thresholds swapped and published only where a
//                                         wave inserted: knn_ring16.hip, DESIGN.md §4.1 "Hit path")
//       knn_mfma16.hip   k_knn_l2_mfma16  f16 (or bf16x3) MFMA, register-staged tiles  smaller launches; ISMHIP_KNN_MODE=bf16x3 for A/B runs;
//                                                                                      its EMIT variant lists rows below a per-query score
//       knn_cand.hip     k_knn_l2_mfma    f32 MFMA (exact fma chain)                   ISMHIP_KNN_MODE=f32: the independent route used by the tests
//                        k_knn_chi2       VALU 64x64 tile, v_rcp_f32                   chi-square is not a contraction
//  2. this file: the query / codebook images the candidate kernels read (k_split_bf16, k_absmax, k_to_f16, k_to_f16_tiled,
//     k_scale_norms, k_pad_rows, k_sqrt_rows; the f16 scale rule and the tiled layout are defined in knn_internal.h), knn_plan /
//     run_knn, and k_knn_rerank (_pca, _hell) — one wave per query: candidates that can still matter are recomputed with the FLANN
//     functor's own summation order (bit-identical to the CPU functor), the k smallest (distance, row) pairs are selected (ties:
//     lowest row), and the result is PROVEN slot by slot from the slot bounds and a rigorous bound of the candidate kernel's error;
//     a (query, slot) pair that cannot be proven is queued for
//  3. k_knn_fallback / k_knn_fallback_merge — exact scan of the queued slots' rows. Rare for descriptor data, the rule for
//     adversarial inputs (un-normalised magnitudes, hundreds of near-duplicates): it keeps the answer exact in every case.
//  The three re-rank kernels differ in how they pick the candidates to evaluate and in their proof; what they share is written once
//  (knn_load_cand, knn_select_write, knn_queue_unproven here; wave_norm2, knn_eps_s_raw in knn_internal.h). run_knn is the phases in
//  that order on one stream: knn_carve_scratch, knn_query_images, knn_launch_candidates, knn_rerank_prove, knn_exact_scan.
//  Also here: the two-stage and the Hellinger (chi-square) drivers, ismhip_knn, _ratio, _rule. Stage 2 of the two-stage search is
//  SEEDED: k_knn_seed_thr turns the k-th exact value stage 1 found for a query into the start threshold of all its lane slots (the
//  slot proofs it inverts are written once, in knn_internal.h: knn_l2_slot_proven, pca_lb_of / pca_slot_proven), and it searches a
//  query again only on the rows of the stage-1 splits whose proof failed (run_knn_stage2_lists: per-split failure lists, ranged
//  searches, one exact scan, stage 1's answer merged with the list results).
//       knn_threshold.hip  ismhip_knn_threshold  radius search: EMIT sweep + k_thr_* 
//       knn_large_k.hip    ismhip_knn_large_k    any K up to 1024: seeded EMIT sweep + certificate, exact top-K scan
#include "knn_internal.h"

int ism_pca_rotate_queries(ismhip_ctx* ctx, const ismhip_codebook* cb, const PcaImage* P, const float* q, int nq, int ldq, unsigned short* dst);   // pca.hip

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

// ---------------------------------------------------------------------------------------------
// exact re-rank with the FLANN functors' summation order
// ---------------------------------------------------------------------------------------------
// Folds the candidates of MANY codebook splits into one slot. A wave per query keeps the KNN_MERGE_KEEP smallest approximate
// scores of all splits' candidates; the merged bound is the smallest score anything dropped: every split slot's own bound and the
// best candidate this merge leaves out. (A NaN bound stays NaN, so that the proof fails and the query takes the exact scan.)
#define KNN_MERGE_KEEP 16
__device__ __forceinline__ unsigned knn_sortable(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__global__ __launch_bounds__(256) void k_knn_merge_splits(int nq, const float* __restrict__ cand_val, const int* __restrict__ cand_idx, int n_cand,
                                                          const float* __restrict__ cand_bound, int n_bound,
                                                          float* __restrict__ out_val, int* __restrict__ out_idx, float* __restrict__ out_bound) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const int lane = lane_id();
    const float* v = cand_val + (size_t)qi * n_cand; const int* id = cand_idx + (size_t)qi * n_cand;
    unsigned long long prev = 0ull;                                    // keys are > 0: bit 63 or the complement of a negative float
    bool first = true;
    float dropped = __builtin_inff();
    for (int r = 0; r <= KNN_MERGE_KEEP; ++r) {
        unsigned long long best = ~0ull;
        for (int i = lane; i < n_cand; i += 64) {
            if (id[i] < 0) continue;                                   // empty slot entry
            const unsigned long long key = ((unsigned long long)knn_sortable(v[i]) << 32) | (unsigned)i;
            if ((first || key > prev) && key < best) best = key;
        }
        best = wave_min_u64(best);
        if (r < KNN_MERGE_KEEP) {
            if (lane == 0) {
                const bool have = best != ~0ull;
                const int i = have ? (int)(best & 0xffffffffull) : 0;
                out_val[(size_t)qi * KNN_MERGE_KEEP + r] = have ? v[i] : __builtin_inff();
                out_idx[(size_t)qi * KNN_MERGE_KEEP + r] = have ? id[i] : -1;
            }
        } else if (best != ~0ull) dropped = v[(int)(best & 0xffffffffull)];
        if (best == ~0ull) { for (int rr = r + 1; rr < KNN_MERGE_KEEP; ++rr) if (lane == 0) { out_val[(size_t)qi * KNN_MERGE_KEEP + rr] = __builtin_inff(); out_idx[(size_t)qi * KNN_MERGE_KEEP + rr] = -1; } break; }
        prev = best; first = false;
    }
    float b = dropped;
    for (int i = lane; i < n_bound; i += 64) { const float x = cand_bound[(size_t)qi * n_bound + i]; if (x < b || x != x) b = x; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float x = __shfl_xor(b, o, 64); if (x < b || x != x) b = x; }
    if (lane == 0) out_bound[qi] = b;
}

#define KNN_HELL_CPL 4            // candidates per lane of k_knn_rerank_hell (256 per query)

#include "functor.h"

// The 16-word counter block at the head of the queue scratch (flag_count of the kernels), zeroed before every search:
enum KnnCounter {
    KNN_CNT_QUERIES = 0, KNN_CNT_ITEMS = 1,   // the queue: unproven queries, their (query, slot) work items (ctx->knn_stats reads both)
    KNN_CNT_QSC = 4,                          // f16 mode, three words: absmax bits of the query batch, -2 / (s_q s_c), 2^-14 / s_q (k_to_f16)
    KNN_CNT_NEGATIVE = 12,                    // chi-square: some query element is negative (k_any_negative)
    KNN_CNT_WORDS = 16
};
// Slot -> rows layout of the exact scan, chosen by knn_plan and decoded by k_knn_fallback (its wr_rows). The two positive values ARE
// the rows per wave-row block of the 32x32 MFMA tile (MI * 32): 64 on the 128-row tile, 128 on the 256-row tile.
enum KnnFbLayout { KNN_FB_TILE128 = 64, KNN_FB_TILE256 = 128, KNN_FB_RING = -1, KNN_FB_ALL = -2, KNN_FB_RING_HALF = -3 };

// ---- steps the three re-rank kernels share (one wave per query, one candidate / bound slot per lane) ------------------------------
// candidate j of query qi: its row and approximate score, or -1 and +inf (j beyond the list, empty entry, row out of range)
__device__ __forceinline__ int knn_load_cand(const int* __restrict__ cand_idx, const float* __restrict__ cand_val, int qi, int cand_stride,
                                             int j, int n_cand, int n_words, float& av) {
    int id = -1; av = __builtin_inff();
    if (j < n_cand) { id = cand_idx[(size_t)qi * cand_stride + j]; av = cand_val[(size_t)qi * cand_stride + j]; }
    if (!(id >= 0 && id < n_words)) { id = -1; av = __builtin_inff(); }
    return id;
}
// The k smallest of the wave's keys (CPL per lane; ~0 = none; distances are >= 0 or NaN: positive float bit patterns order like
// unsigned integers, ties go to the lowest row) become the query's result, -1 / NaN where the keys ran short (k_knn_fallback_merge
// ends the same way on its private lists). Returns whether there were k; dk = the k-th distance.
template <int CPL>
__device__ __forceinline__ bool knn_select_write(unsigned long long* key, int qi, int k, int lane, int32_t* __restrict__ idx_out, float* __restrict__ dist_out, float& dk) {
    bool have_k = true;
    dk = 0.f;
    for (int j = 0; j < k; ++j) {
        unsigned long long lm = key[0];
#pragma unroll
        for (int c = 1; c < CPL; ++c) lm = key[c] < lm ? key[c] : lm;
        const unsigned long long mn = wave_min_u64(lm);
        if (lane == 0) {
            if (mn == ~0ull) { idx_out[(size_t)qi * k + j] = -1; dist_out[(size_t)qi * k + j] = __builtin_nanf(""); }
            else { idx_out[(size_t)qi * k + j] = (int)(mn & 0xffffffffull); dist_out[(size_t)qi * k + j] = __uint_as_float((unsigned)(mn >> 32)); }
        }
        if (mn == ~0ull) have_k = false; else dk = __uint_as_float((unsigned)(mn >> 32));
#pragma unroll
        for (int c = 0; c < CPL; ++c) if (key[c] == mn) key[c] = ~0ull;       // rows are unique among candidates, so exactly one retires
    }
    return have_k;
}
// Several searches may fill ONE queue (the chunks of a ranged stage 2, scanned together): the queries of this search are numbered from
// q_base in it, and its slots carry slot_tag (chunk << 8), which tells k_knn_fallback whose slot -> rows layout to decode. live !=
// nullptr: query i is padding between two lists when live[i] == ~0u -- it has no answer to find and no record to leave.
// known_dk != nullptr (a ranged search, whose rows need not hold the query's answer): an exact functor value the query's k-th best row
// is KNOWN not to exceed -- stage 1's k-th value, whose rows the caller merges into the result (NaN: none). The proof then asks the
// slots to clear the smaller of it and the k-th value found here: a dropped row beyond that value is beyond the final k-th value.
struct KnnQueueTag { const uint32_t* live; int q_base, slot_tag; const float* known_dk; };
__device__ __forceinline__ bool knn_is_padding(const KnnQueueTag& tg, int qi) { return tg.live && tg.live[qi] == ~0u; }
__device__ __forceinline__ bool knn_proof_dk(const KnnQueueTag& tg, int qi, bool have_k, float& dk) {
    if (tg.known_dk) { const float U = tg.known_dk[qi]; if (U == U) { dk = have_k ? fminf(dk, U) : U; return true; } }
    return have_k;
}
// queue: one record per unproven query {query, first item, #items} and one work item {query, slot} per failing slot
__device__ __forceinline__ void knn_queue_unproven(bool viol, int qi, int lane, uint32_t* __restrict__ flag_count, uint32_t* __restrict__ qrec, uint32_t* __restrict__ items, const KnnQueueTag& tg) {
    const unsigned long long vmask = __ballot(viol);
    if (vmask != 0ull) {
        const int nv = __popcll(vmask);
        uint32_t ibase = 0;
        if (lane == 0) {
            const uint32_t qs = atomicAdd(&flag_count[KNN_CNT_QUERIES], 1u);
            ibase = atomicAdd(&flag_count[KNN_CNT_ITEMS], (uint32_t)nv);
            qrec[3 * (size_t)qs] = (uint32_t)(qi + tg.q_base); qrec[3 * (size_t)qs + 1] = ibase; qrec[3 * (size_t)qs + 2] = (uint32_t)nv;
        }
        ibase = __shfl(ibase, 0, 64);
        if (viol) {
            const uint32_t it = ibase + __popcll(vmask & ((1ull << lane) - 1ull));
            items[2 * (size_t)it] = (uint32_t)(qi + tg.q_base); items[2 * (size_t)it + 1] = (uint32_t)(lane | tg.slot_tag);
        }
    }
}

__global__ __launch_bounds__(256) void k_knn_rerank(const float* __restrict__ words, int dim, int dim_pad, int n_words,
                                                    const float* __restrict__ q, int nq, int ldq, int metric,
                                                    const int* __restrict__ cand_idx, const float* __restrict__ cand_val, int cand_stride, int n_cand,
                                                    const float* __restrict__ cand_bound, int n_bound, VerifyParams vp,
                                                    int k, int32_t* __restrict__ idx_out, float* __restrict__ dist_out,
                                                    uint32_t* __restrict__ flag_count, uint32_t* __restrict__ qrec, uint32_t* __restrict__ items, KnnQueueTag tg) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq || knn_is_padding(tg, qi)) return;
    const int lane = lane_id();
    const float* qp = q + (size_t)qi * ldq;
    const float qn2 = wave_norm2(qp, dim, lane);          // needed by the error bounds below
    // n_cand <= 64 by construction (host): one candidate per lane. Only candidates whose approximate score is within twice the
    // error bound of the k-th best approximate score can be among the exact k best; the others skip the functor.
    float av;
    const int id = knn_load_cand(cand_idx, cand_val, qi, cand_stride, lane, n_cand, n_words, av);
    float kth = av;
    {
        float cur = av;                       // k-th smallest approximate score (k <= 4) by k rounds of wave-min
        for (int j = 0; j < k; ++j) {
            const float mn = wave_min_f(cur);
            kth = mn;
            const unsigned long long eq = __ballot(cur == mn);
            if (eq && lane == __ffsll((long long)eq) - 1) cur = __builtin_inff();      // retire one instance
        }
    }
    float slack;
    if (metric == ISMHIP_METRIC_CHI2) slack = 4.f * (((float)dim_pad + 8.f) * KNN_U + vp.ku) * fabsf(kth);
    else slack = 2.f * knn_eps_s_raw(vp, qn2) + 4.f * vp.ku * (qn2 + fabsf(kth) + vp.cmax2);
    unsigned long long key = ~0ull;
    {
        __shared__ __attribute__((aligned(16))) float s_terms[4][KNN_TERMS];
        float* sT = s_terms[threadIdx.x >> 6];
        unsigned long long need = __ballot(id >= 0 && !(av > kth + slack));     // NaN scores are never skipped
        while (need) {
            const int src = __ffsll((long long)need) - 1; need &= need - 1;
            const int cid = __shfl(id, src, 64);
            const float d = wave_functor(metric, qp, words + (size_t)cid * dim_pad, dim, lane, sT);
            if (lane == src) key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)id;
        }
    }
    // every bound slot (L2: split x 4 lane slots, chi2: split) holds the smallest approximate score that slot dropped
    float bnd = __builtin_inff();
    if (lane < n_bound) bnd = cand_bound[(size_t)qi * n_bound + lane];
    float dk;
    const bool have_k = knn_proof_dk(tg, qi, knn_select_write<1>(&key, qi, k, lane, idx_out, dist_out, dk), dk);
    // Proof of exactness, slot by slot. A codeword dropped by slot b has approximate score >= bnd_b, so
    //   L2  : true distance D >= |q|^2 (1 - 16u) + bnd_b - eps_s,  eps_s = 17u |c|max^2 + (2 dot_rel + 2u) |q||c|max
    //         (|c|^2 by a short tree sum: 16u; K-term fma chain: 1.01 K u on sum|q_i c_i| <= |q||c|; final subtraction: u)
    //   chi2: all terms are non-negative, v_rcp_f32 is 1 ulp: D >= bnd_b (1 - (K + 8) u)
    // and its functor value is >= D (1 - 1.01 K u). If that is above the k-th exact functor value, the slot cannot hold a
    // better row. Slots that fail (or NaNs) are handed to the exact scan, restricted to the rows of those slots.
    // A slot whose bound is still +inf dropped nothing -- unless scores overflowed (+inf / NaN scores are never kept): that needs
    // an inf or NaN in |q|^2, |c|max^2 or their product (or in the f16 scales), all of which make the error bound below non-finite.
    bool viol = false;
    const float eps_chk = metric == ISMHIP_METRIC_CHI2 ? qn2 + vp.cmax2 : knn_eps_s_raw(vp, qn2) + qn2;
    if (lane < n_bound && (bnd != __builtin_inff() || !(eps_chk < __builtin_inff()))) {
        if (!have_k) viol = true;
        else if (metric == ISMHIP_METRIC_CHI2) {
            const float lo = bnd * (1.f - ((float)dim_pad + 8.f) * KNN_U) * (1.f - vp.ku);
            viol = !(dk < lo);
        } else viol = !knn_l2_slot_proven(dk, bnd, qn2, vp);
    }
    knn_queue_unproven(viol, qi, lane, flag_count, qrec, items, tg);
}

// ---- re-rank + proof for a stage 1 that ran on the ROTATED, TRUNCATED image (pca.hip) --------------------------------------------
// The candidate scores are now |c^|^2 - 2 c^.q^ over the m leading rotated coordinates (x^ = the f16 image of fl(R x) / scale): up
// to accumulation error a LOWER bound piece of the functor value, not an approximation of it. With
//   L(s)  = |q^|^2 (1 - 16u) + s - eps_acc                  <= |q^ - c^|^2     (eps_acc as in k_knn_rerank, accumulation terms only)
//   LB(s) = ((sqrt(L) - delta_q - delta_c)+ )^2 / sigma_max(R)^2                <= |q - c|^2   (pca.hip header)
// a row whose score is s has functor value >= LB(s) (1 - ku). Consequences:
//   * candidates are evaluated with the exact functor in ascending order of their score until the next one's LB exceeds the k-th
//     exact value found so far (the others cannot be among the k best, nor tie with them);
//   * a slot whose dropped-score bound b has LB(b) (1 - ku) above the k-th exact value cannot hide a better row: proven.
struct PcaVerify {
    const u16* qimg; int nk;          // rotated f16 query image (tiled), slices per row
    float inv_sq2;                    // 1 / scale^2 of that image
    float inv_sig2, d_rel, dq_abs, dc;   // 1 / sigma_max^2 (rounded down); |x^ - R x| <= d_rel |x| + abs; dc = the codeword side for |c| = |c|max
    float eps_c2, dot2, cmax2;        // eps_acc = eps_c2 + dot2 |q^||c^|max;  cmax2 = max |c^|^2
    float ku;
};
// what LB(s) takes of query qi (row qp, |q|^2 = qn2 by wave_norm2), by the whole wave
__device__ __forceinline__ PcaLb pca_lb_query(const PcaVerify& pv, int qi, float qn2, int lane) {
    float qn2h = 0.f;                                                  // |q^|^2 from the image itself (the halves as stored: any element order)
    for (int i = lane; i < pv.nk * F16T_KB; i += 64) {
        const float v = (float)__builtin_bit_cast(_Float16, pv.qimg[f16t_stored(qi, pv.nk, i)]);
        qn2h += v * v;
    }
    PcaLb b;
    b.qn2h = wave_sum_f(qn2h) * pv.inv_sq2;
    b.dlt = pv.d_rel * (sqrtf(qn2) * 1.00001f) + pv.dq_abs + pv.dc;
    b.eps_s = (pv.eps_c2 + pv.dot2 * sqrtf(b.qn2h * pv.cmax2)) * 1.00001f;
    b.inv_sig2 = pv.inv_sig2;
    return b;
}
__global__ __launch_bounds__(256) void k_knn_rerank_pca(const float* __restrict__ words, int dim, int dim_pad, int n_words,
                                                        const float* __restrict__ q, int nq, int ldq,
                                                        const int* __restrict__ cand_idx, const float* __restrict__ cand_val, int cand_stride, int n_cand,
                                                        const float* __restrict__ cand_bound, int n_bound, PcaVerify pv,
                                                        int k, int32_t* __restrict__ idx_out, float* __restrict__ dist_out,
                                                        uint32_t* __restrict__ flag_count, uint32_t* __restrict__ qrec, uint32_t* __restrict__ items, KnnQueueTag tg) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq || knn_is_padding(tg, qi)) return;
    const int lane = lane_id();
    const float* qp = q + (size_t)qi * ldq;
    const PcaLb lbq = pca_lb_query(pv, qi, wave_norm2(qp, dim, lane), lane);
    float av;
    const int id = knn_load_cand(cand_idx, cand_val, qi, cand_stride, lane, n_cand, n_words, av);
    const float lb = id >= 0 ? pca_lb_of(lbq, av) : __builtin_inff();
    bool done = id < 0;
    unsigned long long key = ~0ull;
    {
        __shared__ __attribute__((aligned(16))) float s_terms[4][KNN_TERMS];
        float* sT = s_terms[threadIdx.x >> 6];
        float kth = __builtin_inff(); int n_eval = 0;
        for (;;) {
            const float cur = done ? __builtin_inff() : lb;
            const float mn = wave_min_f(cur);
            if (!(mn < __builtin_inff())) break;
            if (n_eval >= k && mn * (1.f - pv.ku) > kth) break;        // every remaining candidate is strictly worse than the k-th exact value
            const unsigned long long eq = __ballot(!done && cur == mn);
            const int src = __ffsll((long long)eq) - 1;
            const int cid = __shfl(id, src, 64);
            const float d = wave_functor(ISMHIP_METRIC_L2SQ, qp, words + (size_t)cid * dim_pad, dim, lane, sT);
            if (lane == src) { key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)id; done = true; }
            if (++n_eval >= k) {
                unsigned long long kk = key, m_ = ~0ull;
                for (int j = 0; j < k; ++j) { m_ = wave_min_u64(kk); if (kk == m_) kk = ~0ull; }
                kth = __uint_as_float((unsigned)(m_ >> 32));
            }
        }
    }
    float bnd = __builtin_inff();
    if (lane < n_bound) bnd = cand_bound[(size_t)qi * n_bound + lane];
    float dk;
    const bool have_k = knn_proof_dk(tg, qi, knn_select_write<1>(&key, qi, k, lane, idx_out, dist_out, dk), dk);
    // a slot whose bound is still +inf dropped nothing -- unless scores overflowed, which needs a non-finite |q^|^2 or bound term
    bool viol = false;
    if (lane < n_bound && (bnd != __builtin_inff() || !(lbq.eps_s + lbq.qn2h + lbq.dlt < __builtin_inff()))) {
        if (!have_k) viol = true;
        else viol = !pca_slot_proven(dk, bnd, lbq, pv.ku);
    }
    knn_queue_unproven(viol, qi, lane, flag_count, qrec, items, tg);
}

// ---- start thresholds of a SEEDED search (stage 2 of the two-stage search) -------------------------------------------------------
// Stage 1 has left every stage-2 query an exact functor value U for its k-th best row (seed_dk; NaN: fewer than k rows). Only a row
// that beats or ties U can change the answer, and the proof of this search will ask of every slot bound b exactly
// "U' < LB(b)" with U' <= U the k-th value found here (knn_l2_slot_proven / pca_slot_proven). So every lane slot of the query may
// start from the loosest threshold whose bound already passes that test with dk := U: the rows of stage 1's answer lie below it and
// are kept, nearly everything else never reaches the insertion code, and a slot that does not overflow is proven by construction.
// A closed-form inverse of the bound gives a first guess in score units; it is then moved outwards in steps of about an ulp of the
// bound's largest term until the test itself, evaluated on the value the candidate kernel will report (out_scale * threshold), holds.
// Soundness does not depend on any of this (k_knn_l2_ring16: any start value is sound); a seed that cannot be made to hold -- U not
// finite, an image row that overflowed -- is -inf, the cold start. One wave per query, as in the re-rank kernels: the proof's |q|^2
// sums are the same bits.
__global__ __launch_bounds__(256) void k_knn_seed_thr(const float* __restrict__ q, int nq, int ldq, int dim, const float* __restrict__ seed_dk,
                                                      bool pca, PcaVerify pv, VerifyParams vp, const float* __restrict__ out_scale, float* __restrict__ thr,
                                                      const uint32_t* __restrict__ live /* padding (KnnQueueTag) starts at +inf: it inserts nothing */) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    if (live && live[qi] == ~0u) { if (lane_id() == 0) thr[qi] = __builtin_inff(); return; }
    const int lane = lane_id();
    const float qn2 = wave_norm2(q + (size_t)qi * ldq, dim, lane);
    PcaLb lbq{};
    if (pca) lbq = pca_lb_query(pv, qi, qn2, lane);
    if (lane != 0) return;
    const float U = seed_dk[qi], osc = out_scale[0];
    float t0 = -__builtin_inff();
    if (U >= 0.f && U < __builtin_inff()) {
        float s, step;
        if (pca) {
            // LB(s) (1 - ku) > U  <=  t^2 > U / (inv_sig2 (1 - 8u) (1 - ku)),  sqrt(L) (1 - 4u) - dlt = t,  s = L + eps_s - |q^|^2 (1 - 16u)
            const float t = sqrtf((U + 1e-37f) / (lbq.inv_sig2 * (1.f - 8.f * KNN_U) * (1.f - pv.ku))) * (1.f + 4.f * KNN_U);
            const float rl = (t + lbq.dlt) / (1.f - 4.f * KNN_U);
            s = rl * rl * (1.f + 8.f * KNN_U) + lbq.eps_s - lbq.qn2h * (1.f - 16.f * KNN_U);
            step = 4.f * KNN_U * (lbq.qn2h + fabsf(s) + lbq.eps_s);
        } else {
            s = thr_tau_of(U, qn2, dim, vp);
            step = 4.f * KNN_U * (qn2 + fabsf(s) + vp.cmax2);
        }
        s += step;
        for (int it = 0; it < 24 && s < __builtin_inff(); ++it, s += step, step *= 2.f) {
            const float a = s / osc;                                   // accumulator units; the kernel reports osc * a as the slot's bound
            if (pca ? pca_slot_proven(U, osc * a, lbq, pv.ku) : knn_l2_slot_proven(U, osc * a, qn2, vp)) { t0 = a; break; }
        }
    }
    thr[qi] = t0;
}

// fast chi-square of one row by a whole wave: every lane owns the 16-byte chunks lane, lane + 64, ... of the (zero padded) rows, all
// of a row's loads are issued before the first is used (a dependent load per element made this 10 us per row), tree sum at the end.
// Differs from the functor's sequential sum by at most ~2 ku relative. dim_pad <= 1344 (checked by the caller): <= 6 chunks per lane.
#define CHI_FAST_CH 6
__device__ __forceinline__ void chi2_fast_load_q(const float* __restrict__ qp, int n4, int lane, f32x4* qv) {
#pragma unroll
    for (int j = 0; j < CHI_FAST_CH; ++j) { const int g = lane + 64 * j; qv[j] = g < n4 ? *(const f32x4*)(qp + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f}; }
}
__device__ __forceinline__ float chi2_fast(const f32x4* qv, const float* __restrict__ wp, int n4, int lane) {
    f32x4 wv[CHI_FAST_CH];
#pragma unroll
    for (int j = 0; j < CHI_FAST_CH; ++j) { const int g = lane + 64 * j; wv[j] = g < n4 ? *(const f32x4*)(wp + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f}; }
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < CHI_FAST_CH; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float sm = qv[j][e] + wv[j][e], df = qv[j][e] - wv[j][e]; part += sm > 0.f ? df * df / sm : 0.f; }
    return wave_sum_f(part);
}

// ---- chi-square with candidates from the squared-L2 kernels on the SQUARE-ROOT images (Hellinger lower bound) --------------------
// For non-negative a, b: (a - b)^2 / (a + b) = (sqrt a - sqrt b)^2 (sqrt a + sqrt b)^2 / (a + b) >= (sqrt a - sqrt b)^2, because
// (sqrt a + sqrt b)^2 >= a + b; hence  chi2(q, c) >= H(q, c) = |sqrt q - sqrt c|^2 = |sqrt q|^2 + |sqrt c|^2 - 2 sqrt q . sqrt c:
// a dense contraction, i.e. matrix-core work, where the functor itself (utils/distance.cpp:33-52, a division per element) is not.
// The candidate kernels score |sqrt c|^2 - 2 sqrt c . sqrt q with the error eps_s of the f16 path (VerifyParams, on the sqrt
// vectors), so a row with score s has functor value >= LB(s) (1 - ku), LB(s) = |sqrt q|^2 (1 - 16u) + s - eps_s. As in
// k_knn_rerank_pca the score is a lower bound, not an approximation: candidates are evaluated with the exact functor in ascending
// order of LB until the next one cannot beat the k-th exact value; a slot is proven when LB(its bound) clears that value.
// Only for query batches and codebooks without negative / NaN elements (the caller checks); everything else keeps k_knn_chi2.
__global__ __launch_bounds__(256) void k_knn_rerank_hell(const float* __restrict__ words, int dim, int dim_pad, int n_words,
                                                         const float* __restrict__ q, int nq, int ldq, const float* __restrict__ sq /* sqrt(q), ld dim_pad */,
                                                         const uint32_t* __restrict__ perm /* candidate (shadow) row -> codebook row */,
                                                         const int* __restrict__ cand_idx, const float* __restrict__ cand_val, int cand_stride, int n_cand,
                                                         const float* __restrict__ cand_bound, int n_bound, VerifyParams vp,
                                                         int k, int32_t* __restrict__ idx_out, float* __restrict__ dist_out,
                                                         uint32_t* __restrict__ flag_count, uint32_t* __restrict__ qrec, uint32_t* __restrict__ items, KnnQueueTag tg) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq || knn_is_padding(tg, qi)) return;
    const int lane = lane_id();
    const float* qp = q + (size_t)qi * ldq;
    const float qn2 = wave_norm2(sq + (size_t)qi * dim_pad, dim, lane);   // |sqrt q|^2
    const float eps_s = knn_eps_s(vp, qn2);
    auto lb_of = [&](float s) -> float {
        float L = qn2 * (1.f - 16.f * KNN_U) + s - eps_s;
        L -= 4.f * KNN_U * (qn2 + fabsf(s));
        return L > 0.f ? L : 0.f;                                      // also NaN -> 0
    };
    // up to 256 candidates (the Hellinger bound is loose by up to a factor of two: dozens to hundreds of rows can lie below the
    // best chi-square value, so the candidate stage runs eight codebook splits): KNN_HELL_CPL per lane, +inf = empty / evaluated
    int id[KNN_HELL_CPL]; float lb[KNN_HELL_CPL], fd[KNN_HELL_CPL]; unsigned long long key[KNN_HELL_CPL];
#pragma unroll
    for (int c = 0; c < KNN_HELL_CPL; ++c) {
        float av;
        const int x = knn_load_cand(cand_idx, cand_val, qi, cand_stride, lane + 64 * c, n_cand, n_words, av);
        id[c] = -1; lb[c] = __builtin_inff(); fd[c] = __builtin_inff(); key[c] = ~0ull;
        if (x >= 0) { id[c] = (int)perm[x]; lb[c] = lb_of(av); }
    }
    // Phase 1: a FAST chi-square (lanes sum their elements, wave tree sum) for the candidates in ascending LB order. The functor's own
    // value f (one sequential chain of dim additions, ~5 us per row at 1344 elements) differs from it by at most 3 ku f, so with
    // mg = 4 ku: stop when the next LB exceeds the k-th fast value by (1 + mg); phase 2 then walks the sequential chain only for the
    // rows whose fast value is within (1 + 3 mg) of that k-th value -- nothing else can be among, or tie with, the k best.
    const float mg = 4.f * vp.ku;
    float kth_fast = __builtin_inff();
    {
        // (rows are padded with zeros to dim_pad on the codebook side; the query row is when ldq > dim, else dim is a multiple of 4
        // whenever dim_pad == dim, so whole 16-byte chunks up to dim rounded up to 4 are safe on both sides)
        const int n4 = (ldq >= dim_pad ? dim_pad : dim) >> 2;
        f32x4 qv[CHI_FAST_CH];
        chi2_fast_load_q(qp, n4, lane, qv);
        int n_eval = 0;
        for (;;) {
            float cur = lb[0];
#pragma unroll
            for (int c = 1; c < KNN_HELL_CPL; ++c) cur = fminf(cur, lb[c]);
            const float mn = wave_min_f(cur);
            if (!(mn < __builtin_inff())) break;
            if (n_eval >= k && mn * (1.f - vp.ku) > kth_fast * (1.f + mg)) break;
            const unsigned long long eq = __ballot(cur == mn);
            const int src = __ffsll((long long)eq) - 1;
            int mine = -1, cs = 0;
#pragma unroll
            for (int c = KNN_HELL_CPL - 1; c >= 0; --c) if (lb[c] == mn) { mine = id[c]; cs = c; }
            const int cid = __shfl(mine, src, 64);
            float d = chi2_fast(qv, words + (size_t)cid * dim_pad, n4, lane);
            if (d != d) d = 0.f;                                        // NaN data: keep the row for the exact chain
            if (lane == src) {
#pragma unroll
                for (int c = 0; c < KNN_HELL_CPL; ++c) if (c == cs) { fd[c] = d; lb[c] = __builtin_inff(); }
            }
            if (++n_eval >= k) {
                float ff[KNN_HELL_CPL], m_ = __builtin_inff();
#pragma unroll
                for (int c = 0; c < KNN_HELL_CPL; ++c) ff[c] = fd[c];
                for (int j = 0; j < k; ++j) {
                    float lm = ff[0];
#pragma unroll
                    for (int c = 1; c < KNN_HELL_CPL; ++c) lm = fminf(lm, ff[c]);
                    m_ = wave_min_f(lm);
                    const unsigned long long e2 = __ballot(lm == m_);
                    if (lane == __ffsll((long long)e2) - 1) {            // retire ONE instance
                        bool gone = false;
#pragma unroll
                        for (int c = 0; c < KNN_HELL_CPL; ++c) if (!gone && ff[c] == m_) { ff[c] = __builtin_inff(); gone = true; }
                    }
                }
                kth_fast = m_;
            }
        }
    }
    // Phase 2: the functor's sequential chain for the contenders
    {
        __shared__ __attribute__((aligned(16))) float s_terms[4][KNN_TERMS];
        float* sT = s_terms[threadIdx.x >> 6];
        const float win = kth_fast * (1.f + 3.f * mg);
        for (;;) {
            int mine = -1, cs = 0;
#pragma unroll
            for (int c = KNN_HELL_CPL - 1; c >= 0; --c) if (fd[c] <= win && key[c] == ~0ull && id[c] >= 0) { mine = id[c]; cs = c; }
            const unsigned long long pend = __ballot(mine >= 0);
            if (pend == 0ull) break;
            const int src = __ffsll((long long)pend) - 1;
            const int cid = __shfl(mine, src, 64);
            const float d = wave_functor(ISMHIP_METRIC_CHI2, qp, words + (size_t)cid * dim_pad, dim, lane, sT);
            if (lane == src) {
#pragma unroll
                for (int c = 0; c < KNN_HELL_CPL; ++c) if (c == cs) { key[c] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)id[c]; fd[c] = __builtin_inff(); }
            }
        }
    }
    float bnd = __builtin_inff();
    if (lane < n_bound) bnd = cand_bound[(size_t)qi * n_bound + lane];
    float dk;
    const bool have_k = knn_select_write<KNN_HELL_CPL>(key, qi, k, lane, idx_out, dist_out, dk);
    bool viol = false;
    if (lane < n_bound && (bnd != __builtin_inff() || !(eps_s + qn2 < __builtin_inff()))) {
        if (!have_k) viol = true;
        else viol = !(dk < lb_of(bnd) * (1.f - vp.ku) - 1e-37f);
    }
    knn_queue_unproven(viol, qi, lane, flag_count, qrec, items, tg);
}

// Exact scan for the slots that could not be proven. One WAVE per (query, slot) work item; the wave handles 4 codeword rows
// per step (16 lanes each, 64-byte coalesced segments) with the query held in registers; direct (a-b)^2 [/(a+b)] sums pick
// the rows that can still matter, the FLANN functor order ranks them. Each item leaves its k best (distance,row) keys in
// item_out; k_knn_fallback_merge folds them into the query's result.
// Slot -> rows: L2 bit b = split*4 + wr*2 + h owns, in every tile of its split, the rows wr*wr_rows + x (x < wr_rows) with bit 2
// of x equal to h (the C/D layout of the 32x32 MFMA tile, see the candidate kernels); chi2 bit b = split owns all rows of its split.
#define KNN_FB_UNITS 8192u      // work units (item x row range) when items are few
__host__ __device__ inline uint32_t knn_fb_parts(uint32_t n_items) {
    if (n_items == 0 || n_items > KNN_FB_UNITS / 2) return 1u;
    const uint32_t p = KNN_FB_UNITS / n_items;
    return p > 256u ? 256u : p;
}
// How the slots of ONE search map to rows: its plan's tiles per split, tile count and tile rows, the slot -> rows layout (wr_rows: a
// KnnFbLayout value) and, for a ranged search (qrange, knn_internal.h), the number of splits each query's own range was cut into.
struct KnnFbDesc { int tiles_per_split, n_tiles, tile_rows, wr_rows, n_splits; };
// One launch scans the items of up to two searches that shared a queue: bit 8 of an item's slot word picks d1 (KnnQueueTag).
template <int KM>   // KM = capacity of the per-item result lists: 4 (k <= 4, every shipped configuration) or KNN_MAX_K
__global__ __launch_bounds__(256) void k_knn_fallback(const float* __restrict__ words, int dim, int dim_pad, int n_words,
                                                      const float* __restrict__ q, int ldq, int metric, int k, KnnFbDesc d0, KnnFbDesc d1,
                                                      const int* __restrict__ qrange,
                                                      const uint32_t* __restrict__ flag_count, const uint32_t* __restrict__ items,
                                                      const int32_t* __restrict__ idx_in, const float* __restrict__ dist_in,
                                                      unsigned long long* __restrict__ item_out, size_t part_base) {
    __shared__ __attribute__((aligned(16))) float s_terms[4][KNN_TERMS];
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, l16 = lane & 15;
    const uint32_t n_items = flag_count[KNN_CNT_ITEMS];
    const bool l2 = metric != ISMHIP_METRIC_CHI2;
    const int nj = dim_pad / 16;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    // With few items a wave per item would leave the chip idle behind a handful of long scans: every item is cut into P row
    // ranges (P * n_items <= KNN_FB_UNITS), each range leaves its own k best in part_out and the merge kernel folds them.
    const uint32_t P = knn_fb_parts(n_items);
    unsigned long long* outp = P > 1 ? item_out + KM * part_base : item_out;
    for (uint32_t u = gw; u < n_items * P; u += nw) {
        const uint32_t it = u / P, part_i = u % P;
        const int qi = (int)items[2 * (size_t)it], bt = (int)items[2 * (size_t)it + 1], b = bt & 255;
        const KnnFbDesc d = (bt >> 8) ? d1 : d0;
        const int wr_rows = d.wr_rows, tile_rows = d.tile_rows;
        const bool lay_all = l2 && wr_rows == KNN_FB_ALL;                     // merged splits (k_knn_merge_splits): the one slot owns every row
        const bool lay16 = l2 && wr_rows == KNN_FB_RING;                       // k_knn_l2_ring16: slot b = split*8 + wr*4 + fq owns rows wr*128 + 16 m + 4 fq + j
        const bool lay16h = l2 && wr_rows == KNN_FB_RING_HALF;                      // k_knn_l2_ring16<T, 1>: 128-row tiles, slot b = split*4 + fq owns rows 16 m + 4 fq + j
        const int rows_per_tile = lay_all ? tile_rows : ((lay16 || lay16h) ? 32 : (l2 ? wr_rows / 2 : tile_rows));   // else a lane slot sees half of its wave-row block (bit 2 of the row == h)
        const float* qp = q + (size_t)qi * ldq;
        const int split = lay_all ? 0 : (lay16 ? (b >> 3) : (l2 ? (b >> 2) : b));
        const int wr = lay16h ? 0 : (lay16 ? (b >> 2) & 1 : (b >> 1) & 1), h = b & 1, fq = b & 3;
        int mt0 = split * d.tiles_per_split, mt1 = min(d.n_tiles, mt0 + d.tiles_per_split);
        if (qrange) {                                                          // ranged search: the query's own rows, cut as the candidate kernel cut them
            const int* rg = qrange + 4 * (qi >> 8);
            knn_range_split(rg[0] / tile_rows, rg[1] / tile_rows, split, lay_all ? 1 : d.n_splits, mt0, mt1);
        }
        const int total = (mt1 - mt0) * rows_per_tile;
        unsigned long long best[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j) best[j] = ~0ull;
        float thr = __builtin_inff();
        {
            const int id = idx_in[(size_t)qi * k + (k - 1)];
            if (id >= 0) thr = dist_in[(size_t)qi * k + (k - 1)];
        }
        const int steps = (total + 3) / 4;
        const int e_beg = 4 * (int)((long long)steps * part_i / P), e_end = min(total, 4 * (int)((long long)steps * (part_i + 1) / P));
        for (int e0 = e_beg; e0 < e_end; e0 += 4) {
            const int e = e0 + g;
            int r = n_words;                                  // out of range = idle group
            if (e < e_end) {
                const int tile = mt0 + e / rows_per_tile, y = e % rows_per_tile;
                const int x = lay_all ? y : ((lay16 || lay16h) ? (wr * 128 + ((y >> 2) << 4) + (fq << 2) + (y & 3)) : (l2 ? (wr * wr_rows + (((y >> 2) << 3) | (h << 2) | (y & 3))) : y));
                r = tile * tile_rows + x;
            }
            float part = 0.f;
            if (r < n_words) {
                const float* wp = words + (size_t)r * dim_pad;
                if (!l2) { for (int j = 0; j < nj; ++j) { const int i = l16 + 16 * j; const float a = i < dim ? qp[i] : 0.f, c = wp[i], sm = a + c, df = a - c; part += sm > 0.f ? df * df / sm : 0.f; } }
                else { for (int j = 0; j < nj; ++j) { const int i = l16 + 16 * j; const float df = (i < dim ? qp[i] : 0.f) - wp[i]; part += df * df; } }
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            const bool hit = r < n_words && !(part > thr * 1.0001f + 1e-30f);      // NaN-safe: unordered compares count as hits
            unsigned long long hm = __ballot(hit && l16 == 0);
            while (hm) {                                                             // rare
                const int src = __ffsll((long long)hm) - 1; hm &= hm - 1;
                const int rr = __shfl(r, src, 64);
                const float d = wave_functor(metric, qp, words + (size_t)rr * dim_pad, dim, lane, s_terms[threadIdx.x >> 6]);
                unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)rr;
                if (d != d) key = (0x7fc00000ull << 32) | (unsigned)rr;             // NaN sorts after every finite distance and keeps ITS row
#pragma unroll
                for (int j = 0; j < KM; ++j) if (j < k && key < best[j]) { const unsigned long long tmp = best[j]; best[j] = key; key = tmp; }
                unsigned long long kth = ~0ull;
#pragma unroll
                for (int j = 0; j < KM; ++j) if (j == k - 1) kth = best[j];
                if (kth != ~0ull) thr = fminf(thr, __uint_as_float((unsigned)(kth >> 32)));
            }
        }
#pragma unroll
        for (int j = 0; j < KM; ++j) if (lane == j) outp[KM * (size_t)u + j] = best[j];
    }
}

// one wave per unproven query: the lanes fold the per-unit results (and the re-ranked candidates) into private sorted lists, k
// rounds of a wave-wide minimum then pick the result; a row reached through two paths is taken once
template <int KM>
__global__ __launch_bounds__(256) void k_knn_fallback_merge(int k, const uint32_t* __restrict__ flag_count, const uint32_t* __restrict__ qrec,
                                     const unsigned long long* __restrict__ item_out, size_t part_base, int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const uint32_t n_q = flag_count[KNN_CNT_QUERIES];
    const uint32_t P = knn_fb_parts(flag_count[KNN_CNT_ITEMS]);
    const unsigned long long* outp = P > 1 ? item_out + KM * part_base : item_out;
    const int lane = threadIdx.x & 63;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n_q; t += gridDim.x * 4) {
        const int qi = (int)qrec[3 * (size_t)t]; const uint32_t ibase = qrec[3 * (size_t)t + 1], ni = qrec[3 * (size_t)t + 2];
        unsigned long long fin[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j) fin[j] = ~0ull;
        auto ins = [&](unsigned long long key) {
#pragma unroll
            for (int j = 0; j < KM; ++j) if (fin[j] != ~0ull && (fin[j] & 0xffffffffull) == (key & 0xffffffffull)) return;   // same row twice
#pragma unroll
            for (int j = 0; j < KM; ++j) if (key < fin[j]) { const unsigned long long tmp = fin[j]; fin[j] = key; key = tmp; }
        };
        if (lane < k) {
            const int id = idx_out[(size_t)qi * k + lane];
            if (id >= 0) ins(((unsigned long long)__float_as_uint(dist_out[(size_t)qi * k + lane]) << 32) | (unsigned)id);
        }
        for (uint32_t i = lane; i < ni * P; i += 64)
            for (int j = 0; j < k; ++j) { const unsigned long long key = outp[KM * ((size_t)ibase * P + i) + j]; if (key != ~0ull) ins(key); }
        for (int j = 0; j < k; ++j) {
            const unsigned long long mn = wave_min_u64(fin[0]);
            if (lane == 0) {
                if (mn == ~0ull) { idx_out[(size_t)qi * k + j] = -1; dist_out[(size_t)qi * k + j] = __builtin_nanf(""); }
                else { idx_out[(size_t)qi * k + j] = (int)(mn & 0xffffffffull); dist_out[(size_t)qi * k + j] = __uint_as_float((unsigned)(mn >> 32)); }
            }
            if (mn == ~0ull) continue;
            // drop the chosen row from every private list (it can sit in several lanes, with the same key)
            // (a private list is sorted and holds a row at most once: shift the tail down over the hit)
            bool gone = false;
#pragma unroll
            for (int x = 0; x < KM; ++x) {
                if (!gone && fin[x] != ~0ull && (fin[x] & 0xffffffffull) == (mn & 0xffffffffull)) gone = true;
                if (gone) fin[x] = x + 1 < KM ? fin[x + 1] : ~0ull;
            }
        }
    }
}

__global__ void k_pad_rows(const float* __restrict__ src, int n, int dim, float* __restrict__ dst, int dim_pad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * dim_pad) return;
    const int row = (int)(i / dim_pad), col = (int)(i % dim_pad);
    dst[i] = col < dim ? src[(size_t)row * dim + col] : 0.f;
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

// stage1 != nullptr: FIRST stage of the two-stage search -- candidates + exact re-rank + proof only; the unproven queries are
// left in the queue (*stage1 = {flag_count, qrec, items}) for the caller instead of going to the exact scan; with them, how the
// stage cut the codebook: item slot b belongs to split b / slots, and split s swept the rows [s, s + 1) * rows_per_split.
struct KnnStage1 { uint32_t* flag_count; uint32_t* qrec; uint32_t* items; int n_splits, slots, rows_per_split; };
// A queue of unproven work that several searches fill and ONE exact scan empties (knn_scan_queue): the counter block, records and
// items as in KnnScratch, and the slot -> rows layout each search (chunk 0 / 1) leaves behind for the scan.
struct KnnQueue { uint32_t *count, *qrec, *items; unsigned long long* item_out; size_t q_items; KnnFbDesc desc[2]; };
// what the caller of run_knn asks for beyond the search itself
struct KnnRequest {
    KnnStage1* stage1 = nullptr;
    const char* tname = nullptr;       // timer of the candidate kernel
    bool many_splits = false;          // few queries: as many codebook splits as fill the chip, folded into one slot (k_knn_merge_splits)
    int use_pca = 0;                   // 1: stage-1 image, 2: stage-2 image (pca.hip)
    const float* hell_q = nullptr;     // chi-square only: sqrt(q) rows of dim_pad floats -> Hellinger candidates (k_knn_rerank_hell)
    bool half = false;                 // the 128 x 256 ring tile (k_knn_l2_ring16<T, 1>), as with ISMHIP_KNN_HALF=1
    const float* seed_dk = nullptr;    // per query, an exact functor value its k-th best row is known not to exceed (NaN: none): the ring
                                       // kernel starts from the thresholds k_knn_seed_thr derives from it
    // A RANGED search (knn_internal.h: KnnCandArgs::qrange), chunk `chunk` of the run_knn_stage2_lists driver: the queries are the
    // entries q_base ... of the concatenated failure lists (live[i] == ~0u: padding between two lists), every group of 256 sweeps its
    // own row range (the shortest / longest of them: range_rows_min / _max), and what stays unproven goes to `queue`, not to a scan.
    const int* qrange = nullptr; const uint32_t* live = nullptr; KnnQueue* queue = nullptr;
    int q_base = 0, chunk = 0, range_rows_min = 0, range_rows_max = 0;
    const float* known_dk = nullptr;   // per query, see KnnQueueTag (the ranged search's proofs); seed_dk only sets the start thresholds
    int q_ld = 0;                      // row stride of the queries when they are already padded (dim_pad); 0: dim
};

// How run_knn runs one search. knn_plan decides it from the request, the ctx switches and the codebook, without side effects.
enum KnnCand { KNN_CAND_F32, KNN_CAND_CHI2, KNN_CAND_MFMA16, KNN_CAND_RING16 };
struct KnnPlan {
    bool hell;                  // Hellinger candidates: squared L2 on the sqrt images of the shadow codebook
    int mode;                   // squared-L2 candidates: 0 f16, 1 bf16x3, 2 exact f32; -1 chi-square
    KnnCand cand;
    const void* kern;           // KNN_CAND_MFMA16 / KNN_CAND_RING16: the kernel instance (nullptr: not built)
    int BM, BN, threads;        // codeword rows and queries per tile, threads per workgroup
    bool big_tile, half, qpanel2, pca, merged, prepass, seeded, join, ranged;
    int slots, ring_nk;         // lane slots per codebook split (squared L2), 32-k slices per row of the tiled images
    int n_qt, n_splits, tiles_per_split, cand_per_split, n_cand, n_bound;
    int fb_tiles_per_split; KnnFbLayout fb_layout;   // exact scan: tiles per slot's split and the slot -> rows layout
    size_t lds, lds_cap;        // dynamic LDS of this launch, and the largest any launch of the kernel uses
};

// T = candidates kept per lane slot, 1 .. 4
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
    p.qpanel2 = ring && !p.half && ctx->knn_qpanel2 && rq.use_pca && PI.m > 0 && PI.m <= 160 && !rq.range_rows_max;
    // stage 1 of the two-stage search on the rotated, truncated image (pca.hip): same kernel, pca_m / 32 slices instead of dim / 32
    p.pca = rq.use_pca && ring && PI.m > 0;
    p.ring_nk = p.pca ? PI.m / 32 : ((cb->dim + 15) / 16 + 1) / 2;     // 32-k slices per row in the tiled images
    p.merged = rq.many_splits && l2 && use_lp && !p.big_tile;
    p.join = ring && ctx->knn_join;
    p.BM = !l2 ? CHI_B : (p.half ? 128 : (p.big_tile ? 256 : KNN_BM));
    p.BN = !l2 ? CHI_B : (p.big_tile ? 256 : KNN_BN);
    p.slots = ring && !p.half ? 8 : 4;                                 // 16x16x32 MFMA shape: 8 lane slots per query and split
    p.n_qt = (nq + p.BN - 1) / p.BN;
    // (a ranged search plans for its longest range, and keeps a tile for every split of its shortest)
    p.ranged = rq.range_rows_max > 0 && l2 && use_lp;
    const int n_mt = (p.ranged ? rq.range_rows_max : cb->n_words_pad) / p.BM;
    if (l2) {
        const int max_s = (p.hell ? 64 * KNN_HELL_CPL : 64) / (p.slots * T);
        // at least three codebook splits (two when the candidate slots allow no more): with one, the 32 workgroups of an XCD hold 32
        // different query tiles (6 MB of f16 queries re-read per codeword tile) and fall out of its 4 MB L2; two splits halve that
        // working set (measured 21.0 -> 19.9 ms at 262144 queries), three cost the same time as two and fetch a fifth less from
        // beyond the L2 (joined streams); four are 1.5 % slower
        // (stage 1 on the rotated image: two -- with 4-6 slices per tile the epilogue is a larger share of the kernel, and every split
        // is another eight candidate lists per query to fill: 29.8 -> 28.1 ms per bench launch)
        p.n_splits = std::max(1, std::min(std::min(max_s, n_mt), std::max(p.pca ? 2 : 3, (1024 + p.n_qt - 1) / p.n_qt)));
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
    if (p.ranged) p.n_splits = std::max(1, std::min(p.n_splits, rq.range_rows_min / p.BM));
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

// The carve-up of a search's scratch, filled by knn_carve_scratch.
struct KnnScratch {
    float *cand_val, *cand_bound; int* cand_idx; int n_cand, n_bound;      // candidate lists and slot bounds (after a merge: the folded slot)
    uint32_t *flag_count, *qrec, *items; unsigned long long* item_out; size_t q_items;    // counter block and queue of unproven work
    uint32_t* qcount;                    // the queue's counters: the block's own, or those of the request's shared queue
    uint32_t* qsc;                       // the counter block's f16 scalars
};
// One search in flight: what the phases of run_knn hand to each other.
struct KnnRun : KnnScratch {
    ismhip_ctx* ctx; const ismhip_codebook *cb, *xb; const PcaImage* PI; const KnnRequest* rq; KnnPlan p;
    int metric, nq, k, T;
    const float* qq; int ldq;            // the query rows as the kernels read them (padded to dim_pad when dim is not)
    u16 *q_hi, *q_lo;                    // 16-bit query images (knn_query_images; nullptr: the candidate kernel reads the rows themselves)
};

// queue of unproven work: counters | query records [nq*3] | items [nq*n_bound*2] | item results [nq*n_bound*4] u64
int knn_carve_scratch(KnnRun& r) {
    const KnnPlan& p = r.p; const size_t nq = (size_t)r.nq;
    r.n_cand = p.n_cand; r.n_bound = p.n_bound; r.q_items = nq * p.n_bound;
    r.cand_val = (float*)ism_scratch(r.ctx, SCR_KNN_CAND_VAL, nq * (p.n_cand + p.n_bound + (p.merged ? KNN_MERGE_KEEP + 1 : 0)) * sizeof(float));
    r.cand_idx = (int*)ism_scratch(r.ctx, SCR_KNN_CAND_IDX, nq * (p.n_cand + (p.merged ? KNN_MERGE_KEEP : 0)) * sizeof(int));
    r.flag_count = (uint32_t*)ism_scratch(r.ctx, SCR_KNN_FLAGS, (KNN_CNT_WORDS + 3 * nq + 2 * r.q_items) * sizeof(uint32_t) + 8 + (r.q_items + KNN_FB_UNITS) * (r.k > 4 ? KNN_MAX_K : 4) * sizeof(unsigned long long));
    if (!r.cand_val || !r.cand_idx || !r.flag_count) return ISMHIP_ERR_NOMEM;
    r.cand_bound = r.cand_val + nq * p.n_cand;
    r.qrec = r.flag_count + KNN_CNT_WORDS; r.items = r.qrec + 3 * nq; r.qsc = r.flag_count + KNN_CNT_QSC;
    r.item_out = (unsigned long long*)(((uintptr_t)(r.items + 2 * r.q_items) + 7) & ~(uintptr_t)7);
    ISM_HIP(r.ctx, hipMemsetAsync(r.flag_count, 0, KNN_CNT_WORDS * sizeof(uint32_t), r.ctx->stream));
    r.qcount = r.flag_count;
    if (const KnnQueue* Q = r.rq->queue) { r.qcount = Q->count; r.qrec = Q->qrec; r.items = Q->items; r.item_out = Q->item_out; r.q_items = Q->q_items; }
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
        const int rc = ism_pca_rotate_queries(ctx, cb, r.PI, r.qq, nq, r.ldq, r.q_hi);
        if (rc != ISMHIP_OK) return rc;
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

// the constants of the lower-bound proof on the run's rotated image (k_knn_rerank_pca, k_knn_seed_thr)
PcaVerify knn_pca_verify(const KnnRun& r, const VerifyParams& vp) {
    const PcaImage& PI = *r.PI;
    PcaVerify pv;
    const float acc_rel = 1.01f * (float)PI.m * 1.1920929e-07f;            // accumulation only: products of f16 values are exact in fp32
    pv.qimg = r.q_hi; pv.nk = r.p.ring_nk; pv.inv_sq2 = 1.0f / (PI.sq * PI.sq);
    pv.inv_sig2 = PI.inv_sig2; pv.d_rel = PI.d_rel; pv.dq_abs = PI.dq_abs;
    pv.dc = (PI.d_rel * sqrtf(r.cb->max_norm2) + PI.dc_abs) * 1.00001f;
    pv.cmax2 = PI.cmax2;
    // subnormal f16 operands may be flushed to zero by the matrix cores: |dq_i| <= 2^-14 / sq, |dc_i| <= 2^-14 / sc per element
    const float fq = F16_FLUSH / PI.sq, fc = F16_FLUSH / PI.sc, sm = sqrtf((float)PI.m);
    pv.eps_c2 = (17.f * KNN_U + 1.01f * (float)(PI.m + 1) * 1.1920929e-07f) * PI.cmax2 + 2.02f * (sm * fq * sqrtf(PI.cmax2) + sm * sm * fq * fc);
    pv.dot2 = 2.f * acc_rel + 2.f * KNN_U + 2.02f * sm * fc / sqrtf(PI.cmax2);
    pv.ku = vp.ku;
    return pv;
}

// the candidate kernel of the plan; many splits are then folded into one slot, which becomes the run's candidate list
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
        a.qrange = p.ranged ? r.rq->qrange : nullptr;
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
            if (p.seeded) {                                                  // needs the query image and, on the original image, its scalars
                const VerifyParams vp = knn_verify_params(xb, cb->dim_pad, p.mode, r.qsc, true);
                hipLaunchKernelGGL(k_knn_seed_thr, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, r.qq, nq, r.ldq, cb->dim, r.rq->seed_dk,
                                   p.pca, p.pca ? knn_pca_verify(r, vp) : PcaVerify{}, vp, a.out_scale, thr0, r.rq->live);
                ISM_CHECK_LAUNCH(ctx, "k_knn_seed_thr");
                ++ctx->knn_seed_launches;
            }
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
            rc = knn_chi2_launch(ctx, r.T, p.n_qt, cb, r.qq, nq, r.ldq, r.flag_count + KNN_CNT_NEGATIVE, p.tiles_per_split, p.n_splits, r.cand_val, r.cand_idx, r.n_cand, r.cand_bound, r.n_bound);
        }
        if (rc != ISMHIP_OK) return rc;
    }
    if (p.merged) {
        float* m_val = r.cand_bound + (size_t)nq * r.n_bound; float* m_bound = m_val + (size_t)nq * KNN_MERGE_KEEP;
        int* m_idx = r.cand_idx + (size_t)nq * r.n_cand;
        hipLaunchKernelGGL(k_knn_merge_splits, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, nq, r.cand_val, r.cand_idx, r.n_cand, r.cand_bound, r.n_bound, m_val, m_idx, m_bound);
        ISM_CHECK_LAUNCH(ctx, "k_knn_merge_splits");
        r.cand_val = m_val; r.cand_idx = m_idx; r.cand_bound = m_bound; r.n_cand = KNN_MERGE_KEEP; r.n_bound = 1;
    }
    return ISMHIP_OK;
}

// exact functor values of the candidates that matter, the k best, and the proof; what it cannot prove is queued
int knn_rerank_prove(KnnRun& r, int32_t* idx_out, float* dist_out) {
    ismhip_ctx* ctx = r.ctx; const ismhip_codebook* cb = r.cb; const KnnPlan& p = r.p;
    const VerifyParams vp = knn_verify_params(r.xb, cb->dim_pad, p.mode, r.qsc, true);
    const dim3 grid((r.nq + 3) / 4), block(256);
    const KnnQueueTag tg{r.rq->live, r.rq->q_base, r.rq->chunk << 8, r.rq->known_dk};
    TimerScope trr(ctx, "knn_rerank");
    if (p.pca) {
        const PcaVerify pv = knn_pca_verify(r, vp);
        hipLaunchKernelGGL(k_knn_rerank_pca, grid, block, 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words,
                           r.qq, r.nq, r.ldq, r.cand_idx, r.cand_val, r.n_cand, r.n_cand, r.cand_bound, r.n_bound, pv, r.k, idx_out, dist_out, r.qcount, r.qrec, r.items, tg);
    } else if (p.hell) {
        hipLaunchKernelGGL(k_knn_rerank_hell, grid, block, 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words,
                           r.qq, r.nq, r.ldq, r.rq->hell_q, r.xb->shadow_perm, r.cand_idx, r.cand_val, r.n_cand, r.n_cand, r.cand_bound, r.n_bound, vp, r.k, idx_out, dist_out, r.qcount, r.qrec, r.items, tg);
    } else
    hipLaunchKernelGGL(k_knn_rerank, grid, block, 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words,
                       r.qq, r.nq, r.ldq, r.metric, r.cand_idx, r.cand_val, r.n_cand, r.n_cand, r.cand_bound, r.n_bound, vp, r.k, idx_out, dist_out, r.qcount, r.qrec, r.items, tg);
    ISM_CHECK_LAUNCH(ctx, "k_knn_rerank");
    return ISMHIP_OK;
}

// exact scan of the queued slots' rows, folded into the results of the unproven queries: one scan and one merge launch for a
// queue, whichever searches filled it (q, idx_out, dist_out are indexed by the queue's query numbers)
int knn_scan_queue(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int k, const float* q, int ldq, const KnnQueue& Q, const int* qrange,
                   int32_t* idx_out, float* dist_out) {
    TimerScope ts(ctx, "knn_fallback");
    const auto scan = k <= 4 ? k_knn_fallback<4> : k_knn_fallback<KNN_MAX_K>;      // capacity of the per-item result lists
    const auto merge = k <= 4 ? k_knn_fallback_merge<4> : k_knn_fallback_merge<KNN_MAX_K>;
    hipLaunchKernelGGL(scan, dim3(1024), dim3(256), 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words, q, ldq, metric, k,
                       Q.desc[0], Q.desc[1], qrange, Q.count, Q.items, idx_out, dist_out, Q.item_out, Q.q_items);
    ISM_CHECK_LAUNCH(ctx, "k_knn_fallback");
    hipLaunchKernelGGL(merge, dim3(256), dim3(256), 0, ctx->stream, k, Q.count, Q.qrec, Q.item_out, Q.q_items, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_knn_fallback_merge");
    return ISMHIP_OK;
}
KnnFbDesc knn_fb_desc(const KnnPlan& p, const ismhip_codebook* cb) { return KnnFbDesc{p.fb_tiles_per_split, cb->n_words_pad / p.BM, p.BM, (int)p.fb_layout, p.n_splits}; }
int knn_exact_scan(KnnRun& r, int32_t* idx_out, float* dist_out) {
    KnnQueue Q{r.qcount, r.qrec, r.items, r.item_out, r.q_items, {knn_fb_desc(r.p, r.cb), KnnFbDesc{}}};
    return knn_scan_queue(r.ctx, r.cb, r.metric, r.k, r.qq, r.ldq, Q, nullptr, idx_out, dist_out);
}

int run_knn(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, int k, int T,
            int32_t* idx_out, float* dist_out, const KnnRequest& rq = KnnRequest()) {
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
    if (rq.stage1) { *rq.stage1 = KnnStage1{r.flag_count, r.qrec, r.items, r.p.n_splits, r.p.slots, r.p.tiles_per_split * r.p.BM}; return ISMHIP_OK; }
    if (rq.queue) { rq.queue->desc[rq.chunk] = knn_fb_desc(r.p, cb); return ISMHIP_OK; }      // the caller scans the queue once, after its last search
    rc = knn_exact_scan(r, idx_out, dist_out);
    if (rc != ISMHIP_OK) return rc;
    if (ctx->timers_on) ISM_HIP(ctx, hipMemcpyAsync(ctx->knn_stats, r.flag_count, 8, hipMemcpyDeviceToHost, ctx->stream));   // read back after a sync
    return ISMHIP_OK;
}

// ---- two-stage search -------------------------------------------------------------------------------------------------------
// The top-T bookkeeping in the candidate kernel's epilogue costs time in proportion to T (measured, 262144 queries x 102400
// words: T = 4 18.7 ms, T = 2 16.8 ms, T = 1 16.2 ms), but a small T leaves more queries unproven (T = 2: ~0.1 % of them, T = 1:
// ~3 %), and the exact scan that finishes an unproven query reads its slots' share of the f32 codebook (24 us per query).
// So: stage 1 runs T = 2 over all queries; the few queries its proof rejects are gathered and searched again with T = 4 (a
// launch ~1000x smaller), and only what THAT proof rejects goes to the exact scan. Every answer is still the exact functor
// minimum, proven or scanned.
// (dk2 != nullptr: also the k-th exact value stage 1 found for the query, NaN when it found fewer than k rows)
__global__ __launch_bounds__(256) void k_knn_gather_flagged(const uint32_t* __restrict__ qrec, int n2, const float* __restrict__ q, int dim,
                                                            float* __restrict__ q2, uint32_t* __restrict__ list2,
                                                            const int32_t* __restrict__ idx1, const float* __restrict__ dist1, int k, float* __restrict__ dk2) {
    const int i = blockIdx.x;
    if (i >= n2) return;
    const uint32_t qi = qrec[3 * (size_t)i];
    if (threadIdx.x == 0) {
        list2[i] = qi;
        if (dk2) dk2[i] = idx1[(size_t)qi * k + (k - 1)] >= 0 ? dist1[(size_t)qi * k + (k - 1)] : __builtin_nanf("");
    }
    for (int c = threadIdx.x; c < dim; c += blockDim.x) q2[(size_t)i * dim + c] = q[(size_t)qi * dim + c];
}
__global__ void k_knn_scatter_results(const uint32_t* __restrict__ list2, int n2, int k, const int32_t* __restrict__ idx2, const float* __restrict__ dist2,
                                      int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n2 * k) return;
    const size_t o = (size_t)list2[t / k] * k + (t % k);
    idx_out[o] = idx2[t]; dist_out[o] = dist2[t];
}

// The queries a first stage left unproven (s1), gathered for a second search: n2 of them (read back: the one host round trip of the
// call; n2 == 0: nothing left to do), their rows in q2, their ids in list2, and room for the second stage's results idx2 / dist2,
// which knn_scatter_stage2 writes to the queries' places in the caller's arrays. dk2 = the k-th exact values of stage 1's results
// idx1 / dist1 (the seeds of a seeded second search; nullptr: none wanted).
// want_lists (set by the caller, nq = its query count): the per-split failure lists are made first (k_knn_split_lists: lists_d[s * nq
// ...], head_d = {n2, |list 0|, ...}) and their sizes cnt travel in the same read-back; the caller then runs run_knn_stage2_lists
// or, if that declines, knn_gather_unsplit.
struct KnnStage2 { int n2; float* q2; uint32_t* list2; int32_t* idx2; float* dist2; float* dk2;
                   bool want_lists = false; uint32_t *head_d = nullptr, *lists_d = nullptr; uint32_t cnt[16] = {}; };
int knn_gather_unsplit(ismhip_ctx* ctx, const ismhip_codebook* cb, const KnnStage1& s1, const float* q, int k, KnnStage2& g, const int32_t* idx1, const float* dist1);
__global__ void k_knn_split_lists(const uint32_t* __restrict__ flag_count, const uint32_t* __restrict__ qrec, const uint32_t* __restrict__ items,
                                  int slots, int nq, uint32_t* __restrict__ head, uint32_t* __restrict__ lists);      // with the other kernels of the lists, below
int knn_gather_stage2(ismhip_ctx* ctx, const ismhip_codebook* cb, const KnnStage1& s1, const float* q, int k, KnnStage2& g,
                      const int32_t* idx1, const float* dist1, int nq = 0) {
    uint32_t hb[17] = {0};
    if (g.want_lists) {
        g.head_d = (uint32_t*)ism_scratch(ctx, SCR_KNN_LISTS, (32 + (size_t)s1.n_splits * nq) * sizeof(uint32_t));
        if (!g.head_d) return ISMHIP_ERR_NOMEM;
        g.lists_d = g.head_d + 32;
        ISM_HIP(ctx, hipMemsetAsync(g.head_d, 0, 32 * sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(k_knn_split_lists, dim3(256), dim3(256), 0, ctx->stream, (const uint32_t*)s1.flag_count, (const uint32_t*)s1.qrec, (const uint32_t*)s1.items,
                           s1.slots, nq, g.head_d, g.lists_d);
        ISM_CHECK_LAUNCH(ctx, "k_knn_split_lists");
        ISM_HIP(ctx, hipMemcpyAsync(hb, g.head_d, 17 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    } else ISM_HIP(ctx, hipMemcpyAsync(hb, s1.flag_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->knn_stage2_queries = hb[0];
    for (int s = 0; s < 16; ++s) g.cnt[s] = hb[1 + s];
    ctx->knn_stage2_list_entries = 0;
    for (int s = 0; s < 16; ++s) ctx->knn_stage2_list_entries += g.cnt[s];
    g.n2 = (int)hb[0];
    if (g.n2 == 0) { ctx->knn_stats[0] = ctx->knn_stats[1] = 0; return ISMHIP_OK; }
    if (g.want_lists) return ISMHIP_OK;
    return knn_gather_unsplit(ctx, cb, s1, q, k, g, idx1, dist1);
}
int knn_gather_unsplit(ismhip_ctx* ctx, const ismhip_codebook* cb, const KnnStage1& s1, const float* q, int k, KnnStage2& g, const int32_t* idx1, const float* dist1) {
    const int n2 = g.n2;
    g.q2 = (float*)ism_scratch(ctx, SCR_KNN_Q2, (size_t)n2 * cb->dim * sizeof(float));
    g.list2 = (uint32_t*)ism_scratch(ctx, SCR_KNN_LIST2, (size_t)n2 * (sizeof(uint32_t) + (size_t)k * (sizeof(int32_t) + sizeof(float)) + (idx1 ? sizeof(float) : 0)));
    if (!g.q2 || !g.list2) return ISMHIP_ERR_NOMEM;
    g.idx2 = (int32_t*)(g.list2 + n2);
    g.dist2 = (float*)(g.idx2 + (size_t)n2 * k);
    g.dk2 = idx1 ? g.dist2 + (size_t)n2 * k : nullptr;
    hipLaunchKernelGGL(k_knn_gather_flagged, dim3(n2), dim3(256), 0, ctx->stream, s1.qrec, n2, q, cb->dim, g.q2, g.list2, idx1, dist1, k, g.dk2);
    ISM_CHECK_LAUNCH(ctx, "k_knn_gather_flagged");
    return ISMHIP_OK;
}
int knn_scatter_stage2(ismhip_ctx* ctx, const KnnStage2& g, int k, int32_t* idx_out, float* dist_out) {
    hipLaunchKernelGGL(k_knn_scatter_results, dim3((g.n2 * k + 255) / 256), dim3(256), 0, ctx->stream, g.list2, g.n2, k, g.idx2, g.dist2, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_knn_scatter_results");
    return ISMHIP_OK;
}

// ---- stage 2 on per-split failure lists ---------------------------------------------------------------------------------------------
// Stage 1 proves a query split by split: all the slots of one split report the same bound, so a query whose proof failed has failed
// it in some of stage 1's codebook splits and holds it in the others (bench data, two splits: 67 % of the stage-2 queries failed in
// one split only). A split whose slots were proven needs no second look: every row stage 1 dropped there lies strictly beyond U, the
// exact k-th value of stage 1's answer; stage 2 can only LOWER the query's k-th value, so that proof still stands afterwards. Hence
// one failure list per stage-1 split, and a query is searched again only on the rows of the splits in whose lists it stands.
//   k_knn_split_lists   from stage 1's queue: list s = the queries with an unproven slot of split s; head = {failing queries, |list s|}
//                       (read back with the one round trip the gather makes anyway)
//   k_knn_range_layout  the lists laid end to end, each padded to whole groups of 256 queries: the qrange table (knn_internal.h)
//   k_knn_gather_lists  the rows, ids (~0u: padding) and seeds of the concatenated lists
//   run_knn             RANGED searches over that array, cut into chunks and given their kernels by size exactly as an unsplit stage 2
//                       is; their proofs cover the searched range, and what they cannot prove collects in ONE queue
//   knn_scan_queue      one exact scan for the call
//   k_knn_merge_lists   the answer of a query = the k smallest (distance, row) pairs of stage 1's answer and the result of every
//                       list it stands in, rows unique, ties to the lower row: stage 1's rows may lie in a split that was not searched
//                       again. One launch per list: a query stands in a list once, but may stand in several lists.
__global__ void k_knn_split_lists(const uint32_t* __restrict__ flag_count, const uint32_t* __restrict__ qrec, const uint32_t* __restrict__ items,
                                  int slots, int nq, uint32_t* __restrict__ head, uint32_t* __restrict__ lists) {
    const uint32_t n = flag_count[KNN_CNT_QUERIES];
    if (blockIdx.x == 0 && threadIdx.x == 0) head[0] = n;
    const int lane = lane_id();
    // a record per lane; whole waves stay in the loop: the places in a list are handed out with ONE atomic per wave and split (tens
    // of thousands of same-address atomics serialise)
    for (uint32_t t0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); t0 < n; t0 += gridDim.x * blockDim.x) {
        const uint32_t t = t0 + lane;
        uint32_t qi = 0u, mask = 0u;                                    // at most 64 slots of >= 4: at most 16 splits
        if (t < n) {
            qi = qrec[3 * (size_t)t];
            const uint32_t ibase = qrec[3 * (size_t)t + 1], ni = qrec[3 * (size_t)t + 2];
            for (uint32_t j = 0; j < ni; ++j) mask |= 1u << (items[2 * (size_t)(ibase + j) + 1] / (uint32_t)slots);
        }
        uint32_t any = mask;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o, 64);
        while (any) {
            const int s = __ffs((int)any) - 1; any &= any - 1u;
            const unsigned long long in = __ballot((mask >> s) & 1u);
            uint32_t base = 0u;
            if (lane == 0) base = atomicAdd(&head[1 + s], (uint32_t)__popcll(in));
            base = __shfl(base, 0, 64);
            if ((mask >> s) & 1u) lists[(size_t)s * nq + base + __popcll(in & ((1ull << lane) - 1ull))] = qi;
        }
    }
}
__global__ void k_knn_range_layout(const uint32_t* __restrict__ head, int n_lists, int rows_per_split, int n_rows, int* __restrict__ qrange) {
    int off = 0;
    for (int s = 0; s < n_lists; ++s) {
        const int groups = (int)((head[1 + s] + 255u) / 256u);
        for (int g = threadIdx.x; g < groups; g += blockDim.x) {
            int* e = qrange + 4 * (off / 256 + g);
            e[0] = s * rows_per_split; e[1] = min(n_rows, (s + 1) * rows_per_split); e[2] = s; e[3] = off;
        }
        off += groups * 256;
    }
}
// entry i of the concatenated lists (a workgroup each): row into q2 (ld floats apart, zero beyond dim and for padding), id, seed
__global__ __launch_bounds__(256) void k_knn_gather_lists(const uint32_t* __restrict__ head, const uint32_t* __restrict__ lists, int nq, const int* __restrict__ qrange,
                                                          const float* __restrict__ q, int dim, int ld, float* __restrict__ q2, uint32_t* __restrict__ list2,
                                                          const int32_t* __restrict__ idx1, const float* __restrict__ dist1, int k, float* __restrict__ dk2) {
    const int i = blockIdx.x;
    const int* rg = qrange + 4 * (i >> 8);
    const int s = rg[2], pos = i - rg[3];
    const bool live = (uint32_t)pos < head[1 + s];
    const uint32_t qi = live ? lists[(size_t)s * nq + pos] : ~0u;
    if (threadIdx.x == 0) {
        list2[i] = qi;
        if (dk2) dk2[i] = live && idx1[(size_t)qi * k + (k - 1)] >= 0 ? dist1[(size_t)qi * k + (k - 1)] : __builtin_nanf("");
    }
    for (int c = threadIdx.x; c < ld; c += blockDim.x) q2[(size_t)i * ld + c] = live && c < dim ? q[(size_t)qi * dim + c] : 0.f;
}
// entries i0 .. i0 + n - 1 (one list: distinct queries) folded into the caller's results
__global__ void k_knn_merge_lists(const uint32_t* __restrict__ list2, int i0, int n, int k, const int32_t* __restrict__ idx2, const float* __restrict__ dist2,
                                  int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const size_t a = (size_t)list2[i0 + t] * k, b = (size_t)(i0 + t) * k;
    // both inputs are ascending in (distance bits, row) with the empty entries (-1) last, as knn_select_write leaves them
    int32_t oi[KNN_MAX_K]; float od[KNN_MAX_K];
    int ia = 0, ib = 0, no = 0;
    while (no < k) {
        const bool ha = ia < k && idx_out[a + ia] >= 0, hb = ib < k && idx2[b + ib] >= 0;
        if (!ha && !hb) break;
        const unsigned long long ka = ha ? ((unsigned long long)__float_as_uint(dist_out[a + ia]) << 32) | (unsigned)idx_out[a + ia] : ~0ull;
        const unsigned long long kb = hb ? ((unsigned long long)__float_as_uint(dist2[b + ib]) << 32) | (unsigned)idx2[b + ib] : ~0ull;
        const unsigned long long key = ka <= kb ? ka : kb;
        if (ka <= kb) ++ia; else ++ib;
        bool dup = false;                                               // a row both searches found
        for (int j = 0; j < no; ++j) dup |= oi[j] == (int32_t)(key & 0xffffffffull);
        if (!dup) { oi[no] = (int32_t)(key & 0xffffffffull); od[no] = __uint_as_float((unsigned)(key >> 32)); ++no; }
    }
    for (int j = 0; j < k; ++j) { idx_out[a + j] = j < no ? oi[j] : -1; dist_out[a + j] = j < no ? od[j] : __builtin_nanf(""); }
}

// the chunk of a stage 2 over n queries that starts at o: a multiple of 32 768 queries, or the remainder (run_knn_two_stage)
inline int knn_stage2_chunk(int n_total, int o) { const int left = n_total - o; return left >= 32768 ? left / 32768 * 32768 : left; }
// the request of a stage-2 chunk of n queries (run_knn_two_stage explains the chunks).
// A chunk below one full round (a shard of the split on N GPUs: 8 300 stage-2 queries per rank at N = 8) would be 33 query tiles
// x 2 codebook splits = 66 workgroups on 256 CUs. The 128-query tile variant (k_knn_l2_ring16<T, 1>: four lane slots per split,
// so four splits) doubles the workgroups twice over instead.
KnnRequest knn_stage2_request(const ismhip_ctx* ctx, const ismhip_codebook* cb, int n, const float* seed_dk) {
    KnnRequest r2; r2.tname = "knn_stage2"; r2.many_splits = n < 4096;
    // (on the stage-2 image, if the codebook has one: 8 slices per tile instead of 11 on the bench data)
    r2.use_pca = cb->pca2.m > 0 && !(n < 4096) ? 2 : 0;
    r2.half = n >= 4096 && n < 32768 && !ctx->knn_stage2_t4;
    r2.seed_dk = seed_dk;
    return r2;
}

// cnt[s] = |list s| (host copy of the head). taken = false: the lists would not save an eighth of the sweep (queries that failed
// everywhere), or stage 1's splits do not end on 256-row tiles: the caller runs the unsplit stage 2.
int run_knn_stage2_lists(ismhip_ctx* ctx, const ismhip_codebook* cb, const KnnStage1& s1, const uint32_t* head_d, const uint32_t* lists_d, const uint32_t* cnt, int n2,
                         int nq, const float* q, int k, int32_t* idx_out, float* dist_out, bool& taken) {
    taken = false;
    const int S = s1.n_splits, rps = s1.rows_per_split, n_rows = cb->n_words_pad;
    if (S < 2 || rps % 256 != 0 || n_rows % 256 != 0) return ISMHIP_OK;
    int off[17] = {0}, rows_min = n_rows, rows_max = 0;
    double work = 0.0;
    for (int s = 0; s < S; ++s) {
        const int rows = std::min(n_rows, (s + 1) * rps) - s * rps;
        off[s + 1] = off[s] + (int)((cnt[s] + 255u) / 256u) * 256;
        if (cnt[s]) { rows_min = std::min(rows_min, rows); rows_max = std::max(rows_max, rows); work += (double)(off[s + 1] - off[s]) * rows; }
    }
    if (work * 8.0 > (double)n2 * n_rows * 7.0) return ISMHIP_OK;
    taken = true;
    ++ctx->knn_stage2_ranged;
    const int N = off[S], ld = cb->dim_pad;
    // every chunk's plan first: the queue holds the slots of all of them
    const bool seed = ctx->knn_stage2_seed;
    size_t q_items = 0; int n_chunks = 0;
    for (int o = 0; o < N; ++n_chunks) {
        const int n = knn_stage2_chunk(N, o);
        KnnRequest r2 = knn_stage2_request(ctx, cb, n, nullptr);
        r2.range_rows_min = rows_min; r2.range_rows_max = rows_max;
        q_items += (size_t)n * knn_plan(ctx, cb, ISMHIP_METRIC_L2SQ, n, k, 4, r2).n_bound;
        o += n;
    }
    if (n_chunks > 2) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn: more than two stage-2 chunks");       // (knn_stage2_chunk makes at most two)
    const int KM = k > 4 ? KNN_MAX_K : 4;
    float* q2 = (float*)ism_scratch(ctx, SCR_KNN_Q2, (size_t)N * ld * sizeof(float));
    uint32_t* list2 = (uint32_t*)ism_scratch(ctx, SCR_KNN_LIST2, (size_t)N * (sizeof(uint32_t) + (size_t)k * (sizeof(int32_t) + sizeof(float)) + sizeof(float)) + (size_t)(N / 256) * 4 * sizeof(int));
    uint32_t* qmem = (uint32_t*)ism_scratch(ctx, SCR_KNN_QUEUE, (KNN_CNT_WORDS + 3 * (size_t)N + 2 * q_items) * sizeof(uint32_t) + 8 + (q_items + KNN_FB_UNITS) * KM * sizeof(unsigned long long));
    if (!q2 || !list2 || !qmem) return ISMHIP_ERR_NOMEM;
    int32_t* idx2 = (int32_t*)(list2 + N);
    float* dist2 = (float*)(idx2 + (size_t)N * k);
    float* dk2 = dist2 + (size_t)N * k;
    int* qrange = (int*)(dk2 + N);
    KnnQueue Q{};
    Q.count = qmem; Q.qrec = qmem + KNN_CNT_WORDS; Q.items = Q.qrec + 3 * (size_t)N; Q.q_items = q_items;
    Q.item_out = (unsigned long long*)(((uintptr_t)(Q.items + 2 * q_items) + 7) & ~(uintptr_t)7);
    ISM_HIP(ctx, hipMemsetAsync(Q.count, 0, KNN_CNT_WORDS * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_knn_range_layout, dim3(1), dim3(256), 0, ctx->stream, head_d, S, rps, n_rows, qrange);
    ISM_CHECK_LAUNCH(ctx, "k_knn_range_layout");
    hipLaunchKernelGGL(k_knn_gather_lists, dim3(N), dim3(256), 0, ctx->stream, head_d, lists_d, nq, (const int*)qrange, q, cb->dim, ld, q2, list2,
                       (const int32_t*)idx_out, (const float*)dist_out, k, dk2);
    ISM_CHECK_LAUNCH(ctx, "k_knn_gather_lists");
    int chunk = 0;
    for (int o = 0; o < N; ++chunk) {
        const int n = knn_stage2_chunk(N, o);
        KnnRequest r2 = knn_stage2_request(ctx, cb, n, seed ? dk2 + o : nullptr);
        r2.qrange = qrange + 4 * (o / 256); r2.live = list2 + o; r2.queue = &Q; r2.q_base = o; r2.chunk = chunk;
        r2.range_rows_min = rows_min; r2.range_rows_max = rows_max; r2.q_ld = ld; r2.known_dk = dk2 + o;
        const int rc = run_knn(ctx, cb, ISMHIP_METRIC_L2SQ, n, q2 + (size_t)o * ld, k, 4, idx2 + (size_t)o * k, dist2 + (size_t)o * k, r2);
        if (rc != ISMHIP_OK) return rc;
        o += n;
    }
    // the scan's slots are slots of the searched ranges: what was not searched again stays proven (above)
    int rc = knn_scan_queue(ctx, cb, ISMHIP_METRIC_L2SQ, k, q2, ld, Q, qrange, idx2, dist2);
    if (rc != ISMHIP_OK) return rc;
    if (ctx->timers_on) ISM_HIP(ctx, hipMemcpyAsync(ctx->knn_stats, Q.count, 8, hipMemcpyDeviceToHost, ctx->stream));   // read back after a sync
    for (int s = 0; s < S; ++s) {
        if (!cnt[s]) continue;
        hipLaunchKernelGGL(k_knn_merge_lists, dim3((cnt[s] + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t*)list2, off[s], (int)cnt[s], k,
                           (const int32_t*)idx2, (const float*)dist2, idx_out, dist_out);
        ISM_CHECK_LAUNCH(ctx, "k_knn_merge_lists");
    }
    return ISMHIP_OK;
}

int run_knn_two_stage(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, int k, int32_t* idx_out, float* dist_out) {
    KnnStage1 s1{};
    KnnRequest r1; r1.stage1 = &s1; r1.use_pca = 1;
    int rc = run_knn(ctx, cb, ISMHIP_METRIC_L2SQ, nq, q, k, ctx->knn_t1 == 1 && k == 1 ? 1 : 2, idx_out, dist_out, r1);
    if (rc != ISMHIP_OK) return rc;
    KnnStage2 g;
    const bool seed = ctx->knn_stage2_seed;
    // ISMHIP_KNN_STAGE2_SPLITS=0: every stage-2 query sweeps the whole codebook again
    g.want_lists = ctx->knn_stage2_splits && s1.n_splits >= 2 && s1.n_splits <= 16;
    rc = knn_gather_stage2(ctx, cb, s1, q, k, g, seed ? idx_out : nullptr, seed ? dist_out : nullptr, nq);
    if (rc != ISMHIP_OK || g.n2 == 0) return rc;
    if (g.want_lists) {
        bool taken = false;
        rc = run_knn_stage2_lists(ctx, cb, s1, g.head_d, g.lists_d, g.cnt, g.n2, nq, q, k, idx_out, dist_out, taken);
        if (rc != ISMHIP_OK || taken) return rc;
        rc = knn_gather_unsplit(ctx, cb, s1, q, k, g, seed ? idx_out : nullptr, seed ? dist_out : nullptr);
        if (rc != ISMHIP_OK) return rc;
    }
    const int n2 = g.n2;
    // Stage 2 is SEEDED (k_knn_seed_thr): every lane slot starts from the threshold that stage 1's k-th exact value allows, so a slot
    // that does not overflow is proven by construction and few scores ever reach the insertion code. Four candidates per slot and two
    // splits, as in the cold start (ISMHIP_KNN_STAGE2_SEED=0): two candidates leave room for twice the codebook splits and make the sweep
    // itself no slower, but 0.9 % of the bench's stage-2 queries have three or more rows below their seed in ONE slot, overflow it and
    // go to the exact scan (605 instead of 11 queries per launch: + 4.7 ms; on a 114-object shard 97 instead of 6: + 0.07 ms). DESIGN.md §5.
    // Stage 2 runs 256-query tiles x 2 codebook splits on 256 CUs: 65 536 queries are two full rounds of workgroups, 66 000 are three
    // (measured from a cold start: 4.5 vs 6.7 ms). So a large stage 2 is cut into a multiple of 32 768 queries and a remainder, which
    // (below 4096 queries) takes the merged-splits kernel that fills the chip with splits instead of query tiles.
    for (int o = 0; o < n2;) {
        const int n = knn_stage2_chunk(n2, o);
        const KnnRequest r2 = knn_stage2_request(ctx, cb, n, g.dk2 ? g.dk2 + o : nullptr);
        rc = run_knn(ctx, cb, ISMHIP_METRIC_L2SQ, n, g.q2 + (size_t)o * cb->dim, k, 4, g.idx2 + (size_t)o * k, g.dist2 + (size_t)o * k, r2);
        if (rc != ISMHIP_OK) return rc;
        o += n;
    }
    return knn_scatter_stage2(ctx, g, k, idx_out, dist_out);
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

// ---- chi-square, k = 1: the queries the Hellinger proof left open ------------------------------------------------------------------
// Such a query has dozens to hundreds of rows whose Hellinger distance lies below its best chi-square value (more than fixed-size
// candidate lists hold), but stage 1 has already found a very good -- usually the -- nearest row, with exact value dk. Every row
// that can still beat or tie it has LB(score) (1 - ku) <= dk, i.e. score <= tau(dk): k_hell_tau computes tau per query, the EMIT
// variant of k_knn_l2_mfma16 sweeps the sqrt images once more and appends exactly those rows to a per-query list, k_hell_eval
// evaluates a fast chi-square for every listed row (a wave each) and then walks the functor's sequential chain for the rows
// within rounding of the smallest fast value and writes the winner. Proof by construction: a row that is not listed cannot win.
#define HELL_EMIT_CAP 2048
__global__ __launch_bounds__(256) void k_hell_tau(int n2, const uint32_t* __restrict__ list2, const float* __restrict__ sq2, int dim, int dim_pad,
                                                  const float* __restrict__ dist_out, VerifyParams vp, float* __restrict__ tau) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n2) return;
    const int lane = lane_id();
    const float qn2 = wave_norm2(sq2 + (size_t)i * dim_pad, dim, lane);
    if (lane == 0) {
        const float dk = dist_out[list2[i]];                             // k = 1: the best exact value of stage 1 (NaN: no candidate at all)
        const float eps_s = knn_eps_s(vp, qn2);
        // not emitted  <=>  score > tau  =>  LB(score) (1 - ku) > dk  (LB as in k_knn_rerank_hell, |score| <= |sqrt q|^2 + |sqrt c|max^2)
        float t = dk * (1.f + 2.f * vp.ku) - qn2 * (1.f - 16.f * KNN_U) + eps_s + 8.f * KNN_U * (qn2 + vp.cmax2 + dk);
        if (!(dk == dk)) t = __builtin_inff();                           // nothing found so far: everything is a candidate (the cap will tell)
        tau[i] = t;
    }
}
// one workgroup per query: its four waves evaluate the fast chi-square of the listed rows, wave 0 then walks the sequential chain
// for the rows within rounding of the smallest fast value (together with stage 1's answer) and writes the winner
__global__ __launch_bounds__(256) void k_hell_eval(int n2, const uint32_t* __restrict__ list2, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ rows, int cap,
                                                   const uint32_t* __restrict__ perm, const float* __restrict__ q, int dim, const float* __restrict__ words, int dim_pad, float ku,
                                                   int32_t* __restrict__ idx_out, float* __restrict__ dist_out, uint32_t* __restrict__ overflow) {
    __shared__ float s_fast[HELL_EMIT_CAP];
    __shared__ __attribute__((aligned(16))) float s_terms[KNN_TERMS];
    const int i = blockIdx.x;
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t qi = list2[i];
    const uint32_t n = cnt[i];
    if (n > (uint32_t)cap) { if (threadIdx.x == 0) atomicAdd(overflow, 1u); return; }
    const float* qp = q + (size_t)qi * dim;
    {
        const int n4 = dim >> 2;                                        // the caller's rows are dim floats apart: whole chunks only when dim % 4 == 0 (checked on the host)
        f32x4 qv[CHI_FAST_CH];
        chi2_fast_load_q(qp, n4, lane, qv);
        for (uint32_t s_ = wv; s_ < n; s_ += 4) {
            const float part = chi2_fast(qv, words + (size_t)perm[rows[(size_t)i * cap + s_]] * dim_pad, n4, lane);
            if (lane == 0) s_fast[s_] = part;
        }
    }
    __syncthreads();
    if (wv != 0) return;
    float mn = __builtin_inff();
    for (uint32_t s_ = lane; s_ < n; s_ += 64) mn = fminf(mn, s_fast[s_]);
    mn = wave_min_f(mn);
    const float win = mn * (1.f + 12.f * ku);                            // fast and chain values differ by <= 3 ku each way (see k_knn_rerank_hell)
    unsigned long long best = ~0ull;
    {
        const int id0 = idx_out[qi];                                     // stage 1's answer stays in the race
        if (id0 >= 0) best = ((unsigned long long)__float_as_uint(dist_out[qi]) << 32) | (unsigned)id0;
    }
    for (uint32_t s0 = 0; s0 < n; s0 += 64) {
        const uint32_t s_ = s0 + lane;
        const bool in = s_ < n && !(s_fast[s_] > win);
        unsigned long long pend = __ballot(in);
        const int row = in ? (int)perm[rows[(size_t)i * cap + s_]] : -1;
        while (pend) {
            const int src = __ffsll((long long)pend) - 1; pend &= pend - 1;
            const int cid = __shfl(row, src, 64);
            const float d = wave_functor(ISMHIP_METRIC_CHI2, qp, words + (size_t)cid * dim_pad, dim, lane, s_terms);
            const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)cid;
            best = key < best ? key : best;
        }
    }
    if (lane == 0 && best != ~0ull) { idx_out[qi] = (int)(best & 0xffffffffull); dist_out[qi] = __uint_as_float((unsigned)(best >> 32)); }
}

// chi-square, two stages: Hellinger candidates on the matrix cores + exact chi-square re-rank and proof (k_knn_rerank_hell); the
// queries that stage cannot prove are gathered and go through the VALU chi-square kernel (k_knn_chi2) with its own proof and
// exact scan. One 8-byte read-back (negative flag of the batch; later the number of unproven queries) synchronises the call.
int run_knn_chi2_hellinger(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, int k, int32_t* idx_out, float* dist_out, bool& taken) {
    taken = false;
    float* sq = (float*)ism_scratch(ctx, SCR_KNN_QSQRT, (size_t)nq * cb->dim_pad * sizeof(float) + 16);
    if (!sq) return ISMHIP_ERR_NOMEM;
    bool neg = false;
    int rc = knn_sqrt_queries(ctx, cb, nq, q, sq, neg);
    if (rc != ISMHIP_OK || neg) return rc;                              // not histogram data: the caller takes the VALU kernel
    taken = true;
    KnnStage1 s1{};
    KnnRequest rh; rh.stage1 = &s1; rh.hell_q = sq;
    rc = run_knn(ctx, cb, ISMHIP_METRIC_CHI2, nq, q, k, 4, idx_out, dist_out, rh);
    if (rc != ISMHIP_OK) return rc;
    KnnStage2 g;
    rc = knn_gather_stage2(ctx, cb, s1, q, k, g, nullptr, nullptr);
    if (rc != ISMHIP_OK || g.n2 == 0) return rc;
    const int n2 = g.n2;
    uint32_t* list2 = g.list2;
    if (k == 1 && ctx->knn_hell_emit) {
        // k = 1: list every row that can still beat stage 1's answer and evaluate those (see k_hell_tau)
        uint32_t over = 0;
        {
        TimerScope t2(ctx, "knn_stage2");
        const ismhip_codebook* xb = cb->chi_shadow;
        const int dp = cb->dim_pad, cap = HELL_EMIT_CAP;
        const int n2p = (n2 + 127) / 128 * 128;
        const size_t b_sq2 = (size_t)n2 * dp * 4, b_tau = (size_t)n2p * 4, b_cnt = (size_t)n2p * 4 + 64, b_rows = (size_t)n2 * cap * 4, b_img = (size_t)n2p * cb->ld16 * 2;
        char* buf = (char*)ism_scratch(ctx, SCR_KNN_HELL_EMIT, b_sq2 + b_tau + b_cnt + b_rows + b_img + 64);
        if (!buf) return ISMHIP_ERR_NOMEM;
        float* sq2 = (float*)buf; float* tau = (float*)(buf + b_sq2); uint32_t* cnt = (uint32_t*)(buf + b_sq2 + b_tau);
        uint32_t* sc = cnt + n2p;                                       // [0..2] f16 scalars of the gathered batch, [8] overflow counter
        uint32_t* rows = (uint32_t*)(buf + b_sq2 + b_tau + b_cnt); u16* qimg = (u16*)(buf + b_sq2 + b_tau + b_cnt + b_rows);
        ISM_HIP(ctx, hipMemsetAsync(cnt, 0, b_cnt, ctx->stream));
        hipLaunchKernelGGL(k_knn_gather_flagged, dim3(n2), dim3(256), 0, ctx->stream, s1.qrec, n2, (const float*)sq, dp, sq2, list2,
                           (const int32_t*)nullptr, (const float*)nullptr, k, (float*)nullptr);
        ISM_CHECK_LAUNCH(ctx, "k_knn_gather_flagged");
        rc = knn_f16_emit_image(ctx, cb, xb, sq2, n2, dp, n2p, sc, qimg);
        if (rc != ISMHIP_OK) return rc;
        const VerifyParams vp = knn_verify_params(xb, dp, 0, sc, false);
        hipLaunchKernelGGL(k_hell_tau, dim3((n2 + 3) / 4), dim3(256), 0, ctx->stream, n2, (const uint32_t*)list2, (const float*)sq2, cb->dim, dp, (const float*)dist_out, vp, tau);
        ISM_CHECK_LAUNCH(ctx, "k_hell_tau");
        rc = knn_mfma16_emit(ctx, cb, xb, n2, n2p, sc, qimg, tau, cnt, rows, cap);
        if (rc != ISMHIP_OK) return rc;
        hipLaunchKernelGGL(k_hell_eval, dim3(n2), dim3(256), 0, ctx->stream, n2, (const uint32_t*)list2, (const uint32_t*)cnt, (const uint32_t*)rows, cap,
                           (const uint32_t*)xb->shadow_perm, q, cb->dim, (const float*)cb->words, dp, vp.ku, idx_out, dist_out, sc + 8);
        ISM_CHECK_LAUNCH(ctx, "k_hell_eval");
        ISM_HIP(ctx, hipMemcpyAsync(&over, sc + 8, 4, hipMemcpyDeviceToHost, ctx->stream));
        ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        ctx->knn_stats[0] = over; ctx->knn_stats[1] = 0;
        if (over == 0) return ISMHIP_OK;                                // every list fitted: done
        // some query has more than HELL_EMIT_CAP rows below its best value: the VALU kernel answers for all gathered queries
    }
    {
        TimerScope t2(ctx, "knn_stage2");
        KnnRequest rv; rv.tname = "knn_chi2_valu";
        rc = run_knn(ctx, cb, ISMHIP_METRIC_CHI2, g.n2, g.q2, k, k > 2 ? 4 : 2, g.idx2, g.dist2, rv);
        if (rc != ISMHIP_OK) return rc;
    }
    return knn_scatter_stage2(ctx, g, k, idx_out, dist_out);
}

}  // namespace

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

// knn_rerank.hip — exact re-rank with the FLANN functors' summation order, and the proof (map of the units: knn.hip).
// k_knn_rerank (_pca, _hell) — one wave per query: candidates that can still matter are recomputed with the FLANN functor's own
// summation order (bit-identical to the CPU functor), the k smallest (distance, row) pairs are selected (ties: lowest row), and the
// result is PROVEN slot by slot from the slot bounds and a rigorous bound of the candidate kernel's error; a (query, slot) pair that
// cannot be proven is queued for the exact scan (knn_scan.hip). The three kernels differ in how they pick the candidates to evaluate
// and in their proof; what they share is written once (knn_load_cand, knn_select_write, knn_queue_unproven here; wave_norm2,
// knn_eps_s_raw, the slot proofs in knn_internal.h). Also here: k_knn_merge_splits (many splits -> one slot) and k_knn_seed_thr.
#include "knn_internal.h"

namespace {

// Folds the candidates of MANY codebook splits into one slot. A wave per query keeps the KNN_MERGE_KEEP smallest approximate
// scores of all splits' candidates; the merged bound is the smallest score anything dropped: every split slot's own bound and the
// best candidate this merge leaves out. (A NaN bound stays NaN, so that the proof fails and the query takes the exact scan.)
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
    const float *qn2, *qn2h;          // the rotation pass's |q|^2 and sums of squares of the image rows (k_rotate_split16); nullptr: summed here
    float inv_sq2;                    // 1 / scale^2 of that image
    float inv_sig2, d_rel, dq_abs, dc;   // 1 / sigma_max^2 (rounded down); |x^ - R x| <= d_rel |x| + abs; dc = the codeword side for |c| = |c|max
    float eps_c2, dot2, cmax2;        // eps_acc = eps_c2 + dot2 |q^||c^|max;  cmax2 = max |c^|^2
    float ku;
};
// what LB(s) takes of query qi (row qp of dim floats), by the whole wave: |q|^2 and |q^|^2 as the rotation pass left them, or (the
// FP32 rotation) by wave_norm2 and from the image itself. Every kernel that calls this for a query gets the same bits.
__device__ __forceinline__ PcaLb pca_lb_query(const PcaVerify& pv, int qi, const float* __restrict__ qp, int dim, int lane) {
    float qn2, qn2h;
    if (pv.qn2) { qn2 = pv.qn2[qi]; qn2h = pv.qn2h[qi]; }
    else {
        qn2 = wave_norm2(qp, dim, lane);
        float s = 0.f;                                                 // |q^|^2 from the image itself (the halves as stored: any element order)
        for (int i = lane; i < pv.nk * F16T_KB; i += 64) {
            const float v = (float)__builtin_bit_cast(_Float16, pv.qimg[f16t_stored(qi, pv.nk, i)]);
            s += v * v;
        }
        qn2h = wave_sum_f(s);
    }
    PcaLb b;
    b.qn2h = qn2h * pv.inv_sq2;
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
    const PcaLb lbq = pca_lb_query(pv, qi, qp, dim, lane);
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
    float qn2 = 0.f;
    PcaLb lbq{};
    if (pca) lbq = pca_lb_query(pv, qi, q + (size_t)qi * ldq, dim, lane);
    else qn2 = wave_norm2(q + (size_t)qi * ldq, dim, lane);
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

// the constants of the lower-bound proof on the run's rotated image (k_knn_rerank_pca, k_knn_seed_thr)
PcaVerify knn_pca_verify(const KnnRun& r, const VerifyParams& vp) {
    const PcaImage& PI = *r.PI;
    PcaVerify pv;
    const float acc_rel = 1.01f * (float)PI.m * 1.1920929e-07f;            // accumulation only: products of f16 values are exact in fp32
    pv.qimg = r.q_hi; pv.nk = r.p.ring_nk; pv.inv_sq2 = 1.0f / (PI.sq * PI.sq);
    pv.qn2 = r.qn2; pv.qn2h = r.qn2h;
    const bool split = r.qn2 != nullptr;                                   // the query image came from the f16 matrix cores: its own constants
    pv.inv_sig2 = PI.inv_sig2; pv.d_rel = split ? PI.dq_rel16 : PI.d_rel; pv.dq_abs = split ? PI.dq_abs16 : PI.dq_abs;
    pv.dc = (PI.d_rel * sqrtf(r.cb->max_norm2) + PI.dc_abs) * 1.00001f;
    pv.cmax2 = PI.cmax2;
    // subnormal f16 operands may be flushed to zero by the matrix cores: |dq_i| <= 2^-14 / sq, |dc_i| <= 2^-14 / sc per element
    const float fq = F16_FLUSH / PI.sq, fc = F16_FLUSH / PI.sc, sm = sqrtf((float)PI.m);
    pv.eps_c2 = (17.f * KNN_U + 1.01f * (float)(PI.m + 1) * 1.1920929e-07f) * PI.cmax2 + 2.02f * (sm * fq * sqrtf(PI.cmax2) + sm * sm * fq * fc);
    pv.dot2 = 2.f * acc_rel + 2.f * KNN_U + 2.02f * sm * fc / sqrtf(PI.cmax2);
    pv.ku = vp.ku;
    return pv;
}

KnnQueueTag knn_queue_tag(const KnnRanged* g) { return g ? KnnQueueTag{g->live, g->q_base, g->chunk << 8, g->known_dk} : KnnQueueTag{nullptr, 0, 0, nullptr}; }

}  // namespace

int knn_seed_thresholds(KnnRun& r, const float* out_scale, float* thr0) {
    ismhip_ctx* ctx = r.ctx; const ismhip_codebook* cb = r.cb; const KnnPlan& p = r.p;
    const VerifyParams vp = knn_verify_params(r.xb, cb->dim_pad, p.mode, r.qsc, true);
    hipLaunchKernelGGL(k_knn_seed_thr, dim3((r.nq + 3) / 4), dim3(256), 0, ctx->stream, r.qq, r.nq, r.ldq, cb->dim, r.rq->seed_dk,
                       p.pca, p.pca ? knn_pca_verify(r, vp) : PcaVerify{}, vp, out_scale, thr0, knn_queue_tag(r.rq->ranged).live);
    ISM_CHECK_LAUNCH(ctx, "k_knn_seed_thr");
    ++ctx->knn_seed_launches;
    return ISMHIP_OK;
}

int knn_rerank_prove(KnnRun& r, int32_t* idx_out, float* dist_out) {
    ismhip_ctx* ctx = r.ctx; const ismhip_codebook* cb = r.cb; const KnnPlan& p = r.p; const KnnQueue& Q = r.queue;
    const VerifyParams vp = knn_verify_params(r.xb, cb->dim_pad, p.mode, r.qsc, true);
    const dim3 grid((r.nq + 3) / 4), block(256);
    const KnnQueueTag tg = knn_queue_tag(r.rq->ranged);
    if (p.merged) {
        float* m_val = r.cand_bound + (size_t)r.nq * r.n_bound; float* m_bound = m_val + (size_t)r.nq * KNN_MERGE_KEEP;
        int* m_idx = r.cand_idx + (size_t)r.nq * r.n_cand;
        hipLaunchKernelGGL(k_knn_merge_splits, grid, block, 0, ctx->stream, r.nq, r.cand_val, r.cand_idx, r.n_cand, r.cand_bound, r.n_bound, m_val, m_idx, m_bound);
        ISM_CHECK_LAUNCH(ctx, "k_knn_merge_splits");
        r.cand_val = m_val; r.cand_idx = m_idx; r.cand_bound = m_bound; r.n_cand = KNN_MERGE_KEEP; r.n_bound = 1;
    }
    TimerScope trr(ctx, "knn_rerank");
    if (p.pca) {
        const PcaVerify pv = knn_pca_verify(r, vp);
        hipLaunchKernelGGL(k_knn_rerank_pca, grid, block, 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words,
                           r.qq, r.nq, r.ldq, r.cand_idx, r.cand_val, r.n_cand, r.n_cand, r.cand_bound, r.n_bound, pv, r.k, idx_out, dist_out, Q.count, Q.qrec, Q.items, tg);
    } else if (p.hell) {
        hipLaunchKernelGGL(k_knn_rerank_hell, grid, block, 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words,
                           r.qq, r.nq, r.ldq, r.rq->hell_q, r.xb->shadow_perm, r.cand_idx, r.cand_val, r.n_cand, r.n_cand, r.cand_bound, r.n_bound, vp, r.k, idx_out, dist_out, Q.count, Q.qrec, Q.items, tg);
    } else
    hipLaunchKernelGGL(k_knn_rerank, grid, block, 0, ctx->stream, cb->words, cb->dim, cb->dim_pad, cb->n_words,
                       r.qq, r.nq, r.ldq, r.metric, r.cand_idx, r.cand_val, r.n_cand, r.n_cand, r.cand_bound, r.n_bound, vp, r.k, idx_out, dist_out, Q.count, Q.qrec, Q.items, tg);
    ISM_CHECK_LAUNCH(ctx, "k_knn_rerank");
    return ISMHIP_OK;
}

// knn_two_stage.hip — the two-stage drivers of the codeword search (map: knn.hip), squared L2 and chi-square, and the stage-2 steps they share.
#include "knn_internal.h"

namespace {

// ---- two-stage search -------------------------------------------------------------------------------------------------------
// The top-T bookkeeping in the candidate kernel's epilogue costs time in proportion to T (measured, 262144 queries x 102400
// words: T = 4 18.7 ms, T = 2 16.8 ms, T = 1 16.2 ms), but a small T leaves more queries unproven (T = 2: ~0.1 % of them, T = 1:
// ~3 %), and the exact scan that finishes an unproven query reads its slots' share of the f32 codebook (24 us per query).
// So: stage 1 runs T = 2 over all queries; the few queries its proof rejects are gathered and searched again with T = 4 (a
// launch ~1000x smaller), and only what THAT proof rejects goes to the exact scan. Every answer is still the exact functor
// minimum, proven or scanned.
// Entry i of a stage 2 (a workgroup each): its query qi -- record i of stage 1's queue, or (qrange != nullptr) entry i of the failure
// lists laid end to end, ~0u for the padding between two lists -- goes to list2, its row (src_ld floats apart) to q2 (ld apart, zero
// beyond dim and for padding) and, dk2 != nullptr, the k-th exact value stage 1 found for it to dk2: NaN when it found fewer than k rows
__global__ __launch_bounds__(256) void k_knn_gather(const uint32_t* __restrict__ qrec, const uint32_t* __restrict__ head, const uint32_t* __restrict__ lists, int nq,
                                                    const int* __restrict__ qrange, const float* __restrict__ q, int src_ld, int dim, int ld,
                                                    float* __restrict__ q2, uint32_t* __restrict__ list2, const int32_t* __restrict__ idx1, const float* __restrict__ dist1, int k, float* __restrict__ dk2) {
    const int i = blockIdx.x;
    uint32_t qi = ~0u;
    if (!qrange) qi = qrec[3 * (size_t)i];
    else if (const int* rg = qrange + 4 * (i >> 8); (uint32_t)(i - rg[3]) < head[1 + rg[2]]) qi = lists[(size_t)rg[2] * nq + (i - rg[3])];
    const bool live = qi != ~0u;
    if (threadIdx.x == 0) {
        list2[i] = qi;
        if (dk2) dk2[i] = live && idx1[(size_t)qi * k + (k - 1)] >= 0 ? dist1[(size_t)qi * k + (k - 1)] : __builtin_nanf("");
    }
    for (int c = threadIdx.x; c < ld; c += blockDim.x) q2[(size_t)i * ld + c] = live && c < dim ? q[(size_t)qi * src_ld + c] : 0.f;
}
__global__ void k_knn_scatter_results(const uint32_t* __restrict__ list2, int n2, int k, const int32_t* __restrict__ idx2, const float* __restrict__ dist2,
                                      int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n2 * k) return;
    const size_t o = (size_t)list2[t / k] * k + (t % k);
    idx_out[o] = idx2[t]; dist_out[o] = dist2[t];
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
//   k_knn_gather        the rows, ids (~0u: padding) and seeds of the concatenated lists
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

// the chunks of a stage 2 over n_total queries, in order: a multiple of 32 768 queries, then the remainder (run_knn_two_stage
// explains them); each(chunk, o, n) is called for chunk number `chunk`, the n queries from o on, until one fails
template <class F> int knn_stage2_chunks(int n_total, F&& each) {
    for (int o = 0, n, chunk = 0, rc; o < n_total; o += n, ++chunk) {
        const int left = n_total - o; n = left >= 32768 ? left / 32768 * 32768 : left;
        if ((rc = each(chunk, o, n)) != ISMHIP_OK) return rc;
    }
    return ISMHIP_OK;
}
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

// ---- the second stage's bookkeeping, shared by both drivers ---------------------------------------------------------------------------
// n2 queries a first stage left unproven, gathered as n entries (the queries, or their per-split failure lists end to end): rows q2,
// ids list2 (~0u: padding), the second search's results idx2 / dist2, the seeds dk2 (k-th exact value of stage 1; nullptr: none wanted),
// the qrange table of a ranged search (nullptr: none); the failure lists lists_d[s * nq ...], head_d = {n2, |list 0|, ...}, sizes cnt
struct KnnStage2 { int n2, n; float* q2; uint32_t* list2; int32_t* idx2; float* dist2; float* dk2; int* qrange; uint32_t *head_d = nullptr, *lists_d = nullptr; uint32_t cnt[16] = {}; };
// g.n2 (the one host round trip of the call; 0: nothing left to do); want_lists (nq = the call's queries): lists and sizes in the same read-back
int knn_stage2_count(ismhip_ctx* ctx, const KnnStage1& s1, KnnStage2& g, bool want_lists, int nq) {
    uint32_t hb[17] = {0};
    if (want_lists) {
        g.head_d = (uint32_t*)ism_scratch(ctx, SCR_KNN_LISTS, (32 + (size_t)s1.n_splits * nq) * sizeof(uint32_t));
        if (!g.head_d) return ISMHIP_ERR_NOMEM;
        g.lists_d = g.head_d + 32;
        ISM_HIP(ctx, hipMemsetAsync(g.head_d, 0, 32 * sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(k_knn_split_lists, dim3(256), dim3(256), 0, ctx->stream, (const uint32_t*)s1.queue.count, (const uint32_t*)s1.queue.qrec, (const uint32_t*)s1.queue.items,
                           s1.slots, nq, g.head_d, g.lists_d);
        ISM_CHECK_LAUNCH(ctx, "k_knn_split_lists");
        ISM_HIP(ctx, hipMemcpyAsync(hb, g.head_d, 17 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    } else ISM_HIP(ctx, hipMemcpyAsync(hb, s1.queue.count, 4, hipMemcpyDeviceToHost, ctx->stream));
    ISM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->knn_stage2_queries = hb[0]; ctx->knn_stage2_list_entries = 0;
    for (int s = 0; s < 16; ++s) { g.cnt[s] = hb[1 + s]; ctx->knn_stage2_list_entries += g.cnt[s]; }
    g.n2 = (int)hb[0];      // (nothing left: no scan ran, its counters read zero)
    if (g.n2 == 0) ctx->knn_stats[0] = ctx->knn_stats[1] = 0;
    return ISMHIP_OK;
}

// the block of g for n entries with rows of ld floats: q2 | list2 | idx2 | dist2 (| dk2 if seeds) (| qrange if ranges)
int knn_stage2_carve(ismhip_ctx* ctx, KnnStage2& g, int n, int ld, int k, bool seeds, bool ranges) {
    g.n = n;
    g.q2 = (float*)ism_scratch(ctx, SCR_KNN_Q2, (size_t)n * ld * sizeof(float));
    g.list2 = (uint32_t*)ism_scratch(ctx, SCR_KNN_LIST2, (size_t)n * (sizeof(uint32_t) + (size_t)k * (sizeof(int32_t) + sizeof(float)) + (seeds ? sizeof(float) : 0))
                                                         + (ranges ? (size_t)(n / 256) * 4 * sizeof(int) : 0));
    if (!g.q2 || !g.list2) return ISMHIP_ERR_NOMEM;
    g.idx2 = (int32_t*)(g.list2 + n); g.dist2 = (float*)(g.idx2 + (size_t)n * k);
    float* end = g.dist2 + (size_t)n * k; g.dk2 = seeds ? end : nullptr;
    g.qrange = ranges ? (int*)(end + (seeds ? n : 0)) : nullptr;
    return ISMHIP_OK;
}

// the entries of g (k_knn_gather; g.qrange == nullptr: record i of s1's queue) with rows from src to dst; seeds only if idx1
int knn_stage2_gather(ismhip_ctx* ctx, const KnnStage1& s1, const KnnStage2& g, int nq, const float* src, int src_ld, int dim, float* dst, int ld, int k, const int32_t* idx1, const float* dist1) {
    hipLaunchKernelGGL(k_knn_gather, dim3(g.n), dim3(256), 0, ctx->stream, (const uint32_t*)s1.queue.qrec, (const uint32_t*)g.head_d, (const uint32_t*)g.lists_d, nq,
                       (const int*)g.qrange, src, src_ld, dim, ld, dst, g.list2, idx1, dist1, k, idx1 ? g.dk2 : nullptr);
    ISM_CHECK_LAUNCH(ctx, "k_knn_gather");
    return ISMHIP_OK;
}

// The lists route. g.cnt[s] = |list s| (host copy of the head). taken = false: the lists would not save an eighth of the sweep
// (queries that failed everywhere), or stage 1's splits do not end on 256-row tiles: the caller runs the unsplit stage 2.
int run_knn_stage2_lists(ismhip_ctx* ctx, const ismhip_codebook* cb, const KnnStage1& s1, KnnStage2& g, int nq, const float* q, int k, int32_t* idx_out, float* dist_out, bool& taken) {
    taken = false;
    const int S = s1.n_splits, rps = s1.rows_per_split, n_rows = cb->n_words_pad;
    if (S < 2 || rps % 256 != 0 || n_rows % 256 != 0) return ISMHIP_OK;
    int off[17] = {0}; KnnRanged rg{}; rg.rows_min = n_rows;
    double work = 0.0;
    for (int s = 0; s < S; ++s) {
        const int rows = std::min(n_rows, (s + 1) * rps) - s * rps;
        off[s + 1] = off[s] + (int)((g.cnt[s] + 255u) / 256u) * 256;
        if (g.cnt[s]) { rg.rows_min = std::min(rg.rows_min, rows); rg.rows_max = std::max(rg.rows_max, rows); work += (double)(off[s + 1] - off[s]) * rows; }
    }
    if (work * 8.0 > (double)g.n2 * n_rows * 7.0) return ISMHIP_OK;
    taken = true; ++ctx->knn_stage2_ranged;
    const int N = off[S], ld = cb->dim_pad; const bool seed = ctx->knn_stage2_seed;
    // every chunk's plan first: the queue holds the slots of all of them
    size_t q_items = 0; int n_chunks = 0, rc;
    (void)knn_stage2_chunks(N, [&](int, int, int n) {      // (cannot fail)
        KnnRequest r2 = knn_stage2_request(ctx, cb, n, nullptr); r2.ranged = &rg;
        q_items += (size_t)n * knn_plan(ctx, cb, ISMHIP_METRIC_L2SQ, n, k, 4, r2).n_bound; ++n_chunks;
        return ISMHIP_OK;
    });
    if (n_chunks > 2) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "knn: more than two stage-2 chunks");       // (knn_stage2_chunks makes at most two)
    rc = knn_stage2_carve(ctx, g, N, ld, k, true, true);
    if (rc != ISMHIP_OK) return rc;
    void* qmem = ism_scratch(ctx, SCR_KNN_QUEUE, knn_queue_bytes(N, q_items, k));
    if (!qmem) return ISMHIP_ERR_NOMEM;
    KnnQueue Q = knn_queue_carve(qmem, N, q_items);
    ISM_HIP(ctx, hipMemsetAsync(Q.count, 0, KNN_CNT_WORDS * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_knn_range_layout, dim3(1), dim3(256), 0, ctx->stream, (const uint32_t*)g.head_d, S, rps, n_rows, g.qrange);
    ISM_CHECK_LAUNCH(ctx, "k_knn_range_layout");
    rc = knn_stage2_gather(ctx, s1, g, nq, q, cb->dim, cb->dim, g.q2, ld, k, idx_out, dist_out);
    if (rc != ISMHIP_OK) return rc;
    rg.queue = &Q;
    rc = knn_stage2_chunks(N, [&](int chunk, int o, int n) {
        KnnRequest r2 = knn_stage2_request(ctx, cb, n, seed ? g.dk2 + o : nullptr);
        rg.qrange = g.qrange + 4 * (o / 256); rg.live = g.list2 + o; rg.q_base = o; rg.chunk = chunk; rg.known_dk = g.dk2 + o;
        r2.ranged = &rg; r2.q_ld = ld;
        return run_knn(ctx, cb, ISMHIP_METRIC_L2SQ, n, g.q2 + (size_t)o * ld, k, 4, g.idx2 + (size_t)o * k, g.dist2 + (size_t)o * k, r2);
    });
    if (rc != ISMHIP_OK) return rc;
    // the scan's slots are slots of the searched ranges: what was not searched again stays proven (above)
    rc = knn_scan_queue(ctx, cb, ISMHIP_METRIC_L2SQ, k, g.q2, ld, Q, g.qrange, g.idx2, g.dist2);
    if (rc != ISMHIP_OK) return rc;
    if (ctx->timers_on) ISM_HIP(ctx, hipMemcpyAsync(ctx->knn_stats, Q.count, 8, hipMemcpyDeviceToHost, ctx->stream));   // read back after a sync
    for (int s = 0; s < S; ++s) {
        if (!g.cnt[s]) continue;
        hipLaunchKernelGGL(k_knn_merge_lists, dim3((g.cnt[s] + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t*)g.list2, off[s], (int)g.cnt[s], k,
                           (const int32_t*)g.idx2, (const float*)g.dist2, idx_out, dist_out);
        ISM_CHECK_LAUNCH(ctx, "k_knn_merge_lists");
    }
    return ISMHIP_OK;
}

}  // namespace

int run_knn_two_stage(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, int k, int32_t* idx_out, float* dist_out) {
    KnnStage1 s1{}; KnnRequest r1; r1.stage1 = &s1; r1.use_pca = 1;
    int rc = run_knn(ctx, cb, ISMHIP_METRIC_L2SQ, nq, q, k, ctx->knn_t1 == 1 && k == 1 ? 1 : 2, idx_out, dist_out, r1);
    if (rc != ISMHIP_OK) return rc;
    KnnStage2 g{}; const bool seed = ctx->knn_stage2_seed;
    // ISMHIP_KNN_STAGE2_SPLITS=0: every stage-2 query sweeps the whole codebook again
    const bool want_lists = ctx->knn_stage2_splits && s1.n_splits >= 2 && s1.n_splits <= 16;
    rc = knn_stage2_count(ctx, s1, g, want_lists, nq);
    if (rc != ISMHIP_OK || g.n2 == 0) return rc;
    if (want_lists) {
        bool taken = false;
        rc = run_knn_stage2_lists(ctx, cb, s1, g, nq, q, k, idx_out, dist_out, taken);
        if (rc != ISMHIP_OK || taken) return rc;
    }
    // the unsplit route: the n2 queries themselves (rows of dim floats), each sweeps the whole codebook again
    rc = knn_stage2_carve(ctx, g, g.n2, cb->dim, k, seed, false);
    if (rc == ISMHIP_OK) rc = knn_stage2_gather(ctx, s1, g, nq, q, cb->dim, cb->dim, g.q2, cb->dim, k, seed ? idx_out : nullptr, seed ? dist_out : nullptr);
    if (rc != ISMHIP_OK) return rc;
    // Stage 2 is SEEDED (k_knn_seed_thr): every lane slot starts from the threshold that stage 1's k-th exact value allows, so a slot
    // that does not overflow is proven by construction and few scores ever reach the insertion code. Four candidates per slot and two
    // splits, as in the cold start (ISMHIP_KNN_STAGE2_SEED=0): two candidates leave room for twice the codebook splits and make the sweep
    // itself no slower, but 0.9 % of the bench's stage-2 queries have three or more rows below their seed in ONE slot, overflow it and
    // go to the exact scan (605 instead of 11 queries per launch: + 4.7 ms; on a 114-object shard 97 instead of 6: + 0.07 ms). DESIGN.md §5.
    // Stage 2 runs 256-query tiles x 2 codebook splits on 256 CUs: 65 536 queries are two full rounds of workgroups, 66 000 are three
    // (measured from a cold start: 4.5 vs 6.7 ms). So a large stage 2 is cut into a multiple of 32 768 queries and a remainder, which
    // (below 4096 queries) takes the merged-splits kernel that fills the chip with splits instead of query tiles.
    rc = knn_stage2_chunks(g.n, [&](int, int o, int n) {
        const KnnRequest r2 = knn_stage2_request(ctx, cb, n, g.dk2 ? g.dk2 + o : nullptr);
        return run_knn(ctx, cb, ISMHIP_METRIC_L2SQ, n, g.q2 + (size_t)o * cb->dim, k, 4, g.idx2 + (size_t)o * k, g.dist2 + (size_t)o * k, r2);
    });
    if (rc != ISMHIP_OK) return rc;
    hipLaunchKernelGGL(k_knn_scatter_results, dim3((g.n * k + 255) / 256), dim3(256), 0, ctx->stream, g.list2, g.n, k, g.idx2, g.dist2, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_knn_scatter_results");       // idx2 / dist2 to the queries' places in the caller's arrays
    return ISMHIP_OK;
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
    KnnStage2 g{};
    rc = knn_stage2_count(ctx, s1, g, false, nq);
    if (rc != ISMHIP_OK || g.n2 == 0) return rc;
    rc = knn_stage2_carve(ctx, g, g.n2, cb->dim, k, false, false);      // the n2 queries themselves, rows of dim floats
    if (rc == ISMHIP_OK) rc = knn_stage2_gather(ctx, s1, g, nq, q, cb->dim, cb->dim, g.q2, cb->dim, k, nullptr, nullptr);
    if (rc != ISMHIP_OK) return rc;
    const int n2 = g.n2; uint32_t* list2 = g.list2;
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
        rc = knn_stage2_gather(ctx, s1, g, nq, sq, dp, dp, sq2, dp, k, nullptr, nullptr);      // the square-root rows of the same queries
        if (rc != ISMHIP_OK) return rc;
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
    hipLaunchKernelGGL(k_knn_scatter_results, dim3((g.n * k + 255) / 256), dim3(256), 0, ctx->stream, g.list2, g.n, k, g.idx2, g.dist2, idx_out, dist_out);
    ISM_CHECK_LAUNCH(ctx, "k_knn_scatter_results");       // idx2 / dist2 to the queries' places in the caller's arrays
    return ISMHIP_OK;
}

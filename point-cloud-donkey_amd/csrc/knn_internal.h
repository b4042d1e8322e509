// knn_internal.h — what more than one unit of the codeword search needs (the map of the units is at the top of knn.hip; pca.hip
// includes it for the f16 images): the types and device helpers in an anonymous namespace (they appear in kernel signatures, so
// every unit has its own) -- candidate lists, THE definition of the scaled f16 images and their tiled layout, the error model of
// the proofs, the slot proofs, the counter block of the queue -- then the host-side records of a search (request, plan, run, queue)
// and, unit by unit, the host functions through which the units call each other, each defined in the unit whose kernels it launches.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#include "functor.h"         // wave_functor: re-rank, exact scans, EMIT evaluation

#define KNN_BM 128       // codeword rows per tile
#define KNN_BN 128       // queries per tile
#define CHI_B 64         // both, in k_knn_chi2
#define KNN_MAX_K 16
#define KNN_FB_MAXJ 84          // dim_pad <= 1344 -> at most 84 elements per lane of a 16-lane row group
#define KNN_TERMS (16 * KNN_FB_MAXJ)   // floats of LDS a wave hands to wave_functor: one term per element of the longest row

template <int T>
struct TopT {
    float v[T]; int i[T];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int t = 0; t < T; ++t) { v[t] = __builtin_inff(); i[t] = -1; }
    }
    // the same insertion without a branch (k_knn_l2_ring16's epilogue: a wave enters it when ANY lane has a score to insert, and
    // nested exec-mask branches cost more than thirteen predicated instructions); x = +inf leaves the list as it is
    __device__ __forceinline__ void push_flat(float x, int idx) {
        bool c[T];
#pragma unroll
        for (int t = 0; t < T; ++t) c[t] = x < v[t];
#pragma unroll
        for (int t = T - 1; t > 0; --t) {
            v[t] = c[t - 1] ? v[t - 1] : (c[t] ? x : v[t]);
            i[t] = c[t - 1] ? i[t - 1] : (c[t] ? idx : i[t]);
        }
        v[0] = c[0] ? x : v[0];
        i[0] = c[0] ? idx : i[0];
    }
    // insert keeping ascending order; strict < keeps the earlier (lower row) on ties
    __device__ __forceinline__ void push(float x, int idx) {
        if (!(x < v[T - 1])) return;
        v[T - 1] = x; i[T - 1] = idx;
#pragma unroll
        for (int t = T - 1; t > 0; --t) {
            if (v[t] < v[t - 1]) {
                float tv = v[t]; v[t] = v[t - 1]; v[t - 1] = tv;
                int ti = i[t]; i[t] = i[t - 1]; i[t - 1] = ti;
            }
        }
    }
};

// dynamic LDS of k_knn_l2_mfma16 (bytes): two slices of the BM codeword and BN query rows (two images each for bf16x3) + |c|^2 of a tile
constexpr size_t knn_mfma16_lds(int BM, int BN, int KB, int NTERM) { return (size_t)2 * (BM + BN) * KB * sizeof(u16) * (NTERM == 3 ? 2 : 1) + BM * sizeof(float); }
#define RG_BN 256
#define RG_KB 32
// LDS layout of k_knn_l2_ring16<T, WR, QP, PRE> in bytes: the ring of STAGES stages at 0, |c|^2 of four tiles at cn (a DMA always
// delivers 256 floats), the thresholds published to the partner wave at thr (WR = 2: [8 waves][4 n-tiles][64]) and, QP = 2, the
// query panel [ring_nk slices][256 queries][32 halves] at panel. The kernel takes its pointers from it, the host its launch size.
template <int WR, int QP>
struct Ring16Lds {
    static constexpr int STAGES = WR == 2 ? 4 : 3, STAGE_HALVES = (QP ? WR * 128 : WR * 128 + RG_BN) * RG_KB;
    static constexpr size_t cn = (size_t)STAGES * STAGE_HALVES * sizeof(u16);
    static constexpr size_t thr = cn + 4 * 256 * sizeof(float);
    static constexpr size_t panel = thr + (WR == 2 ? 8 * 4 * 64 * sizeof(float) : 0);
    static constexpr size_t total(int ring_nk) { return panel + (QP ? (size_t)ring_nk * 256 * RG_KB * sizeof(u16) : 0); }
};

// ---- the scaled f16 images --------------------------------------------------------------------------------------------------------
// x -> RN_f16(x * s), s a power of two that puts the largest |element| into [2^13, 2^14) (clamped to 2^+-40), so neither overflow
// nor the fp16 subnormal range matters: element error <= 2^-11 |x| + F16_FLUSH / s, where the second term assumes the worst
// (subnormal results flushed to zero). bits = the float bits of that largest |element| or of a bound on it (sign bit clear);
// zero / subnormal and inf / NaN select s = 1.
#define F16_FLUSH 6.103515625e-05f        // 2^-14, the smallest normal f16
__host__ __device__ inline float f16_scale_for(uint32_t bits) {
    const int e = (int)(bits >> 23);                 // biased exponent; 0 = zero/subnormal, 255 = inf/NaN
    if (e == 0 || e == 255) return 1.0f;
    int k = 13 - (e - 127);                          // value * 2^k in [2^13, 2^14)
    k = k > 40 ? 40 : (k < -40 ? -40 : k);
    return __builtin_bit_cast(float, (uint32_t)(127 + k) << 23);
}
// The layout k_knn_l2_ring16 streams: [F16T_ROWS-row tile][F16T_KB-k slice][row][4 x 16-byte segments], i.e. every (tile, slice) is
// one contiguous 16 KB block that already is the LDS image: segment p of row r holds logical segment p ^ f16t_swizzle(r), which
// makes the fragment reads of both MFMA shapes conflict-free. A DMA instruction then copies 1 KB of consecutive, fully used
// 128-byte lines; with a row-major image each slice touches only half of every line and the other half is fetched again one
// slice later. Rows are padded to whole tiles; nk = slices per row.
#define F16T_ROWS 256
#define F16T_KB 32
#define F16T_BLOCK (F16T_ROWS * F16T_KB)             // halves per (tile, slice) block
__host__ __device__ inline size_t f16t_halves(size_t n_tiles, int nk) { return n_tiles * nk * F16T_BLOCK; }
__device__ __forceinline__ int f16t_swizzle(int r) { return (0x78 >> (2 * ((r >> 2) & 3))) & 3; }      // F[(r >> 2) & 3], F = {0,2,3,1}
// index of (row r of tile `tile`, logical column kc * F16T_KB + 8 seg + e): f16t_row(tile, r, nk, kc) + ((seg ^ f16t_swizzle(r)) << 3) + e
__device__ __forceinline__ size_t f16t_row(size_t tile, int r, int nk, int kc) { return ((tile * nk + kc) * F16T_ROWS + r) * F16T_KB; }
// half h (0 .. nk * F16T_KB - 1, in the order they are stored) of image row `row`: for sums that do not care about the order
__device__ __forceinline__ size_t f16t_stored(unsigned row, int nk, unsigned h) { return f16t_row(row / F16T_ROWS, row % F16T_ROWS, nk, h / F16T_KB) + h % F16T_KB; }

struct VerifyParams {
    float ku;         // 1.01 * K * u : relative error bound of a K-term fp32 functor sum (u = 2^-24)
    float dot_rel;    // bound on |approx(q.c) - q.c| / (|q||c|) of the candidate kernel (f32 fma chain: ku; bf16x3: see k_knn_l2_mfma16)
    float cmax2;      // max |c|^2 over the codebook (L2 only)
    float dabs_c;     // f16 candidates: worst-case absolute error of one codebook element (2^-14 / scale), else 0
    const float* dabs_q;   // f16 candidates: the same for the query batch (device scalar), else nullptr
    float sqrt_dim;   // sqrt(dim_pad)
    float cn_acc;     // k_knn_l2_ring16 adds |c|^2 through the accumulator: extra 1.01 (K+1) 2^-23 |c|max^2 on the score, else 0
};
// absolute part of the candidate kernel's dot-product error: sum |dq_i c_i| + |q_i dc_i| + |dq_i dc_i| with |dq_i| <= dq, |dc_i| <= dc
__device__ __forceinline__ float knn_abs_err(const VerifyParams& vp, float qn2) {
    if (!vp.dabs_q) return 0.f;
    const float dq = vp.dabs_q[0], dc = vp.dabs_c;
    return 1.01f * (vp.sqrt_dim * (dq * sqrtf(vp.cmax2) + dc * sqrtf(qn2)) + vp.sqrt_dim * vp.sqrt_dim * dq * dc);
}
#define KNN_U 5.9604645e-08f
// eps_s: the error bound of a candidate score for a query with |q|^2 = qn2 (k_knn_rerank's proof comment derives it). _raw is the
// expression as evaluated (k_knn_rerank, whose slack and proof margins absorb its rounding); the lower-bound proofs
// (k_knn_rerank_hell, k_hell_tau, thr_tau_of) take it rounded up
__device__ __forceinline__ float knn_eps_s_raw(const VerifyParams& vp, float qn2) {
    return 17.f * KNN_U * vp.cmax2 + (2.f * vp.dot_rel + 2.f * KNN_U) * sqrtf(qn2 * vp.cmax2) + 2.f * knn_abs_err(vp, qn2) + vp.cn_acc * vp.cmax2;
}
__device__ __forceinline__ float knn_eps_s(const VerifyParams& vp, float qn2) { return knn_eps_s_raw(vp, qn2) * 1.00001f; }
// |x|^2 of a row of dim floats by a wave: lane l adds the elements l, l + 64, ..., then a tree sum
__device__ __forceinline__ float wave_norm2(const float* __restrict__ x, int dim, int lane) {
    float s = 0.f;
    for (int i = lane; i < dim; i += 64) { const float v = x[i]; s += v * v; }
    return wave_sum_f(s);
}

// error model of the candidate scores for the proofs (k_knn_rerank, k_knn_rerank_hell, k_hell_tau, k_thr_tau). mode as in KnnPlan;
// f16: qsc = the query batch's scalars (k_to_f16), cn_acc = the caller charges |c|^2 carried through the accumulator
VerifyParams knn_verify_params(const ismhip_codebook* xb, int dim_pad, int mode, const uint32_t* qsc, bool cn_acc) {
    VerifyParams vp;
    vp.ku = 1.01f * (float)dim_pad * KNN_U;
    // relative part of the candidate kernel's dot error (see the kernels): representation + accumulation (<= 2^-23 per add, any order)
    vp.dot_rel = mode == 0 ? (2.002f * 4.8828125e-04f + 1.01f * (float)dim_pad * 1.1920929e-07f)
               : mode == 1 ? (3.1f * 1.52587890625e-05f + 1.01f * 3.f * (float)dim_pad * 1.1920929e-07f) : vp.ku;
    vp.cmax2 = xb->max_norm2;
    vp.dabs_c = mode == 0 ? F16_FLUSH / xb->f16_scale : 0.f;
    vp.dabs_q = mode == 0 ? (const float*)(qsc + 2) : nullptr;
    vp.sqrt_dim = sqrtf((float)dim_pad);
    vp.cn_acc = mode == 0 && cn_acc ? 1.01f * (float)(dim_pad + 1) * 1.1920929e-07f : 0.f;
    return vp;
}

// tau_q such that functor(q, c) < thr  =>  score(c) <= tau_q. A row with score s has D >= |q|^2 (1 - 16u) + s - eps_s and functor
// value >= D (1 - ku) (k_knn_rerank, k_hell_tau with dk := thr); the extra (dim/64 + 8) u |q|^2 covers the rounding of this wave's
// own |q|^2 sum. A non-finite tau (inf / NaN in the batch) lists every row: the cap then sends the query to the exact scan.
__device__ __forceinline__ float thr_tau_of(float thr, float qn2, int dim, const VerifyParams& vp) {
    const float eps_s = knn_eps_s(vp, qn2);
    float t = thr * (1.f + 2.f * vp.ku) - qn2 * (1.f - 16.f * KNN_U) + eps_s + 8.f * KNN_U * (qn2 + vp.cmax2 + thr)
            + (float)(dim / 64 + 8) * KNN_U * qn2;
    if (!(fabsf(t) < __builtin_inff())) t = __builtin_inff();
    return t;
}

// ---- the slot proofs of the squared-L2 re-rank kernels, shared with the kernel that seeds stage 2 (k_knn_seed_thr) ------------------
// k_knn_rerank (scores approximate the functor value; the derivation is at its proof): a slot whose dropped scores are all >= bnd
// cannot hold a row that beats or ties the k-th exact value dk
__device__ __forceinline__ bool knn_l2_slot_proven(float dk, float bnd, float qn2, const VerifyParams& vp) {
    const float eps_s = knn_eps_s_raw(vp, qn2);
    const float rhs = qn2 * (1.f - 16.f * KNN_U) + bnd - eps_s;
    return dk < rhs - vp.ku * fabsf(rhs) - 1e-37f;
}
// k_knn_rerank_pca (scores on a rotated, truncated image are lower-bound pieces; derivation at that kernel): what LB(s) needs of one
// query -- |q^|^2 of its image row, the accumulation error eps_s of its scores, dlt = delta_q + delta_c -- and of the image
struct PcaLb { float qn2h, eps_s, dlt, inv_sig2; };
__device__ __forceinline__ float pca_lb_of(const PcaLb& b, float s) {
    float L = b.qn2h * (1.f - 16.f * KNN_U) + s - b.eps_s;
    L -= 4.f * KNN_U * (b.qn2h + fabsf(s));                            // rounding of the two additions above
    if (!(L > 0.f)) return 0.f;                                        // also NaN
    const float t = sqrtf(L) * (1.f - 4.f * KNN_U) - b.dlt;
    if (!(t > 0.f)) return 0.f;
    return t * t * b.inv_sig2 * (1.f - 8.f * KNN_U);
}
__device__ __forceinline__ bool pca_slot_proven(float dk, float bnd, const PcaLb& b, float ku) { return dk < pca_lb_of(b, bnd) * (1.f - ku) - 1e-37f; }

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
// ---- the queue of unproven work: filled by the re-rank kernels (knn_rerank.hip), emptied by the exact scan (knn_scan.hip) -----------
#define KNN_MERGE_KEEP 16         // candidates k_knn_merge_splits keeps of all the splits of a query
#define KNN_HELL_CPL 4            // candidates per lane of k_knn_rerank_hell (256 per query)
// The 16-word counter block at the head of the queue scratch (flag_count of the kernels), zeroed before every search:
enum KnnCounter {
    KNN_CNT_QUERIES = 0, KNN_CNT_ITEMS = 1,   // the queue: unproven queries, their (query, slot) work items (ctx->knn_stats reads both)
    KNN_CNT_QSC = 4,                          // f16 mode, three words: absmax bits of the query batch, -2 / (s_q s_c), 2^-14 / s_q (k_to_f16)
    KNN_CNT_NEGATIVE = 12,                    // chi-square: some query element is negative (k_any_negative)
    KNN_CNT_WORDS = 16
};

// the conditions under which the searches run on the matrix cores (shared by ismhip_knn and ismhip_knn_threshold): a launch big
// enough to fill the chip, whole 16-byte chunks per descriptor, no A/B override of the candidate kernel
bool knn_matrix_gate(const ismhip_ctx* ctx, const ismhip_codebook* cb, int nq) {
    return ctx->knn_mode == 0 && ctx->knn_t == 0 && nq >= 256 && cb->n_words >= 1024 && cb->dim % 4 == 0;
}

}  // namespace

// ---- the host-side records of a search (they cross units: every type in them has a name with linkage) -------------------------------------
// Slot -> rows layout of the exact scan, chosen by knn_plan and decoded by k_knn_fallback (its wr_rows). The two positive values ARE
// the rows per wave-row block of the 32x32 MFMA tile (MI * 32): 64 on the 128-row tile, 128 on the 256-row tile.
enum KnnFbLayout { KNN_FB_TILE128 = 64, KNN_FB_TILE256 = 128, KNN_FB_RING = -1, KNN_FB_ALL = -2, KNN_FB_RING_HALF = -3 };
// How the slots of ONE search map to rows: its plan's tiles per split, tile count and tile rows, the slot -> rows layout (wr_rows: a
// KnnFbLayout value) and, for a ranged search (qrange, below), the number of splits each query's own range was cut into.
struct KnnSlotRows { int tiles_per_split, n_tiles, tile_rows, wr_rows, n_splits; };
// A queue of unproven work that several searches may fill and ONE exact scan empties: counter block, a record per unproven query, an item
// per failing slot, the scan's per-item results (layout: knn_scan.hip), the slot -> rows layout each search (chunk 0 / 1) leaves behind
struct KnnQueue { uint32_t *count, *qrec, *items; unsigned long long* item_out; size_t q_items; KnnSlotRows desc[2]; };
// stage1 != nullptr: FIRST stage of the two-stage search -- candidates + exact re-rank + proof only; the unproven queries are
// left in the queue (*stage1: its counter block, records and items) for the caller instead of going to the exact scan; with them, how
// the stage cut the codebook: item slot b belongs to split b / slots, and split s swept the rows [s, s + 1) * rows_per_split.
struct KnnStage1 { KnnQueue queue; int n_splits, slots, rows_per_split; };
// A RANGED search (KnnCandArgs::qrange below), chunk `chunk` of the run_knn_stage2_lists driver: the queries are the entries q_base ...
// of the concatenated failure lists (live[i] == ~0u: padding between two lists), every group of 256 sweeps its own row range (shortest /
// longest: rows_min / rows_max; all a request for the plan alone fills in), and what stays unproven goes to `queue`, not to a scan.
// known_dk: per query, an exact value its k-th best row is known not to exceed (KnnQueueTag, knn_rerank.hip: the ranged search's proofs).
struct KnnRanged { const int* qrange; const uint32_t* live; KnnQueue* queue; int q_base, chunk, rows_min, rows_max; const float* known_dk; };
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
    const KnnRanged* ranged = nullptr; // a ranged search; seed_dk only sets its start thresholds, ranged->known_dk enters its proofs
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
    bool big_tile, half, qpanel2, pca, merged, prepass, seeded, join, ranged, split_major;
    int slots, ring_nk;         // lane slots per codebook split (squared L2), 32-k slices per row of the tiled images
    int n_qt, n_splits, tiles_per_split, cand_per_split, n_cand, n_bound;
    int fb_tiles_per_split; KnnFbLayout fb_layout;   // exact scan: tiles per slot's split and the slot -> rows layout
    size_t lds, lds_cap;        // dynamic LDS of this launch, and the largest any launch of the kernel uses
};
// One search in flight: what the phases of run_knn hand to each other, the carve-up of its scratch (knn_carve_scratch) included.
struct KnnRun {
    ismhip_ctx* ctx; const ismhip_codebook *cb, *xb; const PcaImage* PI; const KnnRequest* rq; KnnPlan p;
    int metric, nq, k, T;
    const float* qq; int ldq;            // the query rows as the kernels read them (padded to dim_pad when dim is not)
    u16 *q_hi, *q_lo;                    // 16-bit query images (knn_query_images; nullptr: the candidate kernel reads the rows themselves)
    const float *qn2, *qn2h;             // rotated image made on the f16 matrix cores: |q|^2 and the image rows' sums of squares, behind the image (else nullptr)
    float *cand_val, *cand_bound; int* cand_idx; int n_cand, n_bound;      // candidate lists and slot bounds (after a merge: the folded slot)
    uint32_t *counters, *qsc;            // the search's own counter block (KnnCounter) and, in it, the f16 scalars of the query batch
    KnnQueue queue;                      // the queue of unproven work: carved behind the counter block, or the request's shared queue
};

// ---- knn.hip: one search (T = candidates kept per lane slot, 1 .. 4), and the images of other searches' query batches ----------------------
KnnPlan knn_plan(const ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, int k, int T, const KnnRequest& rq);
int run_knn(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, int k, int T, int32_t* idx_out, float* dist_out, const KnnRequest& rq = KnnRequest());
// sq[nq x dim_pad] = sqrt of the query rows (zero padded; 4 more bytes behind them hold the flag); negative = some element is
// negative or NaN, read back: the call synchronises the stream
int knn_sqrt_queries(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, float* sq, bool& negative);
// An f16 EMIT sweep (chi-square stage 2, radius search, large K) is three steps on the stream: knn_f16_emit_image makes the f16
// image qimg of the n query rows qv (row stride ldv, n_pad = n rounded up to 128; sc = the batch's f16 scalars, zeroed by the caller),
// the caller launches its tau kernel with knn_verify_params(xb, dim_pad, 0, sc, cn_acc), knn_mfma16_emit lists the rows.
int knn_f16_emit_image(ismhip_ctx* ctx, const ismhip_codebook* cb, const ismhip_codebook* xb, const float* qv, int n, int ldv, int n_pad,
                       uint32_t* sc, u16* qimg);
// pca.hip: the rotated f16 image of a query batch; when ism_pca_split_queries (the f16 matrix-core route) it also leaves |q|^2 of the rows
// and the sums of squares of the image rows as stored in qn2 / qn2h [nq rounded up to 256], which the proofs then read (PcaVerify)
int ism_pca_rotate_queries(ismhip_ctx* ctx, const ismhip_codebook* cb, const PcaImage* P, const float* q, int nq, int ldq, unsigned short* dst, float* qn2, float* qn2h);
bool ism_pca_split_queries(const ismhip_ctx* ctx, const PcaImage* P);
// ---- knn_rerank.hip (phases of run_knn) ----------------------------------------------------------------------------------------------------
// thr0[nq] = the start thresholds of a seeded search (k_knn_seed_thr; needs the query image and, on the original image, its scalars)
int knn_seed_thresholds(KnnRun& r, const float* out_scale, float* thr0);
// folds many splits into one slot first (it becomes the run's candidate list: r.cand_*, r.n_cand, r.n_bound change), then: exact functor
// values of the candidates that matter, the k best, and the proof; what it cannot prove is queued
int knn_rerank_prove(KnnRun& r, int32_t* idx_out, float* dist_out);
// ---- knn_scan.hip: the exact scan and THE layout of its queue --------------------------------------------------------------------------------
// bytes of a queue for n_queries queries with q_items slots between them (results of up to k rows per item), and its carve-up
size_t knn_queue_bytes(size_t n_queries, size_t q_items, int k);
KnnQueue knn_queue_carve(void* mem, size_t n_queries, size_t q_items);
// exact scan of the queued slots' rows into the unproven queries' results: one scan and one merge launch for a queue, whichever
// searches filled it (q, idx_out, dist_out are indexed by the queue's query numbers)
int knn_scan_queue(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int k, const float* q, int ldq, const KnnQueue& Q, const int* qrange, int32_t* idx_out, float* dist_out);
// ---- knn_wide.hip: rows longer than KNN_TERMS floats, up to ISMHIP_KNN_MAX_DIM -- an exact scan of its own (none of the stages above) ---------
int run_knn_wide(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, int k, int32_t* idx_out, float* dist_out);
// ---- knn_two_stage.hip: the two-stage drivers; chi-square: taken = false: not histogram data, the caller takes the VALU kernel ------------
int run_knn_two_stage(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, int k, int32_t* idx_out, float* dist_out);
int run_knn_chi2_hellinger(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, int k, int32_t* idx_out, float* dist_out, bool& taken);

// ---- the 16-bit candidate kernels: knn_ring16.hip, knn_mfma16.hip ---------------------------------------------------------------------
// what k_knn_l2_ring16 and k_knn_l2_mfma16 both take, under the names of their parameter lists (the ring has no wl / ql)
struct KnnCandArgs {
    const u16 *wh, *wl; const float* word_norm; int n_tiles_m, ld, k_steps;
    const u16 *qh, *ql; int nq; const float* out_scale; int tiles_per_split, n_splits;
    float* cand_val; int* cand_idx; int cand_stride; float* cand_bound; int bound_stride;
    const int* qrange;      // ranged search (knn_range_split), else nullptr: every query sweeps the tiles [0, n_tiles_m)
    int split_major;        // ring kernel: the split is the slow index of the block -> (query tile, split) map (KnnPlan::split_major)
};
// A RANGED search (stage 2 of the two-stage search on per-split failure lists, knn_two_stage.hip): the queries come in groups of 256 and group
// g sweeps only the codeword rows [qrange[4 g], qrange[4 g + 1]) (multiples of 256); qrange[4 g + 2] = the list the group belongs to,
// qrange[4 g + 3] = the first query of that list. The tiles of a range are dealt to the launch's splits evenly (never an empty split:
// the host keeps n_splits <= the tiles of the shortest range), and rows stay GLOBAL rows: only the sweep is shorter.
__host__ __device__ inline void knn_range_split(int lo, int hi, int split, int n_splits, int& mt0, int& mt1) {
    const long long len = hi - lo;
    mt0 = lo + (int)(len * split / n_splits); mt1 = lo + (int)(len * (split + 1) / n_splits);
}
// the instance for T candidates per slot (1 .. 4, else nullptr): WR x 128 codeword rows per tile, QP = 2 with the resident query
// panel, PRE = 1 the sampling pre-pass, RNG = 1 the ranged sweep (KnnCandArgs::qrange; built for T = 4, QP = 0 only)
const void* knn_ring16_kernel(int T, int WR, int QP, int PRE = 0, int RNG = 0);
// one candidate launch of kern = knn_ring16_kernel(T, ...). thr0 != nullptr: every lane slot of query i starts from the threshold
// thr0[i] (accumulator units) instead of -inf. pre_step > 0: the sampling pre-pass over every pre_step-th tile runs first and leaves
// those thresholds in thr0[nq rounded up to 256], relaxed by pre_relax; pre_step == 0: the caller has written thr0[nq]
int knn_ring16_launch(ismhip_ctx* ctx, int T, const void* kern, unsigned grid, int threads, size_t lds, KnnCandArgs a,
                      unsigned int* stream_clock, float* thr0, int pre_step, float pre_relax);
// the candidate instances: bf16x3 on the 256 x 256 or the 128 x 128 tile, f16 on the 128 x 128 tile (nullptr: not built)
const void* knn_mfma16_kernel(int T, int mode, bool big_tile);
int knn_mfma16_launch(ismhip_ctx* ctx, const void* kern, unsigned grid, int threads, size_t lds, KnnCandArgs a,
                      const float* emit_tau, uint32_t* emit_cnt, uint32_t* emit_list, int emit_cap);
// k_knn_l2_mfma16<EMIT> over the f16 image qimg (knn_f16_emit_image): every row with score <= tau[q] is appended to
// rows[q * cap ...] (count in emit_cnt[q])
int knn_mfma16_emit(ismhip_ctx* ctx, const ismhip_codebook* cb, const ismhip_codebook* xb, int n, int n_pad, const uint32_t* sc, const u16* qimg,
                    const float* tau, uint32_t* emit_cnt, uint32_t* rows, int cap);

// ---- knn_cand.hip: the f32 MFMA and the chi-square candidate kernels, T = 1 .. 4 -------------------------------------------------------
int knn_l2_f32_launch(ismhip_ctx* ctx, int T, unsigned grid, const ismhip_codebook* cb, const float* q, int nq, int ldq, int tiles_per_split, int n_splits,
                      float* cand_val, int* cand_idx, int n_cand, float* cand_bound, int n_bound);
// (with k_any_negative over the batch into q_negative, zeroed by the caller, when the codebook has no negative element)
int knn_chi2_launch(ismhip_ctx* ctx, int T, int n_qt, const ismhip_codebook* cb, const float* q, int nq, int ldq, uint32_t* q_negative, int tiles_per_split, int n_splits,
                    float* cand_val, int* cand_idx, int n_cand, float* cand_bound, int n_bound);

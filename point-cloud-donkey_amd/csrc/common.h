// common.h — internal definitions shared by the HIP translation units of libismhip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "../../include/ismhip.h"

#define ISM_WAVE 64

// ---- per-object uniform grid (device-resident) ------------------------------------------------
#define ISM_GRID_MAXDIM 32                      // cells per axis (cell edge doubles until the object fits)
#define ISM_GRID_MAXCELLS (ISM_GRID_MAXDIM * ISM_GRID_MAXDIM * ISM_GRID_MAXDIM)
#define ISM_GRID_STRIDE (ISM_GRID_MAXCELLS + 1) // cell_start entries reserved per object

// The grid is ANISOTROPIC: a ball query walks one contiguous x-run of points per (y,z) cell row, so the y/z edge sets the
// number of rows (per-row set-up, ragged row ends) while the x edge only sets how tightly the chord of the ball clips a row.
// x cells are therefore ISM_GRID_XFRAC times finer than y/z cells: fewer, longer rows AND less over-fetch at their ends.
#define ISM_GRID_XFRAC 3
struct GridMeta {
    float minv[3];
    float cell[3];      // edge actually used per axis (>= requested)
    float inv_cell[3];
    int   dim[3];
    float centroid[3];
    uint32_t n_finite;
};

struct ismhip_cloud {
    int n_obj = 0;
    uint32_t n_pts = 0;
    uint32_t max_pts = 0;                 // largest object
    std::vector<uint32_t> pt_off_h;
    uint32_t* pt_off = nullptr;           // [n_obj+1]
    // caller's arrays (borrowed, original order)
    const float *x = nullptr, *y = nullptr, *z = nullptr, *nx = nullptr, *ny = nullptr, *nz = nullptr;
    const uint32_t* rgba = nullptr;
    // cell-sorted packed copies (owned): one 16-byte record per point and array, so that a candidate costs ONE coalesced
    // global_load_dwordx4 (and a queued neighbour one 16-byte gather for its normal) instead of three dword loads
    float4* sp4 = nullptr;                // (x, y, z, bits of the object-local original index)
    float4* sn4 = nullptr;                // (nx, ny, nz, 0)
    float4* slab4 = nullptr;              // normalised CIELab (L, a, b, 0), only with rgba
    // scratch of the five-kernel grid build, allocated when a batch first takes it (grid.hip)
    uint32_t* cell_of_pt = nullptr;       // scratch: cell id per original point
    uint32_t* rank_of_pt = nullptr;       // scratch: arrival rank inside the cell
    uint32_t* members = nullptr;          // scratch: object-local original indices grouped by cell in arrival order
    GridMeta* meta = nullptr;             // [n_obj]
    uint32_t* cell_start = nullptr;       // [n_obj * ISM_GRID_STRIDE]
    float requested_cell = 0.f;
    // keypoints in cell order (grid.hip: ism_kp_order): object-local keypoint indices of the last keypoint set described on this cloud,
    // sorted by cell id, so that the waves of a workgroup sweep overlapping balls. Scheduling only: any permutation gives the same results.
    uint32_t* kp_perm = nullptr;          // [kp_perm_off.back()]
    size_t kp_perm_cap = 0;
    const float* kp_perm_key = nullptr;   // the kpx pointer the order was built from (nullptr: none)
    std::vector<uint32_t> kp_perm_off;    // and its offsets
    // CoSPAIR's colour codes (cospair.hip), cell-sorted like sp4: the three colour histogram indices of every point, 5 bits each. Built by
    // the first ismhip_cospair on this cloud (cospair_code_valid), kept for the later ones; the allocation is recycled with the cloud.
    uint16_t* cospair_code = nullptr;     // [cospair_code_cap]
    size_t cospair_code_cap = 0;
    bool cospair_code_valid = false;
    // capacities of the owned allocations (clouds are recycled through ismhip_ctx::cloud_pool)
    size_t cap_pts = 0; int cap_obj = 0; bool cap_color = false;
};

// A rotated, truncated f16 image of a codebook. Rows of R = the m leading eigenvectors of the codebook's second-moment matrix
// (orthonormal up to the error folded into inv_sig2), so |R (q - c)|^2 <= sigma_max(R)^2 |q - c|^2: a score over the leading m rotated
// coordinates is a LOWER bound of the functor value.
struct PcaImage {
    int m = 0;                       // leading rotated coordinates kept (multiple of 32); 0: not built
    float* R = nullptr;              // [m x dim_pad] fp32, row j = j-th basis vector (zero in the padding columns)
    unsigned short* f16t = nullptr;  // f16 image of R c (scale sc) in the ring kernel's streaming layout [tile][m/32][256][32]
    float* cn_scaled = nullptr;      // [n_words_pad + 256] |c^|^2 / out_scale of that image (-inf for padding rows): the ring kernel's C operand
    float* osc = nullptr;            // device scalars: [0] out_scale = -2 / (sq sc)
    float sq = 1.f, sc = 1.f;        // power-of-two f16 scales of the query / codebook images (the query scale is FIXED per codebook)
    float cmax2 = 0.f;               // max |c^|^2 over the real rows (c^ = image / sc)
    float inv_sig2 = 1.f;            // 1 / (upper bound of sigma_max(R)^2), rounded down
    float d_rel = 0.f;               // |x^ - R x|_2 <= d_rel |x|_2 + dq_abs (queries) / dc_abs (codewords): rotation + f16 rounding
    float dq_abs = 0.f, dc_abs = 0.f;
    // the query batches' rotation on the f16 matrix cores (pca.hip, k_rotate_split16): R split into two f16 halves, its own error constants
    unsigned short* R16 = nullptr;   // [dim_pad/32][m/16][hi, lo][64 lanes][8] f16(R 2^r16_shift) and f16 of what that leaves, in MFMA A-fragment order
    int r16_shift = 0;
    float dq_rel16 = 0.f, dq_abs16 = 0.f;   // |x^ - R x|_2 <= dq_rel16 |x|_2 + dq_abs16 for a query image made from R16
    float resid2 = 0.f;              // mean second moment per codeword OUTSIDE the leading m coordinates (the pre-pass relaxes its start thresholds by it)
    float energy = 0.f;              // share of the codebook's second moment in the leading m coordinates (diagnostic)
};

struct ismhip_codebook {
    int n_words = 0, dim = 0, dim_pad = 0, n_votes = 0, max_votes = 0, n_classes = 0;
    float* words = nullptr;          // [n_words_pad * dim_pad] row-major, zero padded (MFMA tile friendly)
    int n_words_pad = 0;
    float* word_norm = nullptr;      // [n_words_pad] squared L2 norm (+inf for padding rows)
    unsigned short* words_bf16_hi = nullptr;   // [n_words_pad * dim_pad] RN_bf16(word)            (one allocation holds hi then lo)
    unsigned short* words_bf16_lo = nullptr;   // [n_words_pad * dim_pad] RN_bf16(word - hi)
    unsigned short* words_f16 = nullptr;       // [n_words_pad * dim_pad] RN_f16(word * f16_scale)  (same allocation)
    unsigned short* words_f16t = nullptr;      // the f16 image in k_knn_l2_ring16's streaming layout (k_to_f16_tiled), own allocation
    int ld16 = 0;                    // row stride (halves) of the 16-bit images: dim rounded up to 64, zero padded
    float f16_scale = 1.f;           // power of two: largest |element| * f16_scale in [2^13, 2^14)
    bool words_nonneg = false;       // no negative (or NaN) element: k_knn_chi2 may drop the functor's "sum > 0" test (see there)
    float max_norm2 = 0.f;           // max squared norm over the real rows (bounds the fp32 contraction error of kNN)
    float* word_weight = nullptr;    // [n_words]
    uint32_t* vote_off = nullptr;    // [n_words+1]
    float* vote_xyz = nullptr;       // [n_votes*3]
    float* vote_weight = nullptr;    // [n_votes]
    float* vote_class_weight = nullptr;
    uint32_t* vote_class = nullptr;
    uint32_t* vote_instance = nullptr;
    float* vote_bbox_quat = nullptr; // [n_votes*4]
    float* vote_bbox_size = nullptr; // [n_votes*3]
    float* class_sigma = nullptr;    // [n_classes]
    uint32_t* word_class = nullptr;  // [n_words] Codeword::getClassId
    float* word_keypoint = nullptr;  // [n_words*3] Codeword::getFeaturePosition (ismhip_codebook_set_word_keypoint; the RANSAC vote filter's training keypoints)
    // chi-square candidates on the matrix cores (Hellinger lower bound, k_knn_rerank_hell): a shadow codebook that owns the 16-bit
    // images, norms and scales of sqrt(words); its fp32 words are not kept. Only for codebooks without negative / NaN elements.
    ismhip_codebook* chi_shadow = nullptr;
    uint32_t* shadow_perm = nullptr; // (in the shadow) [n_words] codebook row of every shadow row
    // ---- rotated, truncated images of the squared-L2 search (pca.hip; m == 0: not built) ---------------------------------------------
    // pca: the stage-1 image (leading coordinates that hold 97 % of the second moment); pca2: a longer one (99.7 %) for stage 2, the
    // queries whose stage-1 proof failed -- both cut from the same eigenbasis
    PcaImage pca, pca2;
    // ---- the 0/1 image of the exact binary search (knn_binary.hip; ismhip_codebook_make_binary), nullptr: not built --------------------
    int8_t* bin_words = nullptr;     // [n_words_pad x bin_ld] 0 / 1, zero padded
    int32_t* bin_norm = nullptr;     // [n_words_pad] ones per row (dim + 1 for padding rows)
    int bin_ld = 0, bin_shift = 0;   // row stride in bytes; row bits of the (distance, row) key
};

struct TimerAcc {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms = 0.0;
    int64_t launches = 0;
};

struct ismhip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    bool timers_on = false;
    std::map<std::string, TimerAcc> timers;
    std::vector<hipEvent_t> event_pool;
    // grow-only scratch slots
    struct Slot { void* p = nullptr; size_t bytes = 0; };
    std::map<int, Slot> scratch;
    // LUTs for RGB->Lab (device)
    float* lut_srgb = nullptr;   // [256]
    float* lut_sxyz = nullptr;   // [4000]
    // destroyed clouds keep their device allocations here for the next ismhip_cloud_create (no hipMalloc/hipFree per batch)
    std::vector<ismhip_cloud*> cloud_pool;
    uint32_t* truncated_d = nullptr;  // device counter: maxima dropped by the per-class / per-object caps of find_maxima / hough3d_maxima (ismhip_sync reports and clears it)
    unsigned long long* ransac_counters_d = nullptr;   // device counters of the RANSAC vote filter: clusters, clusters kept, hypotheses needed, hypotheses evaluated (since the last ismhip_timers_reset)
    uint32_t knn_stats[2] = {0, 0};   // last ismhip_knn: {queries, (query,slot) items} sent to the exact fallback (valid with timers on, after a sync)
    std::set<const void*> attr_done;  // kernels whose MaxDynamicSharedMemorySize attribute has been raised on THIS ctx's device
    uint32_t knn_stage2_queries = 0;  // last two-stage ismhip_knn: queries the T = 2 stage could not prove (searched again with T = 4)
    uint32_t knn_stage2_list_entries = 0;   // last two-stage ismhip_knn: sum of the per-split failure list sizes (a query counts once per split it failed in; 0: none made)
    uint32_t knn_stage2_ranged = 0;   // two-stage searches whose stage 2 ran on the per-split lists (tests / bench)
    uint32_t knn_seed_launches = 0;   // candidate launches that started from k_knn_seed_thr's thresholds (tests)
    bool knn_stage2_splits = true;    // env ISMHIP_KNN_STAGE2_SPLITS=0: stage 2 searches the whole codebook again for every query instead of the splits whose proof failed (A/B runs, tests; same results)
    bool knn_stage2_seed = true;      // env ISMHIP_KNN_STAGE2_SEED=0: stage 2 starts its candidate lists cold, with T = 4 (A/B runs, tests; same results)
    bool knn_two_stage = true;   // env ISMHIP_KNN_TWOSTAGE=0: single-stage T = 4 search (A/B runs)
    bool knn_join = true;        // env ISMHIP_KNN_JOIN=0: every workgroup of the ring kernel sweeps its split from the first tile (A/B runs); default: joined streams
    bool knn_qpanel2 = true;     // env ISMHIP_KNN_QPANEL2=0: stage 1 on <= 160 rotated coordinates WITHOUT the 256-query panel resident in LDS (A/B runs; default on: 27.5 -> 25.4 ms per bench launch)
    bool knn_half = false;       // env ISMHIP_KNN_HALF=1: the ring kernel on 128 x 256 tiles, two workgroups per CU (A/B runs; stage-2 chunks of 4096-32767 queries take them anyway)
    int knn_splits = 0;          // env ISMHIP_KNN_SPLITS: force the number of codebook splits of the squared-L2 candidate kernels (A/B runs)
    int knn_split_major = -1;    // env ISMHIP_KNN_SPLIT_MAJOR = 0 | 1: the ring kernel's block -> (query tile, split) map with the split as the fast / slow index for every launch (A/B runs; default: knn_plan's rule)
    int knn_t = 0;               // env ISMHIP_KNN_T = 1 | 2 | 3: candidates kept per slot (default 4 on the 16-bit paths); fewer = cheaper epilogue, more unproven slots
    bool xcd_map = true;         // env ISMHIP_XCD_MAP=0: per-object kernels on the plain object-major block order instead of the XCD-local map (A/B runs)
    bool grid_fused = true;      // env ISMHIP_GRID_FUSED=0: ismhip_cloud_create on the five-kernel grid build instead of one workgroup per object (A/B runs, tests; same bytes)
    bool kp_order = true;        // env ISMHIP_KP_ORDER=0: LRF and SHOT take the keypoints in the caller's order instead of cell order (A/B runs; same results)
    float grid_xfrac = 0.f;      // env ISMHIP_GRID_XFRAC: x cells this many times finer than y/z cells (default ISM_GRID_XFRAC; A/B runs)
    int shot_var = 0;            // env ISMHIP_SHOT_VAR=2: k_shot on the contiguous candidate sweep instead of 16 interleaved segments (A/B runs; same histogram)
    bool knn_hell_emit = true;   // env ISMHIP_KNN_HELL_EMIT=0: queries the Hellinger proof leaves open go to the VALU kernel instead of the list-and-evaluate stage (A/B runs)
    bool knn_hellinger = true;   // env ISMHIP_KNN_HELLINGER=0: chi-square candidates by the VALU kernel k_knn_chi2 only (A/B runs)
    int knn_t1 = 2;              // env ISMHIP_KNN_T1 = 1 | 2: candidates kept per lane slot in stage 1 of the two-stage search (A/B runs)
    int knn_pre_step = 32;       // env ISMHIP_KNN_PRE_STEP: the sampling pre-pass sweeps every n-th codeword tile (measured with the resident query panel, kNN ms per bench launch at gamma 1.0: 8 -> 36.4, 16 -> 33.6, 32 -> 33.2; no pre-pass 34.7)
    float knn_pre_gamma = 1.0f;  // env ISMHIP_KNN_PRE_GAMMA: relaxation of the pre-pass start thresholds in units of the truncated second moment (A/B runs)
    bool knn_prepass = true;     // env ISMHIP_KNN_PREPASS=0: stage 1 starts every candidate list cold instead of from the sampled pre-pass threshold (A/B runs)
    int knn_pca_m = -1;          // env ISMHIP_KNN_PCA_M: leading rotated coordinates of the stage-1 image (0 = no rotated image, -1 = chosen from the spectrum)
    bool knn_stage2_t4 = false;       // env ISMHIP_KNN_STAGE2_T4=1: partial stage-2 chunks on the 256-query tiles of full ones (A/B runs)
    bool codebook_light = false;      // set around ismhip_codebook_create by ism_knn_only_codebook: skip the rotated image and the chi-square shadow
    bool knn_rotate_f32 = false;      // env ISMHIP_KNN_ROTATE_F32=1: query batches are rotated on the FP32 matrix cores (k_rotate_f16t) and the re-rank sums their norms itself, as the codebook images always are (A/B runs, tests; same results)
    int knn_pca_m2 = -1;         // env ISMHIP_KNN_PCA_M2: coordinates of the stage-2 image (0 = stage 2 on all dimensions, -1 = chosen from the spectrum)
    uint32_t knn_pca_launches = 0;    // squared-L2 searches whose stage 1 ran on the rotated image (tests / bench)
    uint32_t knn_thr_overflow = 0;        // last ismhip_knn_threshold on the matrix cores: queries whose list exceeded the emit cap (answered by the exact scan)
    uint32_t knn_thr_mfma_launches = 0;   // radius searches (ismhip_knn_threshold) that ran the candidate sweep on the matrix cores (tests / bench)
    bool knn_lk_fast = false;         // env ISMHIP_KNN_LARGE_K_FAST=1: ismhip_knn_large_k takes the certified matrix-core path for chi-square launches too (squared L2 always)
    bool knn_lk_exact = false;        // env ISMHIP_KNN_LARGE_K_EXACT=1: ismhip_knn_large_k takes the exact scan for every query (overrides _FAST)
    float knn_lk_seed_scale = 1.0f;   // env ISMHIP_KNN_LARGE_K_SEED_SCALE: multiplies the fast path's seed (tests: a wrong seed costs time, never correctness)
    uint32_t knn_lk_stats[3] = {0, 0, 0};   // last ismhip_knn_large_k: queries {certified by the fast path, retried, answered by the exact scan}
    uint32_t knn_binary_launches = 0; // ismhip_knn_binary calls that searched (counter "knn_binary_launches"; tests of the host route)
    uint32_t rank_launches = 0;       // ismhip_rank_scores / ismhip_rank_select calls that reached the device (counter "rank_launches"; tests of the host route)
    bool iss3d_wave = false;          // env ISMHIP_ISS3D_MAP=wave: the ISS3D saliency sweep with one wave per query (k_pca_normals' mapping) instead of one thread per query (A/B runs, tests; same bits: the scatter sums are order free, iss3d.hip)
    int mvbb_work_mb = 512;      // env ISMHIP_MVBB_WORK_MB: work buffer of one ismhip_region_mvbb launch in MiB; a batch that needs more takes several launches (tests; same results)
    int knn_mode = 0;            // env ISMHIP_KNN_MODE = f16 (0, default) | bf16x3 (1) | f32 (2): squared-L2 candidate kernel (A/B runs, tests)
};

enum ScratchSlot {
    SCR_KP_OFF = 1, SCR_TIE_LIST, SCR_TIE_REC, SCR_TIE_KEYS, SCR_COUNTERS, SCR_KNN_CAND_IDX, SCR_KNN_CAND_VAL,
    SCR_QNORM, SCR_FPFH_FLAG, SCR_FPFH_LIST, SCR_FPFH_SPFH, SCR_FPFH_LOOKUP, SCR_SLOT_OFF, SCR_CLASS_BW,
    SCR_COMPACT_KEEP, SCR_COMPACT_POS, SCR_OBJ_COUNT, SCR_QPAD, SCR_LRF_COV, SCR_KNN_FLAGS, SCR_KNN_QSPLIT, SCR_MAX_REC, SCR_QNORM2, SCR_KNN_Q2, SCR_KNN_LIST2, SCR_TRAIN, SCR_TRAIN2, SCR_MAX_WORK, SCR_KMEANS, SCR_KNN_CLOCK, SCR_PCA, SCR_KNN_THR0, SCR_KNN_QSQRT, SCR_KNN_HELL_EMIT, SCR_KNN_THR, SCR_KNN_THR2, SCR_TRAIN_ACT, SCR_KNN_LK, SCR_KNN_LK2, SCR_KNN_LK3, SCR_PREFILTER, SCR_RANSAC, SCR_COSPAIR, SCR_KNNB_FLAG, SCR_KNNB_Q, SCR_KNNB_CAND, SCR_RANK, SCR_RANK_KNN, SCR_KNN_LISTS, SCR_KNN_QUEUE, SCR_ISS3D, SCR_CULL_SCALE, SCR_CULL_SELECT, SCR_RIFT, SCR_RIFT_SCALE, SCR_ESF_LIST, SCR_SIFT3D, SCR_SIFT3D_SCALE, SCR_SIFT3D_DRIVER, SCR_MVBB, SCR_CVFH,
    SCR_SIFT3D_OCTAVE    // the last one: octave i of ismhip_sift3d_keypoints takes slot SCR_SIFT3D_OCTAVE + i
};

int  ism_set_err(ismhip_ctx* ctx, int code, const std::string& msg);
void* ism_scratch(ismhip_ctx* ctx, int slot, size_t bytes);   // nullptr on failure (error recorded)
// raises a kernel's MaxDynamicSharedMemorySize to `bytes` once per ctx (attr_done): pass the largest size any launch of that kernel uses
int  ism_lds_cap(ismhip_ctx* ctx, const void* kern, size_t bytes);

// ---- ragged batches (grid.hip): run r of an offsets array off[0 .. n] is [off[r], off[r + 1]) ---------------------------------
// uploads a small host offsets array into a scratch slot; returns device pointer (nullptr on failure)
uint32_t* ism_upload_offsets(ismhip_ctx* ctx, int slot, const uint32_t* off_h, int n);
struct RaggedOffsets { uint32_t max_run = 0, total = 0; uint32_t* dev = nullptr; };   // longest run, off[n], the offsets on the device
enum { RAGGED_START0 = 1,    // off[0] must be 0 (only the entry points that have always insisted on it)
       RAGGED_EMPTY = 2 };   // upload even when every run is empty (the caller launches regardless)
// The offsets array of entry point `name`: refuses it with "<name>: offsets not monotone" (RAGGED_START0: "<name>: offsets must start
// at 0"), measures it and uploads its n + 1 entries into `slot`. When every run is empty nothing is uploaded and dev stays nullptr
// (the callers return before any device work), unless RAGGED_EMPTY is set.
int ism_ragged_offsets(ismhip_ctx* ctx, const std::string& name, const uint32_t* off_h, int n, int slot, int flags, RaggedOffsets* r);
// per-run counts on the device -> offsets on the host (off_h_out[0 .. n], from 0) and the longest run; synchronises the stream
int ism_offsets_from_counts(ismhip_ctx* ctx, int n, const uint32_t* cnt_d, uint32_t* off_h_out, uint32_t* max_run_out);
// the cell-order permutation of a keypoint set on a cloud, or nullptr (see grid.hip)
const uint32_t* ism_kp_order(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h, const uint32_t* ko,
                             const float* kpx, const float* kpy, const float* kpz, uint32_t maxk);

// ISS3D's last step (compact.hip): the points of `cloud` whose mask entry (device, original order) is set, with their colours and their
// index inside the object, in ascending index, object after object; kp_offsets_h_out[n_obj + 1] receives the ranges. More than
// `capacity` of them: ISMHIP_ERR_INVALID, nothing written. Synchronises.
int ism_compact_keypoints(ismhip_ctx* ctx, const std::string& who, const ismhip_cloud* cloud, const uint8_t* mask, uint32_t capacity,
                          float* kx, float* ky, float* kz, uint32_t* krgba, uint32_t* src_index_out, uint32_t* kp_offsets_h_out);

#define ISM_HIP(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e__ = (call);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return ism_set_err((ctx), ISMHIP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

#define ISM_CHECK_LAUNCH(ctx, name)                                                                 \
    do {                                                                                            \
        hipError_t e__ = hipGetLastError();                                                         \
        if (e__ != hipSuccess)                                                                      \
            return ism_set_err((ctx), ISMHIP_ERR_HIP, std::string("launch ") + name + ": " + hipGetErrorString(e__)); \
    } while (0)

// RAII-ish timer scope: records events around a group of launches on the ctx stream
struct TimerScope {
    ismhip_ctx* ctx; const char* name; hipEvent_t a = nullptr, b = nullptr;
    TimerScope(ismhip_ctx* c, const char* n);
    ~TimerScope();
};

// ---- device helpers ---------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// squared distance exactly as FLANN L2_Simple<float> / the oracle: sequential float accumulate.
// The library is compiled with -ffp-contract=off, so no FMA is formed here.
__device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by, float bz) {
    float r = 0.f, d;
    d = ax - bx; r += d * d;
    d = ay - by; r += d * d;
    d = az - bz; r += d * d;
    return r;
}

// Wave-wide sums on the DPP data path. hipcc lowers __shfl_xor to ds_bpermute_b32 (an LDS-crossbar round trip of ~100+
// cycles per step, 6 dependent steps per sum); the DPP sequence below is 6 register-to-register moves + 1 v_readlane.
// All 64 lanes must be active at the call site (they are: every use is wave-uniform). Steps: quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_shr:4, row_shr:8, row_bcast:15, row_bcast:31 -> the total lands in lane 63 (lanes without a source add 0).
template <int CTRL>
__device__ __forceinline__ int dpp_mov0(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }

__device__ __forceinline__ float wave_sum_f(float v) {
    v += __int_as_float(dpp_mov0<0xb1>(__float_as_int(v)));
    v += __int_as_float(dpp_mov0<0x4e>(__float_as_int(v)));
    v += __int_as_float(dpp_mov0<0x114>(__float_as_int(v)));
    v += __int_as_float(dpp_mov0<0x118>(__float_as_int(v)));
    v += __int_as_float(dpp_mov0<0x142>(__float_as_int(v)));
    v += __int_as_float(dpp_mov0<0x143>(__float_as_int(v)));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_sum_i(int v) {
    v += dpp_mov0<0xb1>(v);
    v += dpp_mov0<0x4e>(v);
    v += dpp_mov0<0x114>(v);
    v += dpp_mov0<0x118>(v);
    v += dpp_mov0<0x142>(v);
    v += dpp_mov0<0x143>(v);
    return __builtin_amdgcn_readlane(v, 63);
}
// the same data path for wave-wide minima (lanes without a source see the identity) and for an inclusive prefix sum
// (row_shr 1,2,4,8 scan the 16-lane rows; row_bcast:15 / :31 with row masks 0xa / 0xc carry the row totals forward)
template <int CTRL>
__device__ __forceinline__ int dpp_movi(int ident, int v) { return __builtin_amdgcn_update_dpp(ident, v, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ float wave_min_f(float v) {        // NaN-free inputs or NaN-last semantics of fminf
    const int inf = 0x7f800000;
    v = fminf(v, __int_as_float(dpp_movi<0xb1>(inf, __float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_movi<0x4e>(inf, __float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_movi<0x114>(inf, __float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_movi<0x118>(inf, __float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_movi<0x142>(inf, __float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_movi<0x143>(inf, __float_as_int(v))));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_min_u64(unsigned long long v) {
    const unsigned lo = (unsigned)dpp_movi<CTRL>(-1, (int)(unsigned)(v & 0xffffffffull)), hi = (unsigned)dpp_movi<CTRL>(-1, (int)(unsigned)(v >> 32));
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o < v ? o : v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    v = dpp_min_u64<0xb1>(v); v = dpp_min_u64<0x4e>(v); v = dpp_min_u64<0x114>(v);
    v = dpp_min_u64<0x118>(v); v = dpp_min_u64<0x142>(v); v = dpp_min_u64<0x143>(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}
// wave-wide maxima and the 64-bit sum, the same way (identity: -inf / 0)
__device__ __forceinline__ float wave_max_f(float v) {        // NaN-free inputs or NaN-last semantics of fmaxf
    const int ninf = (int)0xff800000;
    v = fmaxf(v, __int_as_float(dpp_movi<0xb1>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_movi<0x4e>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_movi<0x114>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_movi<0x118>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_movi<0x142>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_movi<0x143>(ninf, __float_as_int(v))));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, (uint32_t)dpp_mov0<0xb1>((int)v)); v = max(v, (uint32_t)dpp_mov0<0x4e>((int)v)); v = max(v, (uint32_t)dpp_mov0<0x114>((int)v));
    v = max(v, (uint32_t)dpp_mov0<0x118>((int)v)); v = max(v, (uint32_t)dpp_mov0<0x142>((int)v)); v = max(v, (uint32_t)dpp_mov0<0x143>((int)v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_mov0_u64(unsigned long long v) {
    const unsigned lo = (unsigned)dpp_mov0<CTRL>((int)(unsigned)(v & 0xffffffffull)), hi = (unsigned)dpp_mov0<CTRL>((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long readlane63_u64(unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long v) { const unsigned long long o = dpp_mov0_u64<CTRL>(v); return o > v ? o : v; }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    v = dpp_max_u64<0xb1>(v); v = dpp_max_u64<0x4e>(v); v = dpp_max_u64<0x114>(v);
    v = dpp_max_u64<0x118>(v); v = dpp_max_u64<0x142>(v); v = dpp_max_u64<0x143>(v);
    return readlane63_u64(v);
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    v += dpp_mov0_u64<0xb1>(v); v += dpp_mov0_u64<0x4e>(v); v += dpp_mov0_u64<0x114>(v);
    v += dpp_mov0_u64<0x118>(v); v += dpp_mov0_u64<0x142>(v); v += dpp_mov0_u64<0x143>(v);
    return readlane63_u64(v);
}
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) {
    int x = (int)v;
    x += dpp_mov0<0x111>(x); x += dpp_mov0<0x112>(x); x += dpp_mov0<0x114>(x); x += dpp_mov0<0x118>(x);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    return (uint32_t)x;
}
// Exclusive scan of a uint32_t array by ONE workgroup of NT threads (256 or 1024), a chunk of NT entries per step: step(v) takes
// the thread's entry of this chunk and returns its exclusive prefix over the whole array so far, the earlier chunks included;
// after the last step total() is the sum of all entries. Lives in LDS (`__shared__ BlockScan<NT> scan;`), init() comes first.
// Precondition: all 64 lanes of every wave are active in step() (wave_incl_scan_u32 is a DPP sequence, and step() holds
// barriers) -- the workgroup has NT threads, none returns before the chunk loop, and a thread past the end of the array still
// calls step(0) for as many chunks as the others.
template <int NT>
struct BlockScan {
    uint32_t wave[NT / 64];   // inclusive totals of this chunk's waves
    uint32_t carry;           // sum of the earlier chunks
    __device__ __forceinline__ void init() {
        if (threadIdx.x == 0) carry = 0;
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t step(uint32_t v) {
        const uint32_t incl = wave_incl_scan_u32(v);
        const int w = threadIdx.x >> 6;
        if (lane_id() == 63) wave[w] = incl;
        __syncthreads();
        uint32_t before = carry;
        for (int k = 0; k < w; ++k) before += wave[k];
        __syncthreads();
        if (threadIdx.x == NT - 1) carry = before + incl;
        __syncthreads();
        return before + incl - v;
    }
    __device__ __forceinline__ uint32_t total() const { return carry; }
};
// Ordered compaction by ONE workgroup of NT threads, a chunk of NT entries per step: step(flag, total) returns the number of flagged
// threads in front of this one over all chunks so far -- the position of a flagged thread's entry in the compacted list -- and adds
// the chunk's flagged threads to `total`, a register that every thread keeps (0 before the first step). Lives in LDS like BlockScan
// and has the same precondition: every thread of the workgroup calls step() for every chunk. Two barriers per step, the second after
// the last read, so the next step (or another user of the same object) may follow at once. What the caller stores at the returned
// positions is the caller's to publish: a barrier after the last step, where other threads read the list.
template <int NT>
struct BlockRank {
    uint32_t wave[NT / 64];   // flagged threads of this chunk's waves
    __device__ __forceinline__ uint32_t step(bool flag, uint32_t& total) {
        const unsigned long long b = __ballot(flag);
        const int w = threadIdx.x >> 6;
        if (lane_id() == 0) wave[w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = total, chunk = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) { const uint32_t c = wave[k]; chunk += c; if (k < w) before += c; }
        __syncthreads();
        total += chunk;
        return before + (uint32_t)__popcll(b & ((1ull << lane_id()) - 1ull));
    }
};
template <int CTRL>
__device__ __forceinline__ double dpp_mov0_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = dpp_mov0<CTRL>((int)(b & 0xffffffffll)), hi = dpp_mov0<CTRL>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_sum_d(double v) {
    v += dpp_mov0_d<0xb1>(v);
    v += dpp_mov0_d<0x4e>(v);
    v += dpp_mov0_d<0x114>(v);
    v += dpp_mov0_d<0x118>(v);
    v += dpp_mov0_d<0x142>(v);
    v += dpp_mov0_d<0x143>(v);
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// ---- workgroup reductions ---------------------------------------------------------------------------------------------------
// block_<op><NW>(v, red): <op> over the NW waves (4: 256 threads, 16: 1024) of the workgroup, returned to every thread. `red` is the
// caller's LDS scratch, one slot per wave; the helpers declare no __shared__ of their own. One barrier discipline: wave reduce (DPP),
// lane 0 writes its slot, barrier, every thread reads and combines the NW slots, barrier -- so the same scratch serves the next call
// at once and no caller adds a barrier for the helper. Its two barriers also order the caller's own LDS traffic round the call.
// Precondition: every thread of the workgroup calls, from uniform control flow (a thread with nothing to add passes the identity).
// block_fold combines the slots left to right: r = ((red[0] . red[1]) . red[2]) . red[3]
template <int NW, class T, class F>
__device__ __forceinline__ T block_fold(T wave_total, T* red, F&& combine) {
    if (lane_id() == 0) red[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    T r = red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) r = combine(r, red[k]);
    __syncthreads();
    return r;
}
// order-free combines: integer sums (T = int or uint32_t), minima and maxima
template <int NW = 4, class T>
__device__ __forceinline__ T block_sum_i(T v, T* red) { return block_fold<NW>((T)wave_sum_i((int)v), red, [](T a, T b) { return (T)(a + b); }); }
template <int NW = 4>
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
    return block_fold<NW>(wave_sum_u64(v), red, [](unsigned long long a, unsigned long long b) { return a + b; });
}
template <int NW = 4>
__device__ __forceinline__ float block_min_f(float v, float* red) { return block_fold<NW>(wave_min_f(v), red, [](float a, float b) { return fminf(a, b); }); }
template <int NW = 4>
__device__ __forceinline__ float block_max_f(float v, float* red) { return block_fold<NW>(wave_max_f(v), red, [](float a, float b) { return fmaxf(a, b); }); }
template <int NW = 4>
__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, uint32_t* red) { return block_fold<NW>(wave_max_u32(v), red, [](uint32_t a, uint32_t b) { return a > b ? a : b; }); }
template <int NW = 4>
__device__ __forceinline__ unsigned long long block_min_u64(unsigned long long v, unsigned long long* red) {
    return block_fold<NW>(wave_min_u64(v), red, [](unsigned long long a, unsigned long long b) { return b < a ? b : a; });
}
template <int NW = 4>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* red) {
    return block_fold<NW>(wave_max_u64(v), red, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
}
// Float and double sums come in two associations of the wave partials, and results that are promised bit for bit depend on which:
//  * left fold ((r0 + r1) + r2) + r3: the grid build's coordinate sums (grid.hip: GridMeta::centroid), which a region of global.hip
//    must reproduce, every double sum of global.hip, and the mean / variance of k_sor_threshold (prefilter.hip)
//  * pairwise (r0 + r1) + (r2 + r3), 256 threads: the per-maximum sums of maxima.hip (weights, positions, box and quaternion sums) and
//    the covariance of the RANSAC sample-distance threshold (ransac.h), restated in that order by their host models
// A call site keeps the one it has; a new one that promises nothing takes the left fold.
template <int NW = 4>
__device__ __forceinline__ double block_sum_d_left(double v, double* red) { return block_fold<NW>(wave_sum_d(v), red, [](double a, double b) { return a + b; }); }
template <class T>
__device__ __forceinline__ T block_sum_pairwise(T wave_total, T* red) {
    if (lane_id() == 0) red[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    const T r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_sum_f_pairwise(float v, float* red) { return block_sum_pairwise(wave_sum_f(v), red); }
__device__ __forceinline__ double block_sum_d_pairwise(double v, double* red) { return block_sum_pairwise(wave_sum_d(v), red); }

// atan2 to ~1e-7 absolute (Abramowitz & Stegun 4.4.49, |err| <= 2e-8 before rounding) without OCML's expansion: for weights that are
// continuous in the angle (shot.hip) and for estimates whose hard decisions are re-taken exactly when they come close (short_shot.hip)
__device__ __forceinline__ float shot_atan2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float a = mn * __builtin_amdgcn_rcpf(mx);          // mx > 0: the caller excludes x == y == 0
    const float z = a * a;
    float p = 0.0028662257f;
    p = __builtin_fmaf(p, z, -0.0161657367f); p = __builtin_fmaf(p, z, 0.0429096138f); p = __builtin_fmaf(p, z, -0.0752896400f);
    p = __builtin_fmaf(p, z, 0.1065626393f); p = __builtin_fmaf(p, z, -0.1420889944f); p = __builtin_fmaf(p, z, 0.1999355085f);
    p = __builtin_fmaf(p, z, -0.3333314528f); p = __builtin_fmaf(p, z, 1.0f);
    float r = a * p;
    if (ay > ax) r = 1.57079632679489661923f - r;
    if (x < 0.f) r = 3.14159265358979323846f - r;
    return y < 0.f ? -r : r;
}

// CIELab of a packed 0x00RRGGBB colour through the context's two LUTs: PCL's RGB2CIELAB as it returns them (L <= 100, |a|, |b| <= 120),
// the values CoSPAIR rescales itself (cospair.hip)
__device__ __forceinline__ void rgb2lab(const float* lut_srgb, const float* lut_sxyz, uint32_t c4, float& L, float& A, float& B) {
    const float fr = lut_srgb[(c4 >> 16) & 0xff], fg = lut_srgb[(c4 >> 8) & 0xff], fb = lut_srgb[c4 & 0xff];
    const float X = fr * 0.412453f + fg * 0.357580f + fb * 0.180423f;
    const float Y = fr * 0.212671f + fg * 0.715160f + fb * 0.072169f;
    const float Z = fr * 0.019334f + fg * 0.119193f + fb * 0.950227f;
    float vx = X / 0.95047f, vy = Y, vz = Z / 1.08883f;
    int ix = (int)(vx * 4000), iy = (int)(vy * 4000), iz = (int)(vz * 4000);
    ix = ix < 0 ? 0 : (ix > 3999 ? 3999 : ix); iy = iy < 0 ? 0 : (iy > 3999 ? 3999 : iy); iz = iz < 0 ? 0 : (iz > 3999 ? 3999 : iz);
    vx = lut_sxyz[ix]; vy = lut_sxyz[iy]; vz = lut_sxyz[iz];
    L = 116.0f * vy - 16.0f; if (L > 100) L = 100.0f;
    A = 500.0f * (vx - vy); if (A > 120) A = 120.0f; else if (A < -120) A = -120.0f;
    B = 200.0f * (vy - vz); if (B > 120) B = 120.0f; else if (B < -120) B = -120.0f;
}
// the same normalised (L / 100, a / 120, b / 120): the keypoint's reference colour of k_shot<true> (shot.hip) and k_short_cshot (short_cshot.hip)
__device__ __forceinline__ void rgb2lab_norm(const float* lut_srgb, const float* lut_sxyz, uint32_t c4, float& L, float& A, float& B) {
    rgb2lab(lut_srgb, lut_sxyz, c4, L, A, B);
    L /= 100.0f; A /= 120.0f; B /= 120.0f;
}

// XCD-local block map for the per-object kernels. The hardware deals consecutive workgroup ids round-robin over the 8 XCDs
// (blocks b and b + 8 share one, MI355X_MICROARCH "Workgroup dispatch"), each with its own 4 MiB L2. With a (blocks, objects) 2-D
// grid the blocks of ONE object land on all eight XCDs and every L2 pulls every object's cloud from beyond (measured round 1:
// 8x the compulsory fetch). Here the grid is 1-D, 8 * nbx * ceil(n_obj / 8) blocks: the blocks with id = xcd (mod 8) walk the
// objects xcd, xcd + 8, ... one after the other, so an object's ~400 KB cloud is fetched once, into one L2. Speed only: the
// result does not depend on the placement. Returns false for the padding blocks of the last object group.
// Fewer than 8 objects (single-object detect()): plain object-major order, so that all XCDs work.
__device__ __forceinline__ bool xcd_object_block(int nbx, int n_obj, int& o, int& bx) {
    if (n_obj < 8) { o = blockIdx.x / nbx; bx = blockIdx.x % nbx; return true; }
    const int slot = blockIdx.x >> 3;
    o = (slot / nbx) * 8 + (blockIdx.x & 7);
    bx = slot % nbx;
    return o < n_obj;
}
// keypoint of wave `slot` of object o: through the cell-order permutation when there is one (ism_kp_order), else the slot itself
__device__ __forceinline__ uint32_t ordered_keypoint(const uint32_t* __restrict__ perm, uint32_t kp_begin, uint32_t slot) {
    return kp_begin + (perm ? perm[kp_begin + slot] : slot);
}
static inline unsigned xcd_object_grid(unsigned nbx, int n_obj) { return n_obj < 8 ? nbx * (unsigned)n_obj : 8u * nbx * (unsigned)((n_obj + 7) / 8); }

// cell coordinate of a value along one axis, clamped (monotone in v)
__device__ __forceinline__ int cell_coord(float v, float minv, float inv_cell, int dim) {
    int c = (int)floorf((v - minv) * inv_cell);
    return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}

// Conservative cell range of the ball (q, r) along every axis. Returns false when the ball misses the grid.
struct CellRange { int lo[3], hi[3]; };
__device__ __forceinline__ bool ball_cells(const GridMeta& m, float qx, float qy, float qz, float r, CellRange& cr) {
    const float q[3] = {qx, qy, qz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pad = r * 1e-5f + fabsf(q[a]) * 4e-7f + 1e-30f;   // absorbs the rounding of q±r and of the binning
        const float lo = (q[a] - r - pad - m.minv[a]) * m.inv_cell[a];
        const float hi = (q[a] + r + pad - m.minv[a]) * m.inv_cell[a];
        int l = (int)floorf(lo), h = (int)floorf(hi);
        if (h < 0 || l > m.dim[a] - 1) return false;
        cr.lo[a] = l < 0 ? 0 : l;
        cr.hi[a] = h > m.dim[a] - 1 ? m.dim[a] - 1 : h;
    }
    return true;
}

// Clips the x cell range of one (gy, gz) cell row to the chord of the ball (q, r) in that row. Conservative: the padding
// absorbs the float rounding of the cell bounds and of the point binning. Returns false when the row misses the ball.
__device__ __forceinline__ bool row_cells(const GridMeta& m, const CellRange& cr, int gy, int gz,
                                          float qx, float qy, float qz, float r, int& lo, int& hi) {
    const float pad = r * 2e-5f + (fabsf(qx) + fabsf(qy) + fabsf(qz)) * 1e-6f + 1e-30f;
    const float y0 = m.minv[1] + (float)gy * m.cell[1], z0 = m.minv[2] + (float)gz * m.cell[2];
    const float dy = fmaxf(fmaxf(y0 - qy, qy - (y0 + m.cell[1])) - pad, 0.f);
    const float dz = fmaxf(fmaxf(z0 - qz, qz - (z0 + m.cell[2])) - pad, 0.f);
    const float rr = r + pad;
    const float rem = rr * rr - (dy * dy + dz * dz);
    if (!(rem > 0.f)) return false;
    const float hc = sqrtf(rem) + pad;
    int l = (int)floorf((qx - hc - m.minv[0]) * m.inv_cell[0]), h = (int)floorf((qx + hc - m.minv[0]) * m.inv_cell[0]);
    lo = l < cr.lo[0] ? cr.lo[0] : l;
    hi = h > cr.hi[0] ? cr.hi[0] : h;
    return lo <= hi;
}

// One THREAD per query: the rows of cells that the ball (q, r) touches, one after the other, each clipped to its chord. f(b, e) takes
// the row's span [b, e) of object-local sorted point indices and returns false to end the sweep early (k_ror_count of prefilter.hip,
// the ISS3D sweeps of iss3d.hip: the queries are the cloud's own points in cell order, so the lanes of a wave read the same runs).
template <class F>
__device__ __forceinline__ void ball_rows_for_each(const GridMeta& m, const uint32_t* __restrict__ cs, float qx, float qy, float qz, float r, F&& f) {
    CellRange cr;
    if (!ball_cells(m, qx, qy, qz, r, cr)) return;
    for (int gz = cr.lo[2]; gz <= cr.hi[2]; ++gz)
        for (int gy = cr.lo[1]; gy <= cr.hi[1]; ++gy) {
            int xl, xh;
            if (!row_cells(m, cr, gy, gz, qx, qy, qz, r, xl, xh)) continue;
            const int rb = (gz * m.dim[1] + gy) * m.dim[0];
            if (!f(cs[rb + xl], cs[rb + xh + 1])) return;
        }
}

// ---- flattened ball traversal ---------------------------------------------------------------------------------------------
// A ball query touches (2R/cell+1)^2 cell rows; walking them one after the other costs, per row, the chord arithmetic on all 64
// lanes, two dependent cell_start loads and a mostly half-empty wave of points. Here the lanes first take one row EACH (chord,
// start, length: one round trip for up to 64 rows), a wave prefix sum lays the non-empty rows end to end, and the wave then sweeps
// the concatenated candidate list 64 at a time with every lane busy.
// Candidate -> row without a search: every non-empty row marks its LAST candidate in a bit mask (one ds_or_b64 per row batch);
// for the 64 candidates of a block the row of lane l is (rows that ended before the block: a running popcount) + (marks below l:
// v_mbcnt on the block's 64-bit word, which is wave-uniform and read one block ahead), and ONE per-lane LDS read of the row's
// (start - offset) turns the flat index into the sorted point index. Round 1 walked a per-lane cursor through a prefix table:
// three to four dependent LDS round trips per block.
#define ISM_ROWS_CAP 4096                  // candidates per window of the mark mask (64 words); longer row batches take several windows
struct WaveRows {
    unsigned long long last[ISM_ROWS_CAP / 64];   // bit i of last[b]: candidate 64 b + i (window-relative) is the last one of its row
    int delta[64];                                // per non-empty row: first sorted index - flat offset
    uint32_t rows_before[ISM_ROWS_CAP / 64];      // NG > 1 only: rows that ended before block b (window-relative)
};
// L(i, valid) loads and returns the point record (issued one sweep AHEAD of its use, so the next 64 candidates are in flight
// while the current ones are processed); F(record, i, valid) consumes it. i = object-local sorted point index; a lane without a
// candidate gets i = 0 (a valid index: the sweep only runs when a row holds points), so L may load unconditionally -- a conditional
// load costs an exec-mask branch and a zero fill of the record per block -- and F must not use the record when valid is false.
// NG = 1: the wave sweeps the flat list 64 consecutive candidates at a time (fully coalesced: 1 KB per load instruction).
// NG = 8: the list is cut into 8 contiguous segments and every group of 8 lanes walks its own segment (128 B per group and
//         load: still whole cache lines). The 64 candidates a wave looks at together then come from 8 DISTANT parts of the ball
//         instead of one short stretch of one cell row -- for k_shot this is what matters: neighbours that are adjacent in the
//         cell-sorted order fall into the same (sector, cosine) bin, and same-address LDS atomics of one wave instruction
//         serialise (measured: SHOT got SLOWER with finer x cells, i.e. with FEWER candidates but a more coherent order).
template <int NG = 1, bool IL = false, class L, class F>
__device__ __forceinline__ void ball_for_each(const GridMeta& m, const uint32_t* __restrict__ cs, const CellRange& cr,
                                              float qx, float qy, float qz, float r, int lane, WaveRows& wr, L&& load, F&& f) {
    const int ny = cr.hi[1] - cr.lo[1] + 1, nrows = ny * (cr.hi[2] - cr.lo[2] + 1);
    for (int r0 = 0; r0 < nrows; r0 += 64) {
        const int j = r0 + lane;
        uint32_t s = 0, len = 0;
        if (j < nrows) {
            const int gz = cr.lo[2] + j / ny, gy = cr.lo[1] + j % ny;
            int xl, xh;
            if (row_cells(m, cr, gy, gz, qx, qy, qz, r, xl, xh)) {
                const int rb = (gz * m.dim[1] + gy) * m.dim[0];
                s = cs[rb + xl]; len = cs[rb + xh + 1] - s;
            }
        }
        const uint32_t end = wave_incl_scan_u32(len);                            // flat offset one past this row's last candidate
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)end, 63);
        if (total == 0) continue;
        const unsigned long long ne = __ballot(len != 0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                   // the previous batch's table reads are done
        if (len != 0) wr.delta[__popcll(ne & ((1ull << lane) - 1ull))] = (int)s - (int)(end - len);
        for (uint32_t w0 = 0; w0 < total; w0 += ISM_ROWS_CAP) {                  // one window unless a row batch holds > 4096 candidates
            const uint32_t wn = min(total - w0, (uint32_t)ISM_ROWS_CAP);
            wr.last[lane] = 0ull;                                               // LDS traffic of one wave is ordered: no barrier needed
            if (len != 0 && end > w0 && end <= w0 + wn) atomicOr(&wr.last[(end - 1 - w0) >> 6], 1ull << ((end - 1 - w0) & 63));
            // The marks are read back by OTHER lanes. The hardware keeps the LDS operations of a wave in order, but the compiler
            // reasons per thread: without this (instruction-free) wavefront fence it forwards the 0 a lane has just stored to
            // that lane's own read of last[lane], as if no other lane could have written in between.
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t row_base = (uint32_t)__popcll(__ballot(len != 0 && end <= w0));   // rows that ended before this window
            if (NG == 1) {
                auto mask_of = [&](uint32_t b) -> unsigned long long {             // wave-uniform word -> SGPR pair
                    const unsigned long long v = wr.last[b];
                    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32) |
                           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v & 0xffffffffull));
                };
                auto locate = [&](unsigned long long mk, uint32_t rb, uint32_t flat, bool v) -> uint32_t {
                    if (!v) return 0u;
                    const uint32_t row = rb + __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
                    return (uint32_t)(wr.delta[row] + (int)flat);
                };
                unsigned long long mk = mask_of(0);
                bool vn = (uint32_t)lane < wn;
                uint32_t in = locate(mk, row_base, w0 + lane, vn);
                auto rn = load(in, vn);
                for (uint32_t c = 0; c < wn; c += 64) {
                    const bool v = vn; const uint32_t i = in; const auto rec = rn;
                    if (c + 64 < wn) {
                        row_base += (uint32_t)__popcll(mk);
                        mk = mask_of((c >> 6) + 1);
                        vn = c + 64 + lane < wn;
                        in = locate(mk, row_base, w0 + c + 64 + lane, vn);
                        rn = load(in, vn);
                    }
                    f(rec, i, v);
                }
            } else {
                constexpr int GL = 64 / NG;                                      // lanes per group
                {   // rows that ended before every 64-candidate block: exclusive prefix of the blocks' mark counts
                    const uint32_t pc = (uint32_t)__popcll(wr.last[lane]);
                    wr.rows_before[lane] = row_base + wave_incl_scan_u32(pc) - pc;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                }
                const uint32_t seg = ((wn + NG - 1) / NG + GL - 1) / GL * GL;   // segment length, a multiple of the group width
                // IL: lane l walks segment l % NG (the 8 regions alternate from lane to lane) instead of segment l / GL
                const uint32_t grp = IL ? (uint32_t)(lane % NG) : (uint32_t)(lane / GL), sub = IL ? (uint32_t)(lane / NG) : (uint32_t)(lane % GL);
                const uint32_t g0 = grp * seg + sub;
                const uint32_t gend = min((grp + 1u) * seg, wn);
                auto locate = [&](uint32_t flat, bool v) -> uint32_t {          // flat: window-relative
                    if (!v) return 0u;
                    const unsigned long long mk = wr.last[flat >> 6];
                    const uint32_t row = wr.rows_before[flat >> 6] + (uint32_t)__popcll(mk & ((1ull << (flat & 63u)) - 1ull));
                    return (uint32_t)(wr.delta[row] + (int)(w0 + flat));
                };
                bool vn = g0 < gend;
                uint32_t in = locate(g0, vn);
                auto rn = load(in, vn);
                for (uint32_t c = 0; c < seg; c += GL) {
                    const bool v = vn; const uint32_t i = in; const auto rec = rn;
                    if (c + GL < seg) {
                        vn = g0 + c + GL < gend;
                        in = locate(g0 + c + GL, vn);
                        rn = load(in, vn);
                    }
                    f(rec, i, v);
                }
            }
        }
    }
}
#endif

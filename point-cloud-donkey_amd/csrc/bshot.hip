// bshot.hip — the binarisation of B-SHOT: FeaturesBSHOT::getBinaryVector (features/features_bshot.cpp:109-157), applied to the rows
// ismhip_shot352 writes (FeaturesBSHOT::iComputeDescriptors, :40-107). A pure function of four floats; one thread per group of four.
// HBM-bound and tiny next to k_shot: 1408 bytes read and written per row.
#include "common.h"

namespace {

// getBinaryVector in the reference's statement order. Bit i of the result = result[i]. Every sum is a float sum in the written order
// (the unit is compiled with -ffp-contract=off), every comparison is taken in double against (double)sum * 0.9 (the literal 0.9 is a
// double, so the reference promotes both sides). A NaN anywhere makes sum != 0 true and every comparison false: case E, 1111.
__device__ __forceinline__ int bshot_bits(float v0, float v1, float v2, float v3) {
    int r = 0;                                                   // case A
    const float sum = ((v0 + v1) + v2) + v3;
    if (sum != 0) {
        const double t = (double)sum * 0.9;
        // case B
        if ((double)v0 > t) r |= 1;
        if ((double)v1 > t) r |= 2;
        if ((double)v2 > t) r |= 4;
        if ((double)v3 > t) r |= 8;
        const bool case_b = __popc(r) == 1;
        // case C: `result` carries over (two bits left by case B with no pair test firing count as case C)
        bool case_c = false;
        if (!case_b) {
            if ((double)(v0 + v1) > t) r = 1 | 2;
            if ((double)(v0 + v2) > t) r = 1 | 4;
            if ((double)(v0 + v3) > t) r = 1 | 8;
            if ((double)(v1 + v2) > t) r = 2 | 4;
            if ((double)(v1 + v3) > t) r = 2 | 8;
            if ((double)(v2 + v3) > t) r = 4 | 8;
            case_c = __popc(r) == 2;
        }
        // case D
        bool case_d = false;
        if (!case_b && !case_c) {
            if ((double)((v0 + v1) + v2) > t) r = 1 | 2 | 4;
            if ((double)((v0 + v1) + v3) > t) r = 1 | 2 | 8;
            if ((double)((v0 + v2) + v3) > t) r = 1 | 4 | 8;
            if ((double)((v1 + v2) + v3) > t) r = 2 | 4 | 8;
            case_d = __popc(r) == 3;
        }
        // case E
        if (!case_b && !case_c && !case_d) r = 15;
    }
    return r;
}

// VEC: both pointers are 16-byte aligned (one dwordx4 per group); else four dword accesses. A thread reads its group before it writes
// it and no other thread touches it, so dst may be src.
template <bool VEC>
__global__ __launch_bounds__(256) void k_bshot_binarize(const float* src, float* dst, size_t n_groups) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    float4 v;
    if (VEC) v = ((const float4*)src)[g];
    else { v.x = src[4 * g]; v.y = src[4 * g + 1]; v.z = src[4 * g + 2]; v.w = src[4 * g + 3]; }
    const int r = bshot_bits(v.x, v.y, v.z, v.w);
    float4 o;
    o.x = (r & 1) ? 1.f : 0.f; o.y = (r & 2) ? 1.f : 0.f; o.z = (r & 4) ? 1.f : 0.f; o.w = (r & 8) ? 1.f : 0.f;
    if (VEC) ((float4*)dst)[g] = o;
    else { dst[4 * g] = o.x; dst[4 * g + 1] = o.y; dst[4 * g + 2] = o.z; dst[4 * g + 3] = o.w; }
}

int launch_binarize(ismhip_ctx* ctx, size_t n_rows, const float* src, float* dst) {
    const size_t n_groups = n_rows * (ISMHIP_SHOT_DIM / 4);
    if (n_groups == 0) return ISMHIP_OK;
    const size_t blocks = (n_groups + 255) / 256;
    if (blocks > 0x7fffffffull) return ism_set_err(ctx, ISMHIP_ERR_UNSUPPORTED, "bshot_binarize: too many rows for one launch");
    const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    if (vec) hipLaunchKernelGGL(k_bshot_binarize<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, src, dst, n_groups);
    else hipLaunchKernelGGL(k_bshot_binarize<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, src, dst, n_groups);
    ISM_CHECK_LAUNCH(ctx, "k_bshot_binarize");
    return ISMHIP_OK;
}

}  // namespace

extern "C" {

int ismhip_bshot_binarize(ismhip_ctx* ctx, int n_rows, const float* src, float* dst) {
    if (!ctx || n_rows < 0 || (n_rows > 0 && (!src || !dst))) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "bshot_binarize: bad argument");
    TimerScope ts(ctx, "bshot");
    return launch_binarize(ctx, (size_t)n_rows, src, dst);
}

int ismhip_bshot352(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                    const float* kpx, const float* kpy, const float* kpz,
                    const float* lrf9, float radius, float* desc_out, uint32_t* neighbour_count_out) {
    const int rc = ismhip_shot352(ctx, cloud, kp_offsets_h, kpx, kpy, kpz, lrf9, radius, desc_out, neighbour_count_out);
    if (rc != ISMHIP_OK) return rc;
    const size_t nkp = kp_offsets_h[cloud->n_obj];           // ismhip_shot352 has checked the arguments
    TimerScope ts(ctx, "bshot");
    return launch_binarize(ctx, nkp, desc_out, desc_out);
}

}  // extern "C"

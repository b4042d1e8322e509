// mlp.hip — a small perceptron on the exact FP32 matrix cores, and the weights container it is loaded from. Its first user is the CGF
// embedding (third_party/cgf/embedding.py:103-108: 2244 -> 512 -> 512 -> 512 -> 512 -> D, ReLU after the first four layers), the one
// place where the reference leaves its process for a whole framework; nothing here knows about CGF but the container's name.
//
// k_mlp_forward, one launch under the timer "mlp_forward": a workgroup of four waves owns a tile of 64 rows and carries it through
// EVERY layer. The tile's activations live in LDS, act[64][516] floats (129 KiB; the row stride 516 = 4 mod 64 banks keeps the 16-byte
// fragment reads of 32 rows apart); only the first layer's input and the last layer's output touch HBM. The first layer's input, up to
// 4096 wide, passes through the same buffer in chunks of 512 columns.
//   - v_mfma_f32_32x32x2_f32 with the OUTPUT COLUMNS as the rows of the instruction (A = W^T, one coalesced dword of W per lane and k)
//     and the tile's rows as its columns (B = act, a 16-byte LDS read per lane and four k). A lane then holds, for one row of the tile,
//     four consecutive output columns per accumulator quad: the next layer's activations go back to LDS as 16-byte stores.
//   - wave w owns the output columns [128 w, 128 w + 128): 4 column tiles x 2 row tiles = 8 accumulators of 16 registers. Columns
//     beyond `out` and k beyond `in` read as zero (selected, never multiplied: a weight need not be finite to be masked).
//   - k runs in blocks of 8; inside a block the lane half h takes k = 4 h + e at step e. The order is fixed: every output element is
//     ONE fma chain over k in that order, whatever the row count and wherever the row sits in its tile. Bias and ReLU in float after the
//     chain; a NaN stays a NaN (v < 0 ? 0 : v).
// The weights are read from L2 / HBM once per workgroup (7.7 MB for the CGF net, 32 FLOP per byte at 64 rows).
#include "common.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define MLP_ROWS 64
#define MLP_KC 512                                   // columns of the activation buffer in use
#define MLP_LD 516                                   // its row stride in floats
#define MLP_LDS ((size_t)MLP_ROWS * MLP_LD * sizeof(float))
static_assert(MLP_KC == ISMHIP_MLP_MAX_OUT && MLP_KC % 8 == 0 && MLP_LD % 4 == 0, "MLP tile");

struct MlpLayer { const float* W; const float* b; int in, out, relu; };
struct MlpArgs { MlpLayer layer[ISMHIP_MLP_MAX_LAYERS]; int n_layers; const float* x; float* y; unsigned long long n_rows; };

struct ismhip_mlp {
    int n_layers = 0;
    MlpLayer layer[ISMHIP_MLP_MAX_LAYERS] = {};
    float* store = nullptr;                          // one allocation: every W and b
};

struct ismhip_cgfw {
    struct L { int in, out, relu; std::vector<float> W, b; };
    std::vector<L> layers;
};

namespace {

__global__ __launch_bounds__(256) void k_mlp_forward(MlpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float act[];       // [MLP_ROWS][MLP_LD]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    const unsigned long long row0 = (unsigned long long)blockIdx.x * MLP_ROWS;
    for (int l = 0; l < a.n_layers; ++l) {
        const MlpLayer L = a.layer[l];
        const bool last = l + 1 == a.n_layers;
        int nt = (L.out - wv * 128 + 31) / 32;                        // column tiles of this wave that hold a column
        nt = nt < 0 ? 0 : (nt > 4 ? 4 : nt);
        f32x16 acc[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][rt][e] = 0.f;
        for (int kb = 0; kb < L.in; kb += MLP_KC) {                   // one pass but for the first layer
            const int kc = min(MLP_KC, L.in - kb), kc8 = (kc + 7) & ~7;
            if (l == 0) {
                __syncthreads();                                      // the last chunk has been multiplied
                for (int r = wv * 16; r < wv * 16 + 16; ++r) {
                    const unsigned long long row = row0 + r;
                    const float* src = a.x + (row < a.n_rows ? row : 0ull) * (unsigned long long)L.in + kb;
                    for (int k = lane; k < kc8; k += 64) act[r * MLP_LD + k] = (row < a.n_rows && k < kc) ? src[k] : 0.f;
                }
                __syncthreads();
            }
            for (int k0 = 0; k0 < kc8; k0 += 8) {
                f32x4 xb[2];
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) xb[rt] = *(const f32x4*)(act + (r32 + 32 * rt) * MLP_LD + k0 + 4 * h);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (t >= nt) continue;                            // wave-uniform
                    const int oc = wv * 128 + 32 * t + r32;
                    float wa[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = kb + k0 + 4 * h + e;
                        const bool ok = k < L.in && oc < L.out;
                        const float v = L.W[ok ? (size_t)k * L.out + oc : 0];
                        wa[e] = ok ? v : 0.f;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int rt = 0; rt < 2; ++rt) acc[t][rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[e], xb[rt][e], acc[t][rt], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                              // every wave has read the layer's input
        // C layout: column = lane & 31 (the tile's row), row = (e & 3) + 8 (e >> 2) + 4 h (the output column inside its tile)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= nt) continue;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const int r = r32 + 32 * rt;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int oc = wv * 128 + 32 * t + 8 * j + 4 * h;
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const bool ok = oc + i < L.out;
                        float s = acc[t][rt][4 * j + i] + (ok ? L.b[oc + i] : 0.f);
                        if (L.relu) s = s < 0.f ? 0.f : s;
                        v[i] = ok ? s : 0.f;
                    }
                    if (!last) *(f32x4*)(act + r * MLP_LD + oc) = v;  // columns past `out` up to the tile's end: zeros, the next layer's k padding
                    else if (row0 + r < a.n_rows) {
                        float* dst = a.y + (row0 + r) * (unsigned long long)L.out;
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (oc + i < L.out) dst[oc + i] = v[i];
                    }
                }
            }
        }
        __syncthreads();
    }
}

int cgfw_fail(char* err, int err_len, const std::string& msg) {
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", msg.c_str());
    return ISMHIP_ERR_INVALID;
}

}  // namespace

extern "C" {

int ismhip_mlp_create(ismhip_ctx* ctx, int n_layers, const int* in, const int* out, const int* relu,
                      const float* const* W_h, const float* const* b_h, ismhip_mlp** mlp_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!mlp_out || !in || !out || !relu || !W_h || !b_h) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "mlp_create: bad argument");
    if (n_layers < 1 || n_layers > ISMHIP_MLP_MAX_LAYERS) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "mlp_create: layer count outside 1 .. 8");
    size_t total = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (!W_h[l] || !b_h[l]) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "mlp_create: bad argument");
        if (in[l] < 1 || in[l] > ISMHIP_MLP_MAX_IN || out[l] < 1 || out[l] > ISMHIP_MLP_MAX_OUT)
            return ism_set_err(ctx, ISMHIP_ERR_INVALID, "mlp_create: width out of range (in 1 .. 4096, out 1 .. 512)");
        if (l > 0 && in[l] != out[l - 1]) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "mlp_create: inconsistent widths");
        total += ((size_t)in[l] * out[l] + 3) / 4 * 4 + ((size_t)out[l] + 3) / 4 * 4;
    }
    ismhip_mlp* m = new ismhip_mlp();
    if (hipMalloc((void**)&m->store, total * sizeof(float)) != hipSuccess) { delete m; return ism_set_err(ctx, ISMHIP_ERR_NOMEM, "mlp_create: hipMalloc failed"); }
    m->n_layers = n_layers;
    float* p = m->store;
    for (int l = 0; l < n_layers; ++l) {
        const size_t nw = (size_t)in[l] * out[l];
        float* W = p; p += (nw + 3) / 4 * 4;
        float* b = p; p += ((size_t)out[l] + 3) / 4 * 4;
        if (hipMemcpy(W, W_h[l], nw * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(b, b_h[l], (size_t)out[l] * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(m->store); delete m;
            return ism_set_err(ctx, ISMHIP_ERR_HIP, "mlp_create: hipMemcpy failed");
        }
        m->layer[l] = MlpLayer{W, b, in[l], out[l], relu[l] ? 1 : 0};
    }
    *mlp_out = m;
    return ISMHIP_OK;
}

int ismhip_mlp_destroy(ismhip_mlp* mlp) {
    if (!mlp) return ISMHIP_OK;
    if (mlp->store) (void)hipFree(mlp->store);
    delete mlp;
    return ISMHIP_OK;
}

int ismhip_mlp_in(const ismhip_mlp* mlp) { return mlp ? mlp->layer[0].in : -1; }
int ismhip_mlp_out(const ismhip_mlp* mlp) { return mlp ? mlp->layer[mlp->n_layers - 1].out : -1; }

int ismhip_mlp_forward(ismhip_ctx* ctx, const ismhip_mlp* mlp, const float* x, size_t n_rows, float* y) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!mlp) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "mlp_forward: bad argument");
    if (n_rows == 0) return ISMHIP_OK;
    if (!x || !y || (n_rows + MLP_ROWS - 1) / MLP_ROWS > 0x7fffffffull) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "mlp_forward: bad argument");
    { const int rc = ism_lds_cap(ctx, (const void*)k_mlp_forward, MLP_LDS); if (rc != ISMHIP_OK) return rc; }
    MlpArgs a = {};
    for (int l = 0; l < mlp->n_layers; ++l) a.layer[l] = mlp->layer[l];
    a.n_layers = mlp->n_layers; a.x = x; a.y = y; a.n_rows = n_rows;
    TimerScope ts(ctx, "mlp_forward");
    hipLaunchKernelGGL(k_mlp_forward, dim3((unsigned)((n_rows + MLP_ROWS - 1) / MLP_ROWS)), dim3(256), MLP_LDS, ctx->stream, a);
    ISM_CHECK_LAUNCH(ctx, "k_mlp_forward");
    return ISMHIP_OK;
}

// ---- the weights container (header: ".cgfw") ------------------------------------------------------------------------------------
int ismhip_cgfw_open(const char* path, int expect_in, ismhip_cgfw** out, char* err, int err_len) {
    if (!path || !out) return cgfw_fail(err, err_len, "cgfw: bad argument");
    *out = nullptr;
    const std::string who = std::string("cgfw \"") + path + "\": ";
    FILE* f = fopen(path, "rb");
    if (!f) return cgfw_fail(err, err_len, who + "cannot open");
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    auto rd_u32 = [&](uint32_t& v) {                                  // little endian, whatever the host
        unsigned char b[4];
        if (fread(b, 1, 4, f) != 4) return false;
        v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        return true;
    };
    auto rd_f32 = [&](std::vector<float>& dst, size_t n) {
        dst.resize(n);
        std::vector<unsigned char> raw(n * 4);
        if (n && fread(raw.data(), 1, n * 4, f) != n * 4) return false;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t u = (uint32_t)raw[4 * i] | ((uint32_t)raw[4 * i + 1] << 8) | ((uint32_t)raw[4 * i + 2] << 16) | ((uint32_t)raw[4 * i + 3] << 24);
            memcpy(&dst[i], &u, 4);
        }
        return true;
    };
    char magic[4];
    if (fread(magic, 1, 4, f) != 4) return cgfw_fail(err, err_len, who + "truncated file");
    if (memcmp(magic, "CGFW", 4) != 0) return cgfw_fail(err, err_len, who + "wrong magic");
    uint32_t version = 0, nl = 0;
    if (!rd_u32(version) || !rd_u32(nl)) return cgfw_fail(err, err_len, who + "truncated file");
    if (version != 1) return cgfw_fail(err, err_len, who + "unsupported version " + std::to_string(version));
    if (nl < 1 || nl > ISMHIP_MLP_MAX_LAYERS) return cgfw_fail(err, err_len, who + "layer count " + std::to_string(nl) + " outside 1 .. 8");
    std::unique_ptr<ismhip_cgfw> w(new ismhip_cgfw());
    for (uint32_t l = 0; l < nl; ++l) {
        uint32_t in = 0, o = 0, act = 0;
        if (!rd_u32(in) || !rd_u32(o) || !rd_u32(act)) return cgfw_fail(err, err_len, who + "truncated file");
        const std::string at = "layer " + std::to_string(l + 1) + ": ";
        if (in < 1 || in > ISMHIP_MLP_MAX_IN || o < 1 || o > ISMHIP_MLP_MAX_OUT)
            return cgfw_fail(err, err_len, who + at + "width out of range (in 1 .. 4096, out 1 .. 512)");
        if (l == 0 && expect_in > 0 && (int)in != expect_in)
            return cgfw_fail(err, err_len, who + "first layer width " + std::to_string(in) + ", not " + std::to_string(expect_in));
        if (l > 0 && (int)in != w->layers.back().out) return cgfw_fail(err, err_len, who + at + "inconsistent widths");
        if (act > 1) return cgfw_fail(err, err_len, who + at + "unknown activation");
        ismhip_cgfw::L L;
        L.in = (int)in; L.out = (int)o; L.relu = (int)act;
        if (!rd_f32(L.W, (size_t)in * o) || !rd_f32(L.b, o)) return cgfw_fail(err, err_len, who + at + "truncated file");
        for (float v : L.W) if (!std::isfinite(v)) return cgfw_fail(err, err_len, who + at + "non-finite weight");
        for (float v : L.b) if (!std::isfinite(v)) return cgfw_fail(err, err_len, who + at + "non-finite weight");
        w->layers.push_back(std::move(L));
    }
    if (fgetc(f) != EOF) return cgfw_fail(err, err_len, who + "trailing bytes");
    *out = w.release();
    return ISMHIP_OK;
}

int ismhip_cgfw_close(ismhip_cgfw* w) { delete w; return ISMHIP_OK; }
int ismhip_cgfw_layers(const ismhip_cgfw* w) { return w ? (int)w->layers.size() : -1; }
int ismhip_cgfw_layer(const ismhip_cgfw* w, int layer, int* in, int* out, int* relu, const float** W, const float** b) {
    if (!w || layer < 0 || layer >= (int)w->layers.size()) return ISMHIP_ERR_INVALID;
    const ismhip_cgfw::L& L = w->layers[layer];
    if (in) *in = L.in;
    if (out) *out = L.out;
    if (relu) *relu = L.relu;
    if (W) *W = L.W.data();
    if (b) *b = L.b.data();
    return ISMHIP_OK;
}

int ismhip_mlp_from_cgfw(ismhip_ctx* ctx, const ismhip_cgfw* w, ismhip_mlp** mlp_out) {
    if (!ctx) return ISMHIP_ERR_INVALID;
    if (!w || w->layers.empty()) return ism_set_err(ctx, ISMHIP_ERR_INVALID, "mlp_from_cgfw: bad argument");
    int in[ISMHIP_MLP_MAX_LAYERS], out[ISMHIP_MLP_MAX_LAYERS], relu[ISMHIP_MLP_MAX_LAYERS];
    const float *W[ISMHIP_MLP_MAX_LAYERS], *b[ISMHIP_MLP_MAX_LAYERS];
    const int n = (int)w->layers.size();
    for (int l = 0; l < n; ++l) { in[l] = w->layers[l].in; out[l] = w->layers[l].out; relu[l] = w->layers[l].relu; W[l] = w->layers[l].W.data(); b[l] = w->layers[l].b.data(); }
    return ismhip_mlp_create(ctx, n, in, out, relu, W, b, mlp_out);
}

}  // extern "C"

// Device-side LoRA re-merge (HBM-bound): W' = (W0 + r * B.A) * g written straight into the packed weight tensor the
// forward kernels read, so a new LoRA scale / skip gamma r (src/pix2pix_turbo.py:206-207,211,217: set_adapters([..], [r]),
// decoder.gamma = r) costs one streaming pass over the adapted layers instead of a host re-pack + upload.
//   w0  fp32 master of the layer in PACKED layout [N][K] (K = kh*kw*cin_padded, k contiguous)
//   a   fp32 [rank][K]: lora_A in the same k order, adapter scaling lora_alpha/rank folded in; several adapters on one
//       layer are concatenated along rank
//   b   fp32 [N][rank]: lora_B
//   rg  device float[2] = (r, gamma): read at run time so the merge program itself never changes
// One thread owns 4 consecutive k of ROWS rows: the A chunk is loaded once per j for all rows, the B values are
// wave-uniform (scalar loads).  fp32 FMA chain in j order, then one rounding to `T`.
// Three forms share the file: per layer (i2i_lora_merge), every plain layer of a network in one launch (i2i_merge_group_*), and the
// TwinConv fold of the sketch model's conv_in (i2i_twin_fold).
#include <new>

#include "i2i_dev.h"
#include "launch.h"

namespace {

constexpr int LM_ROWS = 4;

// A pointer that was itself LOADED from memory (the grouped kernel's layer table) is a generic address to the compiler: flat vector loads,
// no scalar loads for the wave-uniform B values.  Every operand here lives in global memory; the tile body says so through the pointer
// types, which costs nothing where the pointer came from the kernel arguments (already known to be global) and changes no arithmetic.
#if defined(__HIP_DEVICE_COMPILE__)
#define I2I_GLOBAL __attribute__((address_space(1)))
#else
#define I2I_GLOBAL
#endif

// The plain merge of one tile: 1024 consecutive k (x-tile `xt`, 4 per thread) of LM_ROWS rows (row block `yt`).  The per-layer kernel and
// the grouped kernel both run THIS function, so their stored bits are equal by construction.
template <typename T>
__device__ __forceinline__ void lora_merge_tile(const i2i_lora_merge_params& p, int xt, int yt) {
    const int k = (xt * 256 + (int)threadIdx.x) * 4;
    if (k >= p.K) return;
    const int n0 = yt * LM_ROWS;
    const I2I_GLOBAL float* rg = (const I2I_GLOBAL float*)p.rg;
    const I2I_GLOBAL float* pa = (const I2I_GLOBAL float*)p.a;
    const I2I_GLOBAL float* pb = (const I2I_GLOBAL float*)p.b;
    const I2I_GLOBAL float* pw = (const I2I_GLOBAL float*)p.w0;
    I2I_GLOBAL T* pd = (I2I_GLOBAL T*)p.dst;
    const float r = rg ? rg[0] : 1.f;
    const float g = (rg && p.use_gamma) ? rg[1] : 1.f;
    float acc[LM_ROWS][4];
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
    for (int j = 0; j < p.rank; ++j) {
        const f32x4 a = *(const I2I_GLOBAL f32x4*)(pa + (int64_t)j * p.K + k);
#pragma unroll
        for (int i = 0; i < LM_ROWS; ++i) {
            const int n = n0 + i < p.N ? n0 + i : p.N - 1;
            const float bv = pb[(int64_t)n * p.rank + j];
            acc[i][0] = fmaf(bv, a[0], acc[i][0]);
            acc[i][1] = fmaf(bv, a[1], acc[i][1]);
            acc[i][2] = fmaf(bv, a[2], acc[i][2]);
            acc[i][3] = fmaf(bv, a[3], acc[i][3]);
        }
    }
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i) {
        const int n = n0 + i;
        if (n >= p.N) break;
        const f32x4 w = *(const I2I_GLOBAL f32x4*)(pw + (int64_t)n * p.K + k);
        I2I_GLOBAL T* d = pd + (int64_t)n * p.K + k;
        d[0] = from_f32<T>((w[0] + r * acc[i][0]) * g);
        d[1] = from_f32<T>((w[1] + r * acc[i][1]) * g);
        d[2] = from_f32<T>((w[2] + r * acc[i][2]) * g);
        d[3] = from_f32<T>((w[3] + r * acc[i][3]) * g);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void lora_merge_kernel(const i2i_lora_merge_params p) {
    lora_merge_tile<T>(p, (int)blockIdx.x, (int)blockIdx.y);
}

// Grouped form: a 1-D grid over the tiles of every layer.  prefix[l] = first tile of layer l (prefix[n] = the grid size); the layer of
// a workgroup is the last l with prefix[l] <= blockIdx.x, found by binary search -- everything up to the tile body depends on blockIdx
// alone, so the search, the struct and the B values stay scalar loads.  Tiles of a layer run x-tile fastest, as the 2-D grid does.
template <typename T>
__global__ __launch_bounds__(256) void lora_merge_group_kernel(const i2i_lora_merge_params* __restrict__ table, const int32_t* __restrict__ prefix, int n) {
    const int bid = (int)blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= bid) lo = mid; else hi = mid - 1;
    }
    const i2i_lora_merge_params p = table[lo];
    const int local = bid - prefix[lo];
    const int xtiles = (p.K / 4 + 255) / 256;
    lora_merge_tile<T>(p, local % xtiles, local / xtiles);
}

// TwinConv fold (i2i_twin_fold_params has the contract): the tiling of lora_merge_kernel with two chains per element.
template <typename T>
__global__ __launch_bounds__(256) void twin_fold_kernel(const i2i_twin_fold_params p) {
    const int n0 = (int)blockIdx.y * LM_ROWS;
    const float r = p.rg ? p.rg[0] : 1.f;
    const float q = 1.f - r;
    if (p.bias && blockIdx.x == 0 && (int)threadIdx.x < LM_ROWS && n0 + (int)threadIdx.x < p.N) {
        const int n = n0 + (int)threadIdx.x;
        p.bias[n] = fmaf(q, p.bias_pre[n], r * p.bias_cur[n]);
    }
    const int k = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    if (k >= p.K) return;
    float s0[LM_ROWS][4], s1[LM_ROWS][4];
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s0[i][e] = 0.f; s1[i][e] = 0.f; }
    for (int j = 0; j < p.rank_pre; ++j) {
        const f32x4 a = *(const f32x4*)(p.a_pre + (int64_t)j * p.K + k);
#pragma unroll
        for (int i = 0; i < LM_ROWS; ++i) {
            const int n = n0 + i < p.N ? n0 + i : p.N - 1;
            const float bv = p.b_pre[(int64_t)n * p.rank_pre + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) s0[i][e] = fmaf(bv, a[e], s0[i][e]);
        }
    }
    for (int j = 0; j < p.rank_cur; ++j) {
        const f32x4 a = *(const f32x4*)(p.a_cur + (int64_t)j * p.K + k);
#pragma unroll
        for (int i = 0; i < LM_ROWS; ++i) {
            const int n = n0 + i < p.N ? n0 + i : p.N - 1;
            const float bv = p.b_cur[(int64_t)n * p.rank_cur + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) s1[i][e] = fmaf(bv, a[e], s1[i][e]);
        }
    }
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i) {
        const int n = n0 + i;
        if (n >= p.N) break;
        const f32x4 w0 = *(const f32x4*)(p.w_pre + (int64_t)n * p.K + k);
        const f32x4 w1 = *(const f32x4*)(p.w_cur + (int64_t)n * p.K + k);
        T* d = (T*)p.dst + (int64_t)n * p.K + k;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = from_f32<T>(fmaf(q, fmaf(r, s0[i][e], w0[e]), r * fmaf(r, s1[i][e], w1[e])));
    }
}

__global__ void set_rg_kernel(float* rg, float r, float gamma) {
    if (threadIdx.x == 0) { rg[0] = r; rg[1] = gamma; }
}

// LayerNorm-fold form (i2i_lora_merge_params.kscale ..): one workgroup owns LM_ROWS whole rows and walks K in 1024-element trips, so that the
// row sums the consumer GEMM needs -- colsum[n] = sum_k of the STORED dst[n][k], bias_out[n] = bias0[n] + sum_k w'[n][k] * kshift[k] -- are
// reduced inside the block in a fixed order (thread partials in k order, then 256 partials in thread order through LDS).
template <typename T>
__global__ __launch_bounds__(256) void lora_merge_lnf_kernel(const i2i_lora_merge_params p) {
    const int tid = (int)threadIdx.x;
    const int n0 = (int)blockIdx.y * LM_ROWS;
    const float r = p.rg ? p.rg[0] : 1.f;
    const float g = (p.rg && p.use_gamma) ? p.rg[1] : 1.f;
    float cs[LM_ROWS], bs[LM_ROWS];
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i) { cs[i] = 0.f; bs[i] = 0.f; }
    for (int k = tid * 4; k < p.K; k += 1024) {
        float acc[LM_ROWS][4];
#pragma unroll
        for (int i = 0; i < LM_ROWS; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
        for (int j = 0; j < p.rank; ++j) {
            const f32x4 a = *(const f32x4*)(p.a + (int64_t)j * p.K + k);
#pragma unroll
            for (int i = 0; i < LM_ROWS; ++i) {
                const int n = n0 + i < p.N ? n0 + i : p.N - 1;
                const float bv = p.b[(int64_t)n * p.rank + j];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][e] = fmaf(bv, a[e], acc[i][e]);
            }
        }
        const f32x4 ks = *(const f32x4*)(p.kscale + k), kh = *(const f32x4*)(p.kshift + k);
#pragma unroll
        for (int i = 0; i < LM_ROWS; ++i) {
            const int n = n0 + i;
            if (n >= p.N) break;
            const f32x4 w = *(const f32x4*)(p.w0 + (int64_t)n * p.K + k);
            T* d = (T*)p.dst + (int64_t)n * p.K + k;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float wm = (w[e] + r * acc[i][e]) * g;
                const T st = from_f32<T>(wm * ks[e]);
                d[e] = st;
                cs[i] += to_f32<T>(st);
                bs[i] = fmaf(wm, kh[e], bs[i]);
            }
        }
    }
    float* red = (float*)i2i_smem;                // [256][LM_ROWS][2]
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i) { red[(tid * LM_ROWS + i) * 2] = cs[i]; red[(tid * LM_ROWS + i) * 2 + 1] = bs[i]; }
    __syncthreads();
    if (tid < LM_ROWS && n0 + tid < p.N) {
        float C = 0.f, B = 0.f;
        for (int t = 0; t < 256; ++t) { C += red[(t * LM_ROWS + tid) * 2]; B += red[(t * LM_ROWS + tid) * 2 + 1]; }
        p.colsum[n0 + tid] = C;
        p.bias_out[n0 + tid] = (p.bias0 ? p.bias0[n0 + tid] : 0.f) + B;
    }
}

}  // namespace

namespace i2i {      // runtime_hip.hip (hipMalloc / hipMemcpy) or tests/emu/runtime_emu.cpp (malloc / memcpy)
void* rt_alloc(size_t bytes);
void rt_free(void* p);
int rt_upload(void* dst, const void* src, size_t bytes);
// (plan_file.hip: i2i_plan_set_scale) rg[0..1] = (r, gamma), stream-ordered
int set_rg(float* rg, float r, float gamma, void* stream) {
    if (!rg) return fail(I2I_ERR_BAD_ARG, "set_rg: null pointer");
    hipLaunchKernelGGL(set_rg_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, rg, r, gamma);
    return check_launch("set_rg");
}
}  // namespace i2i

namespace {
bool is_lnf(const i2i_lora_merge_params* p) { return p->kscale || p->kshift || p->colsum || p->bias_out; }

// what every entry refuses; `who` prefixes the message ("lora_merge", "merge_group_create: layer 3")
int check_merge(const i2i_lora_merge_params* p, const char* who) {
    if (!p || !p->dst || !p->w0) return i2i::fail(I2I_ERR_BAD_ARG, "%s: null operand", who);
    if (p->rank > 0 && (!p->a || !p->b)) return i2i::fail(I2I_ERR_BAD_ARG, "%s: rank %d without A/B", who, p->rank);
    if (p->N <= 0 || p->K <= 0 || (p->K & 3) || p->rank < 0) return i2i::fail(I2I_ERR_BAD_ARG, "%s: bad shape N=%d K=%d rank=%d", who, p->N, p->K, p->rank);
    if (is_lnf(p)) {
        if (!p->kscale || !p->kshift || !p->colsum || !p->bias_out) return i2i::fail(I2I_ERR_BAD_ARG, "%s: the LayerNorm fold needs kscale, kshift, colsum and bias_out", who);
        if (((uintptr_t)p->kscale | (uintptr_t)p->kshift) & 15) return i2i::fail(I2I_ERR_BAD_ARG, "%s: kscale / kshift must be 16-byte aligned", who);
    }
    return I2I_OK;
}

struct MergeGroup {
    i2i_lora_merge_params* table = nullptr;      // device
    int32_t* prefix = nullptr;                   // device, n + 1 entries
    int n = 0, tiles = 0, dtype = 0;
};
}  // namespace

extern "C" int i2i_lora_merge(const i2i_lora_merge_params* p, int dtype, void* stream) {
    const int rc = check_merge(p, "lora_merge");
    if (rc != I2I_OK) return rc;
    const dim3 grid((unsigned)((p->K / 4 + 255) / 256), (unsigned)((p->N + LM_ROWS - 1) / LM_ROWS));
    hipStream_t s = (hipStream_t)stream;
    if (is_lnf(p)) {
        const dim3 gl(1u, grid.y);
        const size_t smem = 256 * LM_ROWS * 2 * sizeof(float);
        switch (dtype) {
            case I2I_F32: hipLaunchKernelGGL((lora_merge_lnf_kernel<float>), gl, dim3(256), smem, s, *p); break;
            case I2I_BF16: hipLaunchKernelGGL((lora_merge_lnf_kernel<__bf16>), gl, dim3(256), smem, s, *p); break;
            case I2I_F16: hipLaunchKernelGGL((lora_merge_lnf_kernel<_Float16>), gl, dim3(256), smem, s, *p); break;
            default: return i2i::fail(I2I_ERR_BAD_ARG, "lora_merge: dtype %d", dtype);
        }
        return i2i::check_launch("lora_merge<ln fold>");
    }
    switch (dtype) {
        case I2I_F32: hipLaunchKernelGGL((lora_merge_kernel<float>), grid, dim3(256), 0, s, *p); break;
        case I2I_BF16: hipLaunchKernelGGL((lora_merge_kernel<__bf16>), grid, dim3(256), 0, s, *p); break;
        case I2I_F16: hipLaunchKernelGGL((lora_merge_kernel<_Float16>), grid, dim3(256), 0, s, *p); break;
        default: return i2i::fail(I2I_ERR_BAD_ARG, "lora_merge: dtype %d", dtype);
    }
    return i2i::check_launch("lora_merge");
}

extern "C" int i2i_twin_fold(const i2i_twin_fold_params* p, int dtype, void* stream) {
    if (!p || !p->dst || !p->w_pre || !p->w_cur) return i2i::fail(I2I_ERR_BAD_ARG, "twin_fold: null operand");
    if (p->rank_pre > 0 && (!p->a_pre || !p->b_pre)) return i2i::fail(I2I_ERR_BAD_ARG, "twin_fold: rank %d without A/B (pretrained branch)", p->rank_pre);
    if (p->rank_cur > 0 && (!p->a_cur || !p->b_cur)) return i2i::fail(I2I_ERR_BAD_ARG, "twin_fold: rank %d without A/B (current branch)", p->rank_cur);
    if (p->N <= 0 || p->K <= 0 || (p->K & 3) || p->rank_pre < 0 || p->rank_cur < 0)
        return i2i::fail(I2I_ERR_BAD_ARG, "twin_fold: bad shape N=%d K=%d ranks=%d,%d", p->N, p->K, p->rank_pre, p->rank_cur);
    if (p->bias && (!p->bias_pre || !p->bias_cur)) return i2i::fail(I2I_ERR_BAD_ARG, "twin_fold: bias without bias_pre / bias_cur");
    const dim3 grid((unsigned)((p->K / 4 + 255) / 256), (unsigned)((p->N + LM_ROWS - 1) / LM_ROWS));
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case I2I_F32: hipLaunchKernelGGL((twin_fold_kernel<float>), grid, dim3(256), 0, s, *p); break;
        case I2I_BF16: hipLaunchKernelGGL((twin_fold_kernel<__bf16>), grid, dim3(256), 0, s, *p); break;
        case I2I_F16: hipLaunchKernelGGL((twin_fold_kernel<_Float16>), grid, dim3(256), 0, s, *p); break;
        default: return i2i::fail(I2I_ERR_BAD_ARG, "twin_fold: dtype %d", dtype);
    }
    return i2i::check_launch("twin_fold");
}

extern "C" int i2i_merge_group_create(const i2i_lora_merge_params* layers, int n, int dtype, void** group_out) {
    if (!group_out) return i2i::fail(I2I_ERR_BAD_ARG, "merge_group_create: null group_out");
    *group_out = nullptr;
    if (!layers || n <= 0) return i2i::fail(I2I_ERR_BAD_ARG, "merge_group_create: no layers");
    if (dtype != I2I_F32 && dtype != I2I_BF16 && dtype != I2I_F16) return i2i::fail(I2I_ERR_BAD_ARG, "merge_group_create: dtype %d", dtype);
    int32_t* prefix = new (std::nothrow) int32_t[(size_t)n + 1];
    if (!prefix) return i2i::fail(I2I_ERR_RUNTIME, "merge_group_create: out of host memory");
    int64_t tiles = 0;
    int rc = I2I_OK;
    for (int l = 0; l < n && rc == I2I_OK; ++l) {
        char who[64];
        snprintf(who, sizeof(who), "merge_group_create: layer %d", l);
        rc = check_merge(layers + l, who);
        if (rc == I2I_OK && is_lnf(layers + l)) rc = i2i::fail(I2I_ERR_BAD_ARG, "%s: the LayerNorm-fold form is not grouped (run it through i2i_lora_merge)", who);
        if (rc != I2I_OK) break;
        prefix[l] = (int32_t)tiles;
        tiles += (int64_t)((layers[l].K / 4 + 255) / 256) * ((layers[l].N + LM_ROWS - 1) / LM_ROWS);
        if (tiles > 0x7fffffff) rc = i2i::fail(I2I_ERR_BAD_ARG, "%s: more than 2^31 - 1 tiles in the group", who);
    }
    if (rc != I2I_OK) { delete[] prefix; return rc; }
    prefix[n] = (int32_t)tiles;
    MergeGroup* g = new (std::nothrow) MergeGroup();
    if (!g) { delete[] prefix; return i2i::fail(I2I_ERR_RUNTIME, "merge_group_create: out of host memory"); }
    g->n = n; g->tiles = (int)tiles; g->dtype = dtype;
    g->table = (i2i_lora_merge_params*)i2i::rt_alloc((size_t)n * sizeof(i2i_lora_merge_params));
    g->prefix = (int32_t*)i2i::rt_alloc(((size_t)n + 1) * sizeof(int32_t));
    if (!g->table || !g->prefix) rc = i2i::fail(I2I_ERR_RUNTIME, "merge_group_create: out of device memory");
    if (rc == I2I_OK) rc = i2i::rt_upload(g->table, layers, (size_t)n * sizeof(i2i_lora_merge_params));
    if (rc == I2I_OK) rc = i2i::rt_upload(g->prefix, prefix, ((size_t)n + 1) * sizeof(int32_t));
    delete[] prefix;
    if (rc != I2I_OK) { i2i_merge_group_destroy(g); return rc; }
    *group_out = g;
    return I2I_OK;
}

extern "C" int i2i_merge_group_run(void* group, void* stream) {
    if (!group) return i2i::fail(I2I_ERR_BAD_ARG, "merge_group_run: null group");
    const MergeGroup* g = (const MergeGroup*)group;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)g->tiles);
    switch (g->dtype) {
        case I2I_F32: hipLaunchKernelGGL((lora_merge_group_kernel<float>), grid, dim3(256), 0, s, g->table, g->prefix, g->n); break;
        case I2I_BF16: hipLaunchKernelGGL((lora_merge_group_kernel<__bf16>), grid, dim3(256), 0, s, g->table, g->prefix, g->n); break;
        default: hipLaunchKernelGGL((lora_merge_group_kernel<_Float16>), grid, dim3(256), 0, s, g->table, g->prefix, g->n); break;
    }
    return i2i::check_launch("merge_group_run");
}

extern "C" int i2i_merge_group_destroy(void* group) {
    if (!group) return I2I_OK;
    MergeGroup* g = (MergeGroup*)group;
    if (g->table) i2i::rt_free(g->table);
    if (g->prefix) i2i::rt_free(g->prefix);
    delete g;
    return I2I_OK;
}

// Device-side uint8 image pre-processing of the callers: LANCZOS resize, Canny.
//
// LANCZOS resize of uint8 HWC image batches, bit-identical to Pillow's Image.resize(..., Image.LANCZOS)
// (the reference resizes on the host: src/inference_paired.py:38-41 to a multiple of 8, src/inference_unpaired.py:40,53 to the
// model size and back).  HBM-bound byte work: Pillow's two separable passes (horizontal, then vertical) in 32-bit integer
// arithmetic on 22-bit fixed-point weights; the per-coordinate tap windows and weights come from the host
// (img2img_turbo_amd/image_ops.py restates Pillow's precompute_coeffs / normalize_coeffs_8bpc in double precision).
//   out = clip8((2^21 + sum_t in[first + t] * k[t]) >> 22)
// Horizontal pass: a thread per output pixel, one 8-byte load per tap; vertical pass: a thread per 4 bytes of the flattened row.
// i2i_resize_u8_ragged runs the same passes over a batch of images of different sizes (descriptors and tables on the device), and
// i2i_lanczos_tables restates the host-side table computation for callers that are not Python.
//
// Canny (second half of the file): cv::Canny for 8-bit input, aperture 3, L1 gradient, in integer arithmetic (the contract is the
// comment of i2i_canny_u8_params in include/i2i_turbo.h; the reference runs it on the host: src/image_prep.py:6-12).
#include <cmath>
#include <vector>

#include "i2i_dev.h"
#include "launch.h"

namespace {

__device__ __forceinline__ uint8_t clip8(int32_t acc) {
    const int v = acc >> 22;                                  // arithmetic shift, as Pillow's clip8 table index
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Horizontal pass: one thread per output pixel.  A tap's c <= 4 channel bytes are fetched as ONE 8-byte load from the enclosing
// aligned dword pair (the tensor base is at least 4-byte aligned) instead of c byte loads.
__global__ __launch_bounds__(256) void resize_h_u8_kernel(const i2i_resize_u8_params p) {
    const int wo = p.nout;
    const int64_t total = (int64_t)p.n * p.hin * wo;
    const uint8_t* __restrict__ base = (const uint8_t*)p.src;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int xo = (int)(i % wo);
        const int64_t row = i / wo;                           // (image, y) flattened
        const int first = p.bounds[2 * xo], cnt = p.bounds[2 * xo + 1];
        const int32_t* __restrict__ k = p.coeffs + (int64_t)xo * p.ksize;
        int64_t a = (row * p.win + first) * p.c;              // byte offset of the first tap's channel 0
        int32_t acc[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) acc[ch] = 1 << 21;
        const int64_t nbytes = (int64_t)p.n * p.hin * p.win * p.c;
        if (a + (int64_t)cnt * p.c + 8 <= nbytes) {
            for (int t = 0; t < cnt; ++t) {
                const uint32_t* q = (const uint32_t*)(base + (a & ~(int64_t)3));
                const uint64_t v = ((uint64_t)q[0] | ((uint64_t)q[1] << 32)) >> (8 * (int)(a & 3));
                const int32_t w = k[t];
#pragma unroll
                for (int ch = 0; ch < 4; ++ch)
                    if (ch < p.c) acc[ch] += (int32_t)((v >> (8 * ch)) & 0xff) * w;
                a += p.c;
            }
        } else {                                              // the last pixels of the batch: no read past the tensor's end
            for (int t = 0; t < cnt; ++t) {
                const int32_t w = k[t];
#pragma unroll
                for (int ch = 0; ch < 4; ++ch)
                    if (ch < p.c) acc[ch] += (int32_t)base[a + ch] * w;
                a += p.c;
            }
        }
        uint8_t* d = (uint8_t*)p.dst + i * p.c;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
            if (ch < p.c) d[ch] = clip8(acc[ch]);
    }
}

// Vertical pass: every byte of an output row takes the same taps, so a thread owns 4 consecutive bytes of the flattened
// [w * c] row (dword loads / one dword store) when the row length is a multiple of 4, else single bytes.
template <int VEC>
__global__ __launch_bounds__(256) void resize_v_u8_kernel(const i2i_resize_u8_params p) {
    const int rowb = p.win * p.c, units = rowb / VEC;
    const int64_t total = (int64_t)p.n * p.nout * units;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int u = (int)(i % units);
        const int64_t r = i / units;
        const int yo = (int)(r % p.nout), img = (int)(r / p.nout);
        const int first = p.bounds[2 * yo], cnt = p.bounds[2 * yo + 1];
        const int32_t* __restrict__ k = p.coeffs + (int64_t)yo * p.ksize;
        const uint8_t* __restrict__ s = (const uint8_t*)p.src + ((int64_t)img * p.hin + first) * rowb + (int64_t)u * VEC;
        int32_t acc[VEC];
#pragma unroll
        for (int b = 0; b < VEC; ++b) acc[b] = 1 << 21;
        for (int t = 0; t < cnt; ++t) {
            const int32_t w = k[t];
            if constexpr (VEC == 4) {
                const uint32_t v = *(const uint32_t*)s;
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[b] += (int32_t)((v >> (8 * b)) & 0xff) * w;
            } else {
                acc[0] += (int32_t)s[0] * w;
            }
            s += rowb;
        }
        uint8_t* d = (uint8_t*)p.dst + ((int64_t)img * p.nout + yo) * rowb + (int64_t)u * VEC;
        if constexpr (VEC == 4) {
            *(uint32_t*)d = (uint32_t)clip8(acc[0]) | ((uint32_t)clip8(acc[1]) << 8) | ((uint32_t)clip8(acc[2]) << 16) | ((uint32_t)clip8(acc[3]) << 24);
        } else {
            d[0] = clip8(acc[0]);
        }
    }
}

}  // namespace

extern "C" int i2i_resize_u8(const i2i_resize_u8_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p || !p->src || !p->dst || !p->bounds || !p->coeffs) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8: null pointer");
    if (p->c < 1 || p->c > 4 || p->n < 1 || p->hin < 1 || p->win < 1 || p->nout < 1 || p->ksize < 1 || (p->axis != 0 && p->axis != 1))
        return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8: bad geometry");
    if (((uintptr_t)p->src | (uintptr_t)p->dst) & 3) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8: image batches must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    auto blocks = [](int64_t total) { const int64_t b = (total + 255) / 256; return (unsigned)(b < 65536 ? b : 65536); };
    if (p->axis == 1) {
        hipLaunchKernelGGL(resize_h_u8_kernel, dim3(blocks((int64_t)p->n * p->hin * p->nout)), dim3(256), 0, s, *p);
    } else {
        const int rowb = p->win * p->c;
        if (rowb % 4 == 0) hipLaunchKernelGGL(resize_v_u8_kernel<4>, dim3(blocks((int64_t)p->n * p->nout * (rowb / 4))), dim3(256), 0, s, *p);
        else hipLaunchKernelGGL(resize_v_u8_kernel<1>, dim3(blocks((int64_t)p->n * p->nout * rowb)), dim3(256), 0, s, *p);
    }
    return i2i::check_launch("resize_u8");
}

// ------------------------------------------------------------------------------------------------------------------------
// Ragged batch (i2i_resize_u8_ragged, the contract is the comment of i2i_resize_u8_ragged_params in include/i2i_turbo.h): the same two
// passes with everything that differs between images -- extents, arena offsets, tap tables -- read from a device descriptor.  Grid y = image,
// grid x = a capacity hint; every workgroup first decides whether its image is empty, valid or rejected (the same verdict in every
// workgroup of that image: it depends on the descriptor, the table and the launch parameters only), then strides over the image's outputs.
namespace {

constexpr int RAGGED_MAX_X = 1024;                           // workgroups per image at most

// 0 = empty slot, 1 = run, -1 = rejected.  Called by all 256 threads of the workgroup (two barriers); i2i_smem holds one int.
__device__ int ragged_verdict(const i2i_resize_u8_ragged_params& p, const i2i_resize_image& d) {
    if (d.hin == 0 || d.win == 0) return 0;
    bool ok = d.hin > 0 && d.win > 0 && d.nout >= 1 && d.ksize >= 1 && d.src_off >= 0 && d.dst_off >= 0 && ((d.src_off | d.dst_off) & 3) == 0 &&
              d.src_off <= p.src_bytes && d.dst_off <= p.dst_bytes && d.bounds_off >= 0 && d.coeffs_off >= 0 && d.bounds_off <= p.tables_len &&
              d.coeffs_off <= p.tables_len;
    if (ok) {                                                // sizes as quotients: no product can overflow
        const int64_t spx = (int64_t)d.hin * d.win;
        const int64_t dpx = p.axis == 1 ? (int64_t)d.hin * d.nout : (int64_t)d.nout * d.win;
        ok = spx <= (p.src_bytes - d.src_off) / p.c && dpx <= (p.dst_bytes - d.dst_off) / p.c && 2 * (int64_t)d.nout <= p.tables_len - d.bounds_off &&
             (int64_t)d.nout * d.ksize <= p.tables_len - d.coeffs_off;
    }
    int* verdict = (int*)i2i_smem;
    if (threadIdx.x == 0) *verdict = ok ? 1 : 0;
    __syncthreads();
    if (ok) {                                                // every bounds row: the taps it names lie inside the source extent and the weight row
        const int extent = p.axis == 1 ? d.win : d.hin;
        const int32_t* __restrict__ b = p.tables + d.bounds_off;
        bool rows_ok = true;
        for (int o = (int)threadIdx.x; o < d.nout; o += 256) {
            const int first = b[2 * o], cnt = b[2 * o + 1];
            rows_ok = rows_ok && first >= 0 && cnt >= 0 && cnt <= d.ksize && first <= extent - cnt;
        }
        if (!rows_ok) *verdict = 0;                          // (every writer stores the same 0)
    }
    __syncthreads();
    const int v = *verdict;
    __syncthreads();                                         // the word is reused for the workgroup's next image
    return v ? 1 : -1;
}

__device__ __forceinline__ void ragged_h_image(const i2i_resize_u8_ragged_params& p, const i2i_resize_image& d) {
    const int wo = d.nout, c = p.c;
    const int64_t total = (int64_t)d.hin * wo;
    const uint8_t* __restrict__ base = (const uint8_t*)p.src;                 // the ARENA: `a` below is an arena offset
    const int32_t* __restrict__ bounds = p.tables + d.bounds_off;
    const int32_t* __restrict__ coeffs = p.tables + d.coeffs_off;
    uint8_t* __restrict__ dst = (uint8_t*)p.dst + d.dst_off;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int xo = (int)(i % wo);
        const int64_t y = i / wo;
        const int first = bounds[2 * xo], cnt = bounds[2 * xo + 1];
        const int32_t* __restrict__ k = coeffs + (int64_t)xo * d.ksize;
        int64_t a = d.src_off + (y * d.win + first) * c;
        int32_t acc[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) acc[ch] = 1 << 21;
        if (a + (int64_t)cnt * c + 8 <= p.src_bytes) {       // the last window ends at most 8 - c bytes behind the last tap: inside the arena
            for (int t = 0; t < cnt; ++t) {
                const uint32_t* q = (const uint32_t*)(base + (a & ~(int64_t)3));
                const uint64_t v = ((uint64_t)q[0] | ((uint64_t)q[1] << 32)) >> (8 * (int)(a & 3));
                const int32_t w = k[t];
#pragma unroll
                for (int ch = 0; ch < 4; ++ch)
                    if (ch < c) acc[ch] += (int32_t)((v >> (8 * ch)) & 0xff) * w;
                a += c;
            }
        } else {                                             // the last pixels of the arena: the image's own bytes only
            for (int t = 0; t < cnt; ++t) {
                const int32_t w = k[t];
#pragma unroll
                for (int ch = 0; ch < 4; ++ch)
                    if (ch < c) acc[ch] += (int32_t)base[a + ch] * w;
                a += c;
            }
        }
        uint8_t* o = dst + i * c;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
            if (ch < c) o[ch] = clip8(acc[ch]);
    }
}

template <int VEC>
__device__ __forceinline__ void ragged_v_image(const i2i_resize_u8_ragged_params& p, const i2i_resize_image& d) {
    const int64_t rowb = (int64_t)d.win * p.c, units = rowb / VEC;
    const int64_t total = (int64_t)d.nout * units;
    const int32_t* __restrict__ bounds = p.tables + d.bounds_off;
    const int32_t* __restrict__ coeffs = p.tables + d.coeffs_off;
    const uint8_t* __restrict__ src = (const uint8_t*)p.src + d.src_off;
    uint8_t* __restrict__ dst = (uint8_t*)p.dst + d.dst_off;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t u = i % units;
        const int yo = (int)(i / units);
        const int first = bounds[2 * yo], cnt = bounds[2 * yo + 1];
        const int32_t* __restrict__ k = coeffs + (int64_t)yo * d.ksize;
        const uint8_t* __restrict__ s = src + (int64_t)first * rowb + u * VEC;
        int32_t acc[VEC];
#pragma unroll
        for (int b = 0; b < VEC; ++b) acc[b] = 1 << 21;
        for (int t = 0; t < cnt; ++t) {
            const int32_t w = k[t];
            if constexpr (VEC == 4) {
                const uint32_t v = *(const uint32_t*)s;
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[b] += (int32_t)((v >> (8 * b)) & 0xff) * w;
            } else {
                acc[0] += (int32_t)s[0] * w;
            }
            s += rowb;
        }
        uint8_t* o = dst + (int64_t)yo * rowb + u * VEC;
        if constexpr (VEC == 4) {
            *(uint32_t*)o = (uint32_t)clip8(acc[0]) | ((uint32_t)clip8(acc[1]) << 8) | ((uint32_t)clip8(acc[2]) << 16) | ((uint32_t)clip8(acc[3]) << 24);
        } else {
            o[0] = clip8(acc[0]);
        }
    }
}

__global__ __launch_bounds__(256) void resize_ragged_u8_kernel(const i2i_resize_u8_ragged_params p) {
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_resize_image d = p.images[b];
        const int v = ragged_verdict(p, d);
        if (v < 0 && p.bad_mask && blockIdx.x == 0 && threadIdx.x == 0) agent_or_u32(p.bad_mask, 1u << (b & 31));
        if (v <= 0) continue;
        if (p.axis == 1) ragged_h_image(p, d);
        else if (((int64_t)d.win * p.c) % 4 == 0) ragged_v_image<4>(p, d);   // rows of whole dwords (the image base is 4-byte aligned)
        else ragged_v_image<1>(p, d);
    }
}

// Pillow's filters (src/libImaging/Resample.c: sinc_filter, lanczos_filter, bicubic_filter)
inline double lanczos_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return sin(x) / x;
}
inline double lanczos_weight(double x) { return (-3.0 <= x && x < 3.0) ? lanczos_sinc(x) * lanczos_sinc(x / 3) : 0.0; }
// Keys' cubic with a = -0.5, statement for statement as Pillow evaluates it (no fused multiply-add: the weights are rounded to 22 bits)
inline double bicubic_weight(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
struct resample_filter { double (*weight)(double); double support; };
inline const resample_filter* resample_filter_of(int filter) {
    static const resample_filter lanczos = {lanczos_weight, 3.0}, bicubic = {bicubic_weight, 2.0};
    return filter == I2I_FILTER_LANCZOS ? &lanczos : (filter == I2I_FILTER_BICUBIC ? &bicubic : nullptr);
}

}  // namespace

extern "C" int i2i_resize_u8_ragged(const i2i_resize_u8_ragged_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: null pointer");
    if (p->c < 1 || p->c > 4) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: c = %d outside 1..4", p->c);
    if (p->n < 0) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: n = %d < 0", p->n);
    if (p->axis != 0 && p->axis != 1) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: axis = %d (1 = horizontal, 0 = vertical)", p->axis);
    if (p->grid_units < 1) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: grid_units must be >= 1");
    if (p->src_bytes < 0 || p->dst_bytes < 0 || p->tables_len < 0) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: negative arena / pool size");
    if (p->n == 0) return I2I_OK;
    if (!p->src || !p->dst || !p->images || !p->tables) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: null pointer (src, dst, images, tables)");
    if (((uintptr_t)p->src | (uintptr_t)p->dst | (uintptr_t)p->tables | (uintptr_t)p->bad_mask) & 3)
        return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: src, dst, tables and bad_mask must be 4-byte aligned");
    if ((uintptr_t)p->images & 7) return i2i::fail(I2I_ERR_BAD_ARG, "resize_u8_ragged: images must be 8-byte aligned");
    const int64_t bx = (p->grid_units + 255) / 256;
    const dim3 grid((unsigned)(bx < RAGGED_MAX_X ? bx : RAGGED_MAX_X), (unsigned)(p->n < 65535 ? p->n : 65535));
    hipLaunchKernelGGL(resize_ragged_u8_kernel, grid, dim3(256), 16, (hipStream_t)stream, *p);
    return i2i::check_launch("resize_u8_ragged");
}

// `what` names the entry in error messages (i2i_lanczos_* are the LANCZOS case of i2i_resample_*)
static int resample_ksize(const char* what, const resample_filter* f, int in_size, int out_size) {
    if (!f) return i2i::fail(I2I_ERR_BAD_ARG, "%s_ksize: unknown filter", what);
    if (in_size < 1 || out_size < 1) return i2i::fail(I2I_ERR_BAD_ARG, "%s_ksize: sizes must be >= 1", what);
    const double scale = (double)in_size / out_size, support = f->support * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc, statement for statement as image_ops.resample_coeffs; a fused multiply-add in
// `center - support + 0.5` or in the weight's argument would move tap windows, so contraction stays off here whatever the flags say
static int resample_tables(const char* what, const resample_filter* f, int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize_capacity) {
#pragma clang fp contract(off)
    if (!bounds || !coeffs) return i2i::fail(I2I_ERR_BAD_ARG, "%s_tables: null pointer", what);
    const int ksize = resample_ksize(what, f, in_size, out_size);
    if (ksize < 0) return ksize;
    if (ksize_capacity < ksize) return i2i::fail(I2I_ERR_BAD_ARG, "%s_tables: ksize_capacity %d < ksize %d", what, ksize_capacity, ksize);
    const double scale = (double)in_size / out_size, filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = f->support * filterscale, ss = 1.0 / filterscale;
    std::vector<double> kk((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double w = f->weight(((double)(x + xmin) - center + 0.5) * ss);
            kk[x] = w;
            ww += w;
        }
        int32_t* row = coeffs + (size_t)xx * ksize_capacity;
        for (int x = 0; x < ksize_capacity; ++x) {
            double v = x < xmax ? kk[x] : 0.0;
            if (x < xmax && ww != 0.0) v /= ww;
            row[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << 22)) : (int32_t)(0.5 + v * (double)(1 << 22));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

extern "C" int i2i_lanczos_ksize(int in_size, int out_size) { return resample_ksize("lanczos", resample_filter_of(I2I_FILTER_LANCZOS), in_size, out_size); }
extern "C" int i2i_lanczos_tables(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize_capacity) {
    return resample_tables("lanczos", resample_filter_of(I2I_FILTER_LANCZOS), in_size, out_size, bounds, coeffs, ksize_capacity);
}
extern "C" int i2i_resample_ksize(int filter, int in_size, int out_size) { return resample_ksize("resample", resample_filter_of(filter), in_size, out_size); }
extern "C" int i2i_resample_tables(int filter, int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize_capacity) {
    return resample_tables("resample", resample_filter_of(filter), in_size, out_size, bounds, coeffs, ksize_capacity);
}

// ------------------------------------------------------------------------------------------------------------------------
// Canny.  Five launches, whatever the image holds:
//   1 canny_nms_kernel    a workgroup per 64 x 16 tile: input with a 2-pixel halo in LDS (a pixel = one dword), Sobel + channel choice
//                         on the tile with a 1-pixel halo, non-maximum suppression -> class map (0 none, 1 weak, 2 strong)
//   2 canny_label_kernel  connected components of candidates INSIDE a tile: min-label propagation with pointer jumping in LDS to the
//                         tile-local fixpoint; label[p] = global pixel index of the tile-local root (-1: no candidate), flag[p] = 0
//   3 canny_merge_kernel  candidates on both sides of a tile edge: lock-free union of their roots (atomic min on the larger root, retry
//                         on change).  `label` is a union-find parent array whose entries only ever decrease (parent[p] <= p).
//   4 canny_flag_kernel   every strong pixel marks the root of its component
//   5 canny_emit_kernel   edge = candidate whose root is marked
// Hysteresis is therefore exact for chains of any length across any number of tiles, with no grid-wide wait and no pass count that
// depends on the image: the loop of (2) is bounded by the tile's pixel count, every union-find walk by the image's (labels strictly
// decrease along a walk).  Inside launch 3 the parent words are touched only by agent-scope atomics (i2i_dev.h agent_*); everything
// written with plain stores (class map, initial labels, flags) is read by a LATER launch only.  Workspace: label int32[P] | flag
// int32[P] | class uint8[P], P = n*h*w; every word is written before it is read in each run (nothing to zero, no state kept).
namespace {

constexpr int CTW = 64, CTH = 16, CTPIX = CTW * CTH;         // tile; 256 threads own 4 pixels each
constexpr int CPW = CTW + 4, CPH = CTH + 4;                  // input region (2-pixel halo)
constexpr int CMW = CTW + 2, CMH = CTH + 2;                  // gradient / label region (1-pixel halo)
constexpr int CANNY_INF = 1 << 20;                           // label of a non-candidate in the tile-local propagation

struct canny_ws {
    int32_t* label; int32_t* flag; uint8_t* cls;
};
__host__ __device__ __forceinline__ canny_ws canny_carve(void* ws, int64_t P) {
    canny_ws r;
    r.label = (int32_t*)ws;
    r.flag = r.label + P;
    r.cls = (uint8_t*)(r.flag + P);
    return r;
}

struct canny_tile { int img, x0, y0; };
__device__ __forceinline__ canny_tile canny_tile_of(const i2i_canny_u8_params& p, int t) {
    const int ntx = (p.w + CTW - 1) / CTW, nty = (p.h + CTH - 1) / CTH;
    canny_tile r;
    r.x0 = (t % ntx) * CTW;
    r.y0 = ((t / ntx) % nty) * CTH;
    r.img = t / (ntx * nty);
    return r;
}

// thr_stride: int32 words between the {low, high} pairs of consecutive images in p.thr_dev (0 = one pair for the batch: i2i_canny_u8;
// 2 = i2i_canny_u8_batch).  The only kernel of the five that reads thresholds.
__global__ __launch_bounds__(256) void canny_nms_kernel(const i2i_canny_u8_params p, const int thr_stride) {
    const int64_t P = (int64_t)p.n * p.h * p.w;
    const canny_ws ws = canny_carve(p.ws, P);
    const canny_tile t = canny_tile_of(p, (int)blockIdx.x);
    const int tid = (int)threadIdx.x;
    const int32_t* thr = p.thr_dev ? p.thr_dev + (int64_t)t.img * thr_stride : nullptr;
    int low = thr ? thr[0] : p.low, high = thr ? thr[1] : p.high;
    if (low > high) { const int s = low; low = high; high = s; }

    uint32_t* pix = (uint32_t*)i2i_smem;                     // [CPH][CPW], channel ch in byte ch
    int16_t* mg = (int16_t*)(pix + CPH * CPW);               // [CMH][CMW] each
    int16_t* gx = mg + CMH * CMW;
    int16_t* gy = gx + CMH * CMW;

    // input with BORDER_REPLICATE (clamped coordinates).  A pixel's c <= 4 bytes come as ONE 8-byte load from the enclosing aligned
    // dword pair (the tensor base is 4-byte aligned), as in resize_h_u8_kernel; the last pixels of the batch byte by byte
    const uint8_t* __restrict__ base = (const uint8_t*)p.src;
    const int64_t nbytes = P * p.c;
    for (int i = tid; i < CPH * CPW; i += 256) {
        const int ly = i / CPW, lx = i % CPW;
        int yy = t.y0 + ly - 2, xx = t.x0 + lx - 2;
        yy = yy < 0 ? 0 : (yy > p.h - 1 ? p.h - 1 : yy);
        xx = xx < 0 ? 0 : (xx > p.w - 1 ? p.w - 1 : xx);
        const int64_t a = (((int64_t)t.img * p.h + yy) * p.w + xx) * p.c;
        uint32_t v = 0;
        if ((a & ~(int64_t)3) + 8 <= nbytes) {
            const uint32_t* q = (const uint32_t*)(base + (a & ~(int64_t)3));
            v = (uint32_t)((((uint64_t)q[0]) | ((uint64_t)q[1] << 32)) >> (8 * (int)(a & 3)));
        } else {
            for (int ch = 0; ch < p.c; ++ch) v |= (uint32_t)base[a + ch] << (8 * ch);
        }
        pix[i] = v;
    }
    __syncthreads();

    // Sobel per channel, the channel of the largest |dx| + |dy| (the lowest one on a tie); magnitude 0 outside the image
    for (int i = tid; i < CMH * CMW; i += 256) {
        const int ly = i / CMW, lx = i % CMW;
        const int yy = t.y0 + ly - 1, xx = t.x0 + lx - 1;
        int bm = 0, bdx = 0, bdy = 0;
        if (yy >= 0 && yy < p.h && xx >= 0 && xx < p.w) {
            const uint32_t* r0 = pix + ly * CPW + lx;        // row above, column to the left
            const uint32_t* r1 = r0 + CPW;
            const uint32_t* r2 = r1 + CPW;
            const uint32_t p00 = r0[0], p01 = r0[1], p02 = r0[2], p10 = r1[0], p12 = r1[2], p20 = r2[0], p21 = r2[1], p22 = r2[2];
            bm = -1;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                if (ch < p.c) {
                    const int s = 8 * ch;
                    const int a00 = (p00 >> s) & 0xff, a01 = (p01 >> s) & 0xff, a02 = (p02 >> s) & 0xff, a10 = (p10 >> s) & 0xff;
                    const int a12 = (p12 >> s) & 0xff, a20 = (p20 >> s) & 0xff, a21 = (p21 >> s) & 0xff, a22 = (p22 >> s) & 0xff;
                    const int dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
                    const int dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
                    const int m = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
                    if (m > bm) { bm = m; bdx = dx; bdy = dy; }
                }
            }
        }
        mg[i] = (int16_t)bm;
        gx[i] = (int16_t)bdx;
        gy[i] = (int16_t)bdy;
    }
    __syncthreads();

#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + k * 256, ly = i / CTW, lx = i % CTW;
        const int yy = t.y0 + ly, xx = t.x0 + lx;
        if (yy >= p.h || xx >= p.w) continue;
        const int16_t* c = mg + (ly + 1) * CMW + lx + 1;
        const int m = c[0];
        int cls = 0;
        if (m > low) {
            const int dx = gx[(ly + 1) * CMW + lx + 1], dy = gy[(ly + 1) * CMW + lx + 1];
            const int ax = dx < 0 ? -dx : dx, ay = (dy < 0 ? -dy : dy) << 15;
            const int tg22x = ax * 13573, tg67x = tg22x + (ax << 16);
            bool keep;
            if (ay < tg22x) keep = m > c[-1] && m >= c[1];
            else if (ay > tg67x) keep = m > c[-CMW] && m >= c[CMW];
            else {
                const int s = ((dx ^ dy) < 0) ? -1 : 1;
                keep = m > c[-CMW - s] && m > c[CMW + s];
            }
            if (keep) cls = m > high ? 2 : 1;
        }
        ws.cls[((int64_t)t.img * p.h + yy) * p.w + xx] = (uint8_t)cls;
    }
}

__global__ __launch_bounds__(256) void canny_label_kernel(const i2i_canny_u8_params p) {
    const int64_t P = (int64_t)p.n * p.h * p.w;
    const canny_ws ws = canny_carve(p.ws, P);
    const canny_tile t = canny_tile_of(p, (int)blockIdx.x);
    const int tid = (int)threadIdx.x;
    int* lab = (int*)i2i_smem;                               // [CMH][CMW]: tile-local index of the smallest pixel known to be connected
    int* chg = lab + CMH * CMW;                              // [2]: "some label moved" of the even / odd sweeps
    for (int i = tid; i < CMH * CMW; i += 256) lab[i] = CANNY_INF;
    if (tid == 0) chg[0] = chg[1] = 0;
    __syncthreads();
    int pos[4], cur[4];
    int64_t g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + k * 256, ly = i / CTW, lx = i % CTW;
        const int yy = t.y0 + ly, xx = t.x0 + lx;
        pos[k] = (ly + 1) * CMW + lx + 1;
        g[k] = (yy < p.h && xx < p.w) ? ((int64_t)t.img * p.h + yy) * p.w + xx : -1;
        cur[k] = (g[k] >= 0 && ws.cls[g[k]] != 0) ? i : CANNY_INF;
        lab[pos[k]] = cur[k];
    }
    __syncthreads();
    // Sweep = every candidate takes the minimum over its 3 x 3 neighbourhood, then the label of THAT pixel (pointer jumping); reads and
    // writes of a sweep are separated by barriers.  Labels never fall below their component's minimum and fall at least as fast as under
    // plain propagation, which reaches the fixpoint within the longest geodesic of the tile (< CTPIX sweeps): the bound is never the exit.
    for (int it = 0; it < CTPIX; ++it) {
        int nl[4];
        bool moved = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nl[k] = cur[k];
            if (cur[k] == CANNY_INF) continue;
            const int* c = lab + pos[k];
            int m = cur[k];
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) m = min(m, c[dy * CMW + dx]);
            m = min(m, lab[(m / CTW + 1) * CMW + (m % CTW) + 1]);
            nl[k] = m;
            moved |= m < cur[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (nl[k] < cur[k]) lab[pos[k]] = cur[k] = nl[k];
        if (moved) chg[it & 1] = 1;
        if (tid == 0) chg[(it + 1) & 1] = 0;
        __syncthreads();
        if (!chg[it & 1]) break;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (g[k] < 0) continue;
        int32_t root = -1;
        if (cur[k] != CANNY_INF) root = (int32_t)((((int64_t)t.img * p.h + t.y0 + cur[k] / CTW) * p.w) + t.x0 + cur[k] % CTW);
        ws.label[g[k]] = root;
        ws.flag[g[k]] = 0;
    }
}

// root of x in launch 3, where other workgroups lower parent words concurrently: atomic loads only; the walk strictly descends
__device__ __forceinline__ int32_t canny_find_live(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t n = agent_load_i32(parent + x);
        if (n == x) return x;
        x = n;
    }
}
// root of x once the parent array is final (launches 4 and 5)
__device__ __forceinline__ int32_t canny_find(const int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t n = parent[x];
        if (n == x) return x;
        x = n;
    }
}
// Lock-free union: hang the larger root under the smaller one with an atomic min.  If the word was no longer a root (another union got
// there first and left `old` < a in it) it now holds min(old, b) and the other of the two still has to be joined: go on with (old, b).
// Every retry continues from a strictly smaller index.
__device__ __forceinline__ void canny_union(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = canny_find_live(parent, a);
        b = canny_find_live(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t s = a; a = b; b = s; }
        const int32_t old = agent_min_i32(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// a thread per pixel of the first row / first column of a tile (only those do anything): its candidate neighbours in the row above /
// the column to the left lie in other tiles (diagonal tiles included)
__global__ __launch_bounds__(256) void canny_merge_kernel(const i2i_canny_u8_params p) {
    const int64_t P = (int64_t)p.n * p.h * p.w;
    const canny_ws ws = canny_carve(p.ws, P);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % p.w), y = (int)((i / p.w) % p.h);
        const bool top = (y % CTH) == 0 && y > 0, left = (x % CTW) == 0 && x > 0;
        if (!(top || left) || ws.cls[i] == 0) continue;
        if (top) {
            for (int dx = -1; dx <= 1; ++dx) {
                if (x + dx < 0 || x + dx >= p.w) continue;
                const int64_t j = i - p.w + dx;
                if (ws.cls[j] != 0) canny_union(ws.label, (int32_t)i, (int32_t)j);
            }
        }
        if (left) {
            for (int dy = -1; dy <= 1; ++dy) {
                if (y + dy < 0 || y + dy >= p.h) continue;
                const int64_t j = i + (int64_t)dy * p.w - 1;
                if (ws.cls[j] != 0) canny_union(ws.label, (int32_t)i, (int32_t)j);
            }
        }
    }
}

__global__ __launch_bounds__(256) void canny_flag_kernel(const i2i_canny_u8_params p) {
    const int64_t P = (int64_t)p.n * p.h * p.w;
    const canny_ws ws = canny_carve(p.ws, P);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256)
        if (ws.cls[i] == 2) ws.flag[canny_find(ws.label, (int32_t)i)] = 1;      // (every writer stores the same 1; read by launch 5)
}

// a thread per 4 consecutive pixels: whole dwords of the output where all four exist (dst is 4-byte aligned)
__global__ __launch_bounds__(256) void canny_emit_kernel(const i2i_canny_u8_params p) {
    const int64_t P = (int64_t)p.n * p.h * p.w;
    const canny_ws ws = canny_carve(p.ws, P);
    const int64_t groups = (P + 3) / 4;
    uint8_t* dst = (uint8_t*)p.dst;
    for (int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * 256) {
        const int64_t i0 = gi * 4;
        uint32_t e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k;
            e[k] = (i < P && ws.cls[i] != 0 && ws.flag[canny_find(ws.label, (int32_t)i)] != 0) ? 0xffu : 0u;
        }
        if (i0 + 4 <= P && p.out_c == 1) {
            *(uint32_t*)(dst + i0) = e[0] | (e[1] << 8) | (e[2] << 16) | (e[3] << 24);
        } else if (i0 + 4 <= P) {                            // out_c == 3: 12 bytes
            uint32_t* d = (uint32_t*)(dst + i0 * 3);
            d[0] = e[0] * 0x010101u | (e[1] << 24);
            d[1] = e[1] * 0x0101u | (e[2] << 16) | (e[2] << 24);
            d[2] = e[2] | (e[3] * 0x010101u << 8);
        } else {
            for (int k = 0; k < 4 && i0 + k < P; ++k)
                for (int ch = 0; ch < p.out_c; ++ch) dst[(i0 + k) * p.out_c + ch] = (uint8_t)e[k];
        }
    }
}

}  // namespace

extern "C" size_t i2i_canny_ws_bytes(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1) return 0;
    const size_t P = (size_t)n * (size_t)h * (size_t)w;
    return (P * 9 + 15) & ~(size_t)15;
}

// both entries: the checks and the five launches
static int canny_launch(const char* what, const i2i_canny_u8_params* p, int thr_stride, void* stream) {
    if (!p->src || !p->dst || !p->ws) return i2i::fail(I2I_ERR_BAD_ARG, "%s: null pointer", what);
    if (p->c < 1 || p->c > 4 || (p->out_c != 1 && p->out_c != 3) || p->n < 1 || p->h < 1 || p->w < 1)
        return i2i::fail(I2I_ERR_BAD_ARG, "%s: bad geometry (c 1..4, out_c 1 or 3, positive sizes)", what);
    const int64_t P = (int64_t)p->n * p->h * p->w;
    if (P > 0x7fffffff) return i2i::fail(I2I_ERR_BAD_ARG, "%s: more than 2^31 - 1 pixels in the batch (labels are 32-bit pixel indices)", what);
    if (((uintptr_t)p->src | (uintptr_t)p->dst) & 3) return i2i::fail(I2I_ERR_BAD_ARG, "%s: image batches must be 4-byte aligned", what);
    if ((uintptr_t)p->ws & 15) return i2i::fail(I2I_ERR_BAD_ARG, "%s: the workspace must be 16-byte aligned", what);
    if ((uintptr_t)p->thr_dev & 3) return i2i::fail(I2I_ERR_BAD_ARG, "%s: thr_dev must be 4-byte aligned", what);
    hipStream_t s = (hipStream_t)stream;
    const int64_t tiles = (int64_t)p->n * ((p->h + CTH - 1) / CTH) * ((p->w + CTW - 1) / CTW);
    auto blocks = [](int64_t total) { const int64_t b = (total + 255) / 256; return (unsigned)(b < 65536 ? b : 65536); };
    const size_t lds_nms = CPH * CPW * 4 + 3 * CMH * CMW * 2, lds_lab = (CMH * CMW + 2) * 4;
    hipLaunchKernelGGL(canny_nms_kernel, dim3((unsigned)tiles), dim3(256), lds_nms, s, *p, thr_stride);
    hipLaunchKernelGGL(canny_label_kernel, dim3((unsigned)tiles), dim3(256), lds_lab, s, *p);
    hipLaunchKernelGGL(canny_merge_kernel, dim3(blocks(P)), dim3(256), 0, s, *p);
    hipLaunchKernelGGL(canny_flag_kernel, dim3(blocks(P)), dim3(256), 0, s, *p);
    hipLaunchKernelGGL(canny_emit_kernel, dim3(blocks((P + 3) / 4)), dim3(256), 0, s, *p);
    return i2i::check_launch(what);
}

extern "C" int i2i_canny_u8(const i2i_canny_u8_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "canny_u8: null pointer");
    return canny_launch("canny_u8", p, 0, stream);
}

extern "C" int i2i_canny_u8_batch(const i2i_canny_u8_batch_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "canny_u8_batch: null pointer");
    if (!p->thr) return i2i::fail(I2I_ERR_BAD_ARG, "canny_u8_batch: thr (device int32 [n][2]) is required");
    i2i_canny_u8_params q;
    q.src = p->src; q.dst = p->dst;
    q.n = p->n; q.h = p->h; q.w = p->w; q.c = p->c; q.out_c = p->out_c;
    q.low = q.high = 0;
    q.thr_dev = p->thr;
    q.ws = p->ws;
    return canny_launch("canny_u8_batch", &q, 2, stream);
}

// ------------------------------------------------------------------------------------------------------------------------
// Automatic per-image Canny thresholds (i2i_canny_auto_thr, the contract is the comment of i2i_canny_auto_thr_params in include/i2i_turbo.h):
// the median rule on the byte histogram of every image, written into the {low, high} table canny_nms_kernel reads.  Three launches:
//   1 canny_hist_clear_kernel  ws[n][256] = 0
//   2 canny_hist_kernel        grid (slices of an image, images), capped in total like scan_batch_kernel (elementwise.hip); a workgroup
//                              works on one image at a time: 16-byte loads on the image's aligned part, byte loads on its head and tail (the
//                              split comes from THAT image's start address), counts into one 256-bin copy per wave in LDS (a photograph puts
//                              most bytes into a few neighbouring bins: one shared copy serialises on them), then one agent-scope add per
//                              non-zero bin into the image's row of ws
//   3 canny_select_kernel      one wave per image: lane l owns bins 4l .. 4l + 3, inclusive wave scan of the lane totals, the two middle
//                              ranks, the formula, plain stores
// Images with a negative sigma (manual sliders) are skipped by 2 and 3.
namespace {

constexpr int HIST_THREADS = 256, HIST_WAVES = HIST_THREADS / 64;
constexpr int HIST_MAX_GRID = 1024;                          // workgroups of one launch at most (as SCAN_BATCH_MAX_GRID)
constexpr int HIST_CHUNKS_PER_WG = 1024;                     // 16-byte chunks a workgroup is sized for (4 per lane)

__global__ __launch_bounds__(256) void canny_hist_clear_kernel(uint32_t* hist, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) hist[i] = 0;
}

__device__ __forceinline__ void hist_word(uint32_t* mine, uint32_t v) {
    lds_add_u32(mine + (v & 0xff), 1);
    lds_add_u32(mine + ((v >> 8) & 0xff), 1);
    lds_add_u32(mine + ((v >> 16) & 0xff), 1);
    lds_add_u32(mine + (v >> 24), 1);
}

__global__ __launch_bounds__(HIST_THREADS) void canny_hist_kernel(const i2i_canny_auto_thr_params p) {
    uint32_t* lds = (uint32_t*)i2i_smem;                     // [HIST_WAVES][256]
    const int tid = (int)threadIdx.x;
    uint32_t* mine = lds + (tid >> 6) * 256;
    const int64_t N = (int64_t)p.h * p.w * p.c;
    uint32_t* hist = (uint32_t*)p.ws;
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        if (p.sigma_q16[b] < 0) continue;                    // (the same verdict in every lane: no barrier is skipped by a part of the workgroup)
#pragma unroll
        for (int w = 0; w < HIST_WAVES; ++w) lds[w * 256 + tid] = 0;
        __syncthreads();
        const uint8_t* __restrict__ x = (const uint8_t*)p.src + (int64_t)b * N;
        const int64_t mis = (int64_t)((uintptr_t)x & 15);
        const int64_t head = mis ? (16 - mis < N ? 16 - mis : N) : 0;
        const int64_t nb = (N - head) / 16, tail = N - head - nb * 16;
        const u32x4* __restrict__ body = (const u32x4*)(x + head);
        for (int64_t i = (int64_t)blockIdx.x * HIST_THREADS + tid; i < nb; i += (int64_t)gridDim.x * HIST_THREADS) {
            const u32x4 v = body[i];
            hist_word(mine, v[0]);
            hist_word(mine, v[1]);
            hist_word(mine, v[2]);
            hist_word(mine, v[3]);
        }
        // the < 16 bytes in front of the first 16-byte boundary and the < 16 behind the last whole chunk
        for (int64_t i = (int64_t)blockIdx.x * HIST_THREADS + tid; i < head + tail; i += (int64_t)gridDim.x * HIST_THREADS)
            lds_add_u32(mine + x[i < head ? i : i + nb * 16], 1);
        __syncthreads();
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < HIST_WAVES; ++w) tot += lds[w * 256 + tid];
        if (tot) agent_add_u32(hist + (int64_t)b * 256 + tid, tot);
        __syncthreads();                                     // the copies are free again before the next image of this workgroup zeroes them
    }
}

// value of 0-based rank r, if it lies in this lane's four bins (lo = count of bytes below the lane's first bin), else 0: exactly one
// lane of the wave finds it, so the wave sum of the returns is the value
__device__ __forceinline__ int select_rank(const uint32_t c[4], uint32_t lo, uint32_t r, int first_bin) {
    int v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (r >= lo && r < lo + c[k]) v = first_bin + k;
        lo += c[k];
    }
    return v;
}

__global__ __launch_bounds__(64) void canny_select_kernel(const i2i_canny_auto_thr_params p) {
    const int lane = (int)threadIdx.x;
    const uint32_t N = (uint32_t)((int64_t)p.h * p.w * p.c);
    for (int b = (int)blockIdx.x; b < p.n; b += (int)gridDim.x) {
        int s = p.sigma_q16[b];
        if (s < 0) continue;
        s = s > 65536 ? 65536 : s;
        const uint32_t* row = (const uint32_t*)p.ws + (int64_t)b * 256 + 4 * lane;
        const uint32_t c[4] = {row[0], row[1], row[2], row[3]};
        uint32_t incl = c[0] + c[1] + c[2] + c[3];
        const uint32_t own = incl;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {                   // inclusive scan over the lanes
            const uint32_t o = __shfl(incl, (lane - d) & 63);
            if (lane >= d) incl += o;
        }
        int ab = select_rank(c, incl - own, (N - 1) / 2, 4 * lane) + select_rank(c, incl - own, N / 2, 4 * lane);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ab += __shfl_xor(ab, m);
        if (lane == 0) {
            const int m2 = ab;                               // 0 .. 510: both products below fit in int32
            const int low = (m2 * (65536 - s)) >> 17, high = (m2 * (65536 + s)) >> 17;
            p.thr[2 * b] = low < 0 ? 0 : low;
            p.thr[2 * b + 1] = high > 255 ? 255 : high;
            if (p.median2) p.median2[b] = (uint32_t)m2;
        }
    }
}

}  // namespace

extern "C" size_t i2i_canny_auto_ws_bytes(int n) { return n < 1 ? 0 : (size_t)n * 256 * sizeof(uint32_t); }

extern "C" int i2i_canny_auto_thr(const i2i_canny_auto_thr_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "canny_auto_thr: null pointer");
    if (p->c < 1 || p->c > 4) return i2i::fail(I2I_ERR_BAD_ARG, "canny_auto_thr: c = %d outside 1..4", p->c);
    if (p->n < 0 || p->h < 0 || p->w < 0) return i2i::fail(I2I_ERR_BAD_ARG, "canny_auto_thr: negative size (n = %d, h = %d, w = %d)", p->n, p->h, p->w);
    if (p->n == 0) return I2I_OK;
    if (p->h == 0 || p->w == 0) return i2i::fail(I2I_ERR_BAD_ARG, "canny_auto_thr: empty images (h = %d, w = %d) have no median", p->h, p->w);
    const int64_t N = (int64_t)p->h * p->w * p->c;           // (h * w < 2^62, c <= 4: no overflow)
    if (N > 0x7fffffff) return i2i::fail(I2I_ERR_BAD_ARG, "canny_auto_thr: more than 2^31 - 1 bytes per image (the bins are 32-bit counts)");
    if (!p->src || !p->sigma_q16 || !p->thr || !p->ws) return i2i::fail(I2I_ERR_BAD_ARG, "canny_auto_thr: null pointer (src, sigma_q16, thr, ws)");
    if (((uintptr_t)p->sigma_q16 | (uintptr_t)p->thr | (uintptr_t)p->median2) & 3)
        return i2i::fail(I2I_ERR_BAD_ARG, "canny_auto_thr: sigma_q16, thr and median2 must be 4-byte aligned");
    if ((uintptr_t)p->ws & 15) return i2i::fail(I2I_ERR_BAD_ARG, "canny_auto_thr: the workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t words = (int64_t)p->n * 256;
    const int64_t cb = (words + 255) / 256;
    hipLaunchKernelGGL(canny_hist_clear_kernel, dim3((unsigned)(cb < HIST_MAX_GRID ? cb : HIST_MAX_GRID)), dim3(256), 0, s, (uint32_t*)p->ws, words);
    // slices per image: what the chunk loop of one image can use, then the cap on the whole grid
    const int64_t want = (N / 16 + HIST_CHUNKS_PER_WG - 1) / HIST_CHUNKS_PER_WG;
    const unsigned gy = (unsigned)(p->n < HIST_MAX_GRID ? p->n : HIST_MAX_GRID);
    const int64_t cap = HIST_MAX_GRID / gy;
    const unsigned gx = (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
    hipLaunchKernelGGL(canny_hist_kernel, dim3(gx, gy), dim3(HIST_THREADS), HIST_WAVES * 256 * sizeof(uint32_t), s, *p);
    hipLaunchKernelGGL(canny_select_kernel, dim3(gy), dim3(64), 0, s, *p);
    return i2i::check_launch("canny_auto_thr");
}

// ------------------------------------------------------------------------------------------------------------------------
// Tiled forward at native resolution (i2i_tile_positions, i2i_tile_cut, i2i_tile_blend_u8; the contract is the comment of i2i_tile_request
// in include/i2i_turbo.h): requests larger than the model size are cut into overlapping tiles, and the tile outputs are blended back with
// an integer feather.  Both kernels follow resize_ragged_u8_kernel: grid y = request, grid x = a capacity hint, everything that differs
// between requests is read from a device descriptor, and every workgroup judges its request before it touches a pixel.  Work is dealt
// by ROWS: a wave owns one row of a tile (cut) or of the image (blend) at a time, so everything that depends on the row -- tile slot,
// plane, source row, the covering ky set and its weights -- is wave-uniform, and the lanes run along the row (coalesced).
namespace {

constexpr int TILE_MAX_X = 1024;                             // workgroups per request at most
constexpr int TILE_WAVES = 4;                                // waves of a workgroup of 256

// 0 = empty slot, 1 = run, -1 = rejected; as ragged_verdict (all 256 threads, i2i_smem holds one int).  `px`: bytes per pixel times planes
// is the request's size; `ordered`: the blend's extra condition on the positions of an axis.
__device__ int tile_verdict(const i2i_tile_request& d, const int32_t* __restrict__ pos, int64_t pos_len, int64_t arena_bytes, int planes, int px,
                            int tw, int th, int tiles_capacity, bool ordered) {
    if (d.h == 0 || d.w == 0) return 0;
    bool ok = d.h > 0 && d.w > 0 && d.nx >= 1 && d.ny >= 1 && d.off >= 0 && (d.off & 3) == 0 && d.off <= arena_bytes && d.xs_off >= 0 && d.ys_off >= 0 &&
              d.xs_off <= pos_len && d.ys_off <= pos_len && d.tile0 >= 0 && d.tile0 <= tiles_capacity && tw <= d.w && th <= d.h;
    if (ok) {                                                // sizes as quotients: no product can overflow
        const int64_t pxs = (int64_t)d.h * d.w;              // < 2^62
        ok = pxs <= (arena_bytes - d.off) / px / planes && d.nx <= pos_len - d.xs_off && d.ny <= pos_len - d.ys_off &&
             d.nx <= (tiles_capacity - d.tile0) / d.ny;
    }
    int* verdict = (int*)i2i_smem;
    if (threadIdx.x == 0) *verdict = ok ? 1 : 0;
    __syncthreads();
    if (ok) {
        bool pos_ok = true;
        for (int axis = 0; axis < 2; ++axis) {
            const int32_t* __restrict__ q = pos + (axis ? d.ys_off : d.xs_off);
            const int cnt = axis ? d.ny : d.nx, ext = axis ? d.h : d.w, t = axis ? th : tw;
            for (int k = (int)threadIdx.x; k < cnt; k += 256) {
                const int x = q[k];
                pos_ok = pos_ok && x >= 0 && x <= ext - t;
                if (ordered) {
                    if (k + 1 < cnt) pos_ok = pos_ok && q[k + 1] > x;
                    if (k + 3 < cnt) pos_ok = pos_ok && q[k + 3] >= x && q[k + 3] - x >= t;
                }
            }
        }
        if (!pos_ok) *verdict = 0;                           // (every writer stores the same 0)
    }
    __syncthreads();
    const int v = *verdict;
    __syncthreads();                                         // the word is reused for the workgroup's next request
    return v ? 1 : -1;
}

// VEC = 4: tile rows of whole dwords (tw * px_bytes % 4 == 0; every tile row of dst then starts on a dword); VEC = 1: bytes
template <int VEC>
__device__ __forceinline__ void tile_cut_request(const i2i_tile_cut_params& p, const i2i_tile_request& d) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int px = p.px_bytes;
    const int64_t rowb = (int64_t)p.tw * px;                 // bytes of a tile row
    const int units = (int)(rowb / VEC);
    const int64_t rows = (int64_t)d.nx * d.ny * p.planes * p.th;
    const int32_t* __restrict__ xs = p.pos + d.xs_off;
    const int32_t* __restrict__ ys = p.pos + d.ys_off;
    const uint8_t* __restrict__ base = (const uint8_t*)p.src;                 // the ARENA: `a` below is an arena offset
    uint8_t* __restrict__ dst = (uint8_t*)p.dst;
    for (int64_t row = (int64_t)blockIdx.x * TILE_WAVES + wave; row < rows; row += (int64_t)gridDim.x * TILE_WAVES) {
        const int r = (int)(row % p.th);
        const int64_t tp = row / p.th;
        const int pl = (int)(tp % p.planes), t = (int)(tp / p.planes);
        const int ky = t / d.nx, kx = t - ky * d.nx;
        const int64_t a0 = d.off + (((int64_t)pl * d.h + ys[ky] + r) * d.w + xs[kx]) * px;
        uint8_t* __restrict__ o = dst + ((((int64_t)(d.tile0 + t) * p.planes + pl) * p.th + r) * rowb);
        for (int u = lane; u < units; u += 64) {
            if constexpr (VEC == 4) {
                const int64_t a = a0 + 4 * (int64_t)u;
                const int sh = 8 * (int)(a & 3);
                uint32_t v;
                if (sh == 0) {
                    v = *(const uint32_t*)(base + a);
                } else if ((a & ~(int64_t)3) + 8 <= p.arena_bytes) {
                    const uint32_t* q = (const uint32_t*)(base + (a & ~(int64_t)3));
                    v = (q[0] >> sh) | (q[1] << (32 - sh));
                } else {                                     // the arena's last dword: the request's own bytes only
                    v = (uint32_t)base[a] | ((uint32_t)base[a + 1] << 8) | ((uint32_t)base[a + 2] << 16) | ((uint32_t)base[a + 3] << 24);
                }
                *(uint32_t*)(o + 4 * (int64_t)u) = v;
            } else {
                o[u] = base[a0 + u];
            }
        }
    }
}

__global__ __launch_bounds__(256) void tile_cut_kernel(const i2i_tile_cut_params p) {
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_tile_request d = p.reqs[b];
        const int v = tile_verdict(d, p.pos, p.pos_len, p.arena_bytes, p.planes, p.px_bytes, p.tw, p.th, p.tiles_capacity, false);
        if (v < 0 && p.bad_mask && blockIdx.x == 0 && threadIdx.x == 0) agent_or_u32(p.bad_mask, 1u << (b & 31));
        if (v <= 0) continue;
        if (((int64_t)p.tw * p.px_bytes) % 4 == 0) tile_cut_request<4>(p, d);
        else tile_cut_request<1>(p, d);
    }
}

__device__ __forceinline__ int feather(int i, int t, int ramp) {
    const int a = i + 1, b = t - i;
    const int m = a < b ? a : b;
    return m < ramp ? m : ramp;
}

// VEC = 4: image rows of whole dwords (w * c % 4 == 0; the request's base is 4-byte aligned); VEC = 1: bytes.  Returns whether this thread
// met a byte that no tile covers.
template <int VEC>
__device__ __forceinline__ bool tile_blend_request(const i2i_tile_blend_u8_params& p, const i2i_tile_request& d) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int c = p.c;
    const int64_t rowb = (int64_t)d.w * c;
    const int units = (int)(rowb / VEC);
    const int64_t trow = (int64_t)p.tw * c;                  // bytes of a tile row
    const int32_t* __restrict__ xs = p.pos + d.xs_off;
    const int32_t* __restrict__ ys = p.pos + d.ys_off;
    const uint8_t* __restrict__ tiles = (const uint8_t*)p.tiles;
    uint8_t* __restrict__ dst = (uint8_t*)p.dst + d.off;
    bool hole = false;
    for (int y = (int)blockIdx.x * TILE_WAVES + wave; y < d.h; y += (int)gridDim.x * TILE_WAVES) {
        // the tile rows over y (wave-uniform; at most 3, the positions increase): first tile of the tile row, row inside the tile, weight
        int nky = 0, wy[3];
        int64_t rbase[3];
        for (int ky = 0; ky < d.ny && nky < 3; ++ky) {
            const int y0 = ys[ky];
            if (y0 > y) break;
            if (y - y0 < p.th) {
                wy[nky] = feather(y - y0, p.th, p.ramp);
                rbase[nky] = (((int64_t)d.tile0 + (int64_t)ky * d.nx) * p.th + (y - y0)) * trow;
                ++nky;
            }
        }
        uint8_t* __restrict__ o = dst + (int64_t)y * rowb;
        for (int u = lane; u < units; u += 64) {
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < VEC; ++b) {
                const int j = u * VEC + b, x = j / c, ch = j - x * c;
                uint32_t num = 0, den = 0;
                for (int kx = 0; kx < d.nx; ++kx) {
                    const int x0 = xs[kx];
                    if (x0 > x) break;
                    if (x - x0 >= p.tw) continue;
                    const uint32_t wx = (uint32_t)feather(x - x0, p.tw, p.ramp);
                    const int64_t within = (int64_t)kx * p.th * trow + (int64_t)(x - x0) * c + ch;
                    for (int k = 0; k < nky; ++k) {
                        const uint32_t w = wx * (uint32_t)wy[k];
                        num += w * tiles[rbase[k] + within];
                        den += w;
                    }
                }
                uint32_t out = 0;
                if (den) out = (2 * num + den) / (2 * den);
                else hole = true;
                word |= out << (8 * b);
            }
            if constexpr (VEC == 4) *(uint32_t*)(o + 4 * (int64_t)u) = word;
            else o[u] = (uint8_t)word;
        }
    }
    return hole;
}

__global__ __launch_bounds__(256) void tile_blend_u8_kernel(const i2i_tile_blend_u8_params p) {
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_tile_request d = p.reqs[b];
        const int v = tile_verdict(d, p.pos, p.pos_len, p.arena_bytes, 1, p.c, p.tw, p.th, p.tiles_capacity, true);
        if (v < 0 && p.bad_mask && blockIdx.x == 0 && threadIdx.x == 0) agent_or_u32(p.bad_mask, 1u << (b & 31));
        if (v <= 0) continue;
        const bool hole = (((int64_t)d.w * p.c) % 4 == 0) ? tile_blend_request<4>(p, d) : tile_blend_request<1>(p, d);
        if (hole && p.bad_mask) agent_or_u32(p.bad_mask, 1u << (b & 31));
    }
}

// what both entries check alike; `what` names the entry
int tile_args(const char* what, int n, int planes, int px, int tw, int th, int tiles_capacity, int64_t grid_units, int64_t arena_bytes, int64_t pos_len,
              const void* arena, const void* tiles, const void* reqs, const void* pos, const void* bad_mask) {
    if (n < 0) return i2i::fail(I2I_ERR_BAD_ARG, "%s: n = %d < 0", what, n);
    if (planes < 1) return i2i::fail(I2I_ERR_BAD_ARG, "%s: planes = %d < 1", what, planes);
    if (px < 1 || px > 4) return i2i::fail(I2I_ERR_BAD_ARG, "%s: %d bytes per pixel outside 1..4", what, px);
    if (tw < 1 || th < 1) return i2i::fail(I2I_ERR_BAD_ARG, "%s: tile extent (tw = %d, th = %d) must be positive", what, tw, th);
    if (tiles_capacity < 0) return i2i::fail(I2I_ERR_BAD_ARG, "%s: tiles_capacity = %d < 0", what, tiles_capacity);
    if (grid_units < 1) return i2i::fail(I2I_ERR_BAD_ARG, "%s: grid_units must be >= 1", what);
    if (arena_bytes < 0 || pos_len < 0) return i2i::fail(I2I_ERR_BAD_ARG, "%s: negative arena_bytes / pos_len", what);
    if (n == 0) return I2I_OK;
    if (!arena || !tiles || !reqs || !pos) return i2i::fail(I2I_ERR_BAD_ARG, "%s: null pointer (arena, tiles, reqs, pos)", what);
    if (((uintptr_t)arena | (uintptr_t)tiles | (uintptr_t)pos | (uintptr_t)bad_mask) & 3)
        return i2i::fail(I2I_ERR_BAD_ARG, "%s: the arena, the tile batch, pos and bad_mask must be 4-byte aligned", what);
    if ((uintptr_t)reqs & 7) return i2i::fail(I2I_ERR_BAD_ARG, "%s: reqs must be 8-byte aligned", what);
    return I2I_OK;
}

dim3 tile_grid(int n, int64_t grid_units) {
    const int64_t bx = (grid_units + 1023) / 1024;
    return dim3((unsigned)(bx < TILE_MAX_X ? bx : TILE_MAX_X), (unsigned)(n < 65535 ? n : 65535));
}

}  // namespace

extern "C" int i2i_tile_positions(int L, int t, int ov, int32_t* out, int capacity) {
    if (t < 8 || t % 8 != 0) return i2i::fail(I2I_ERR_BAD_ARG, "tile_positions: tile extent %d is not a positive multiple of 8", t);
    if (ov < 0 || ov % 8 != 0 || ov > t / 2) return i2i::fail(I2I_ERR_BAD_ARG, "tile_positions: overlap %d (a multiple of 8 in 0 .. %d)", ov, t / 2);
    if (L < t) return i2i::fail(I2I_ERR_BAD_ARG, "tile_positions: length %d is smaller than the tile extent %d", L, t);
    const int s = t - ov;
    const int64_t n = 1 + ((int64_t)L - t + s - 1) / s;
    if (n > 0x7fffffff) return i2i::fail(I2I_ERR_BAD_ARG, "tile_positions: more than 2^31 - 1 tiles");
    if (!out) return (int)n;
    if (capacity < n) return i2i::fail(I2I_ERR_BAD_ARG, "tile_positions: capacity %d < %d tiles", capacity, (int)n);
    for (int64_t k = 0; k < n; ++k) out[k] = (int32_t)(k * s < (int64_t)L - t ? k * s : (int64_t)L - t);
    return (int)n;
}

extern "C" int i2i_tile_cut(const i2i_tile_cut_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "tile_cut: null pointer");
    const int rc = tile_args("tile_cut", p->n, p->planes, p->px_bytes, p->tw, p->th, p->tiles_capacity, p->grid_units, p->arena_bytes, p->pos_len,
                             p->src, p->dst, p->reqs, p->pos, p->bad_mask);
    if (rc != I2I_OK || p->n == 0) return rc;
    hipLaunchKernelGGL(tile_cut_kernel, tile_grid(p->n, p->grid_units), dim3(256), 16, (hipStream_t)stream, *p);
    return i2i::check_launch("tile_cut");
}

extern "C" int i2i_tile_blend_u8(const i2i_tile_blend_u8_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "tile_blend_u8: null pointer");
    if (p->ramp < 1 || p->ramp > 256) return i2i::fail(I2I_ERR_BAD_ARG, "tile_blend_u8: ramp = %d outside 1..256", p->ramp);
    const int rc = tile_args("tile_blend_u8", p->n, 1, p->c, p->tw, p->th, p->tiles_capacity, p->grid_units, p->arena_bytes, p->pos_len,
                             p->dst, p->tiles, p->reqs, p->pos, p->bad_mask);
    if (rc != I2I_OK || p->n == 0) return rc;
    hipLaunchKernelGGL(tile_blend_u8_kernel, tile_grid(p->n, p->grid_units), dim3(256), 16, (hipStream_t)stream, *p);
    return i2i::check_launch("tile_blend_u8");
}

// ------------------------------------------------------------------------------------------------------------------------
// Baseline JPEG encoding, the last uint8 boundary op (i2i_jpeg_encode_u8, i2i_jpeg_workspace_bytes, i2i_jpeg_header)
#include "jpeg.inc"
// PNG encoding beside it (i2i_png_encode_u8, i2i_png_workspace_bytes, i2i_png_bound)
#include "png.inc"

// Boundary and latent-space elementwise kernels for gfx950 (all HBM-bound, one thread per pixel):
//   NCHW <-> NHWC conversion at the .forward() boundary (torch callers hand NCHW; the kernels run NHWC),
//   DiagonalGaussianDistribution.sample()*scaling_factor + the stochastic mix (src/pix2pix_turbo.py:198,210),
//   DDPMScheduler.step + /scaling_factor + post_quant_conv (src/pix2pix_turbo.py:200-203),
//   the seeded Gaussian noise of the callers (torch.manual_seed + torch.randn, src/inference_paired.py:58-60): Philox4x32-10 + Box-Muller,
//   the numerical health scan of an activation tensor (NaN / Inf / near-saturation counts into a device record; no reference counterpart),
//   the image-major replication of the encoder's outputs for ForwardPlan(variations = V) (i2i_repeat: one read, V stores per vector).
#include <string.h>

#include <type_traits>

#include "i2i_dev.h"
#include "launch.h"

namespace {

template <typename T, typename S>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const i2i_nchw_to_nhwc_params p) {
    const int64_t hw = (int64_t)p.h * p.w, total = (int64_t)p.n * hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t img = i / hw, px = i - img * hw;
        const S* x = (const S*)p.x + img * p.c * hw + px;
        T* y = (T*)p.y + i * p.cpad;
        for (int c = 0; c < p.cpad; ++c) y[c] = (c < p.c) ? from_f32<T>((float)x[(int64_t)c * hw] * p.mul + p.add) : from_f32<T>(0.f);
    }
}

template <typename T, typename D>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const i2i_nhwc_to_nchw_params p) {
    const int64_t hw = (int64_t)p.h * p.w, total = (int64_t)p.n * hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t img = i / hw, px = i - img * hw;
        const T* x = (const T*)p.x + i * p.ldx;
        D* y = (D*)p.y + img * p.c * hw + px;
        for (int c = 0; c < p.c; ++c) {
            float v = to_f32<T>(x[c]);
            if (p.clamp) v = fminf(fmaxf(v, -1.f), 1.f);
            y[(int64_t)c * hw] = (D)v;
        }
    }
}

// uint8 HWC image batch -> NHWC `T` (channels padded with zeros): F.to_tensor (+ Normalize) of the callers folded in
template <typename T>
__global__ __launch_bounds__(256) void u8hwc_to_nhwc_kernel(const i2i_nchw_to_nhwc_params p) {
    const int64_t total = (int64_t)p.n * p.h * p.w;
    const float k = p.mul * (1.0f / 255.0f);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const uint8_t* x = (const uint8_t*)p.x + i * p.c;
        T* y = (T*)p.y + i * p.cpad;
        for (int c = 0; c < p.cpad; ++c) {
            float v = 0.f;
            if (c < p.c) v = p.binarize_below > 0 ? ((int)x[c] < p.binarize_below ? p.mul + p.add : p.add) : (float)x[c] * k + p.add;
            y[c] = from_f32<T>(v);
        }
    }
}
// NHWC `T` -> uint8 HWC: clamp, x*mul+add, ToPILImage's mul(255).byte() (truncation)
template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_u8hwc_kernel(const i2i_nhwc_to_nchw_params p) {
    const int64_t total = (int64_t)p.n * p.h * p.w;
    const float mul = (p.mul == 0.f && p.add == 0.f) ? 1.f : p.mul;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const T* x = (const T*)p.x + i * p.ldx;
        uint8_t* y = (uint8_t*)p.y + i * p.c;
        for (int c = 0; c < p.c; ++c) {
            float v = to_f32<T>(x[c]);
            if (p.clamp) v = fminf(fmaxf(v, -1.f), 1.f);
            v = fminf(fmaxf(v * mul + p.add, 0.f), 1.f);
            y[c] = (uint8_t)(v * 255.0f);
        }
    }
}

// CLIP text embeddings: one 8-element unit per thread, y = tok[ids[row]] + pos[row % T] (sum in fp32)
template <typename T>
__global__ __launch_bounds__(256) void embed_kernel(const i2i_embed_params p) {
    typedef typename Elem<T>::chunk_t chunk_t;
    constexpr int EPC = Elem<T>::EPC;
    const int upr = p.c / EPC;
    const int64_t total = (int64_t)p.rows * upr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i / upr), u = (int)(i - (int64_t)row * upr);
        int64_t id = p.ids[row];
        id = id < 0 ? 0 : (id >= p.vocab ? p.vocab - 1 : id);
        const chunk_t a = *(const chunk_t*)((const T*)p.tok + id * p.c + u * EPC);
        const chunk_t b = *(const chunk_t*)((const T*)p.pos + (int64_t)(row % p.T) * p.c + u * EPC);
        chunk_t o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) o[e] = from_f32<T>(to_f32<T>(a[e]) + to_f32<T>(b[e]));
        *(chunk_t*)((T*)p.y + (int64_t)row * p.c + u * EPC) = o;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void posterior_kernel(const i2i_posterior_params p) {
    const int64_t total = (int64_t)p.n * p.hw;
    const float r = p.r_dev ? p.r_dev[0] : p.r;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t img = i / p.hw, px = i - img * p.hw;
        const T* m = (const T*)p.moments + i * p.ldm;
        const float* mf = (const float*)p.moments + i * p.ldm;
        T* u = (T*)p.u + i * p.ldu;
        for (int c = 0; c < p.ldu; ++c) {
            float v = 0.f;
            if (c < p.lat) {
                const float mean = p.moments_f32 ? mf[c] : to_f32<T>(m[c]);
                const float logvar = fminf(fmaxf(p.moments_f32 ? mf[p.lat + c] : to_f32<T>(m[p.lat + c]), -30.f), 20.f);
                const float e = p.eps[(img * p.lat + c) * p.hw + px];
                v = (mean + __expf(0.5f * logvar) * e) * p.sf;
                if (p.noise) {
                    const int64_t nimg = (p.noise_n == 1) ? 0 : img;
                    v = v * r + p.noise[(nimg * p.lat + c) * p.hw + px] * (1.f - r);
                }
            }
            u[c] = from_f32<T>(v);
            if (p.u_f32 && c < p.lat) p.u_f32[i * p.lat + c] = v;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ddpm_kernel(const i2i_ddpm_params p) {
    const int64_t total = (int64_t)p.n * p.hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const T* u = (const T*)p.u + i * p.ldu;
        const T* e = (const T*)p.e + i * p.lde;
        T* y = (T*)p.y + i * p.ldy;
        float x0[8];
        const float* uf = (const float*)p.u + i * p.ldu;
        const float* ef = (const float*)p.e + i * p.lde;
        for (int c = 0; c < p.lat; ++c) {
            const float uv = p.u_f32 ? uf[c] : to_f32<T>(u[c]);
            const float ev = p.e_f32 ? ef[c] : to_f32<T>(e[c]);
            x0[c] = ((uv - p.sqrt_1m_abar * ev) / p.sqrt_abar) / p.sf;
        }
        for (int o = 0; o < p.ldy; ++o) {
            float v = 0.f;
            if (o < p.lat) {
                v = p.bpq[o];
                for (int c = 0; c < p.lat; ++c) v += p.wpq[o * p.lat + c] * x0[c];
            }
            y[o] = from_f32<T>(v);
        }
    }
}

// ---- seeded noise (the contract is the comment of i2i_randn_params): one thread per Philox counter = four consecutive elements
__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = umulhi_u32(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = umulhi_u32(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const u32x4 nx = {hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0};
        c = nx;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// words (wa, wb) -> two normal deviates; u1 in (0, 1] and 2*u2 in [0, 2) are exact in fp32, the functions are the precise ones
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, uint32_t& x, uint32_t& y) {
    const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;
    const float t = (float)(wb >> 8) * 0x1p-23f;
    const float rad = sqrtf(-2.0f * logf(u1));
    x = __builtin_bit_cast(uint32_t, rad * cospi_f(t));
    y = __builtin_bit_cast(uint32_t, rad * sinpi_f(t));
}

// dst[0 .. n) from one state: the body of both noise kernels (a counter per thread, grid-stride along x)
template <bool NORMAL>
__device__ __forceinline__ void randn_fill(uint32_t* dst, int64_t n, uint32_t k0, uint32_t k1, uint32_t step, uint32_t stream_id) {
    const bool wide = ((uintptr_t)dst & 15) == 0;          // dst + 4q is then 16-byte aligned for every q
    const int64_t nq = (n + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        const u32x4 ctr = {(uint32_t)q, (uint32_t)((uint64_t)q >> 32), step, stream_id};
        u32x4 w = philox4x32_10(ctr, k0, k1);
        if (NORMAL) {
            uint32_t a, b, c, d;
            box_muller(w[0], w[1], a, b);
            box_muller(w[2], w[3], c, d);
            const u32x4 g = {a, b, c, d};
            w = g;
        }
        const int64_t i = q << 2;
        if (wide && i + 4 <= n) {
            *(u32x4*)(dst + i) = w;
        } else {
            for (int e = 0; e < 4; ++e)
                if (i + e < n) dst[i + e] = w[e];
        }
    }
}

template <bool NORMAL>
__global__ __launch_bounds__(256) void randn_kernel(const i2i_randn_params p) {
    const uint32_t k0 = p.state ? p.state[0] : (uint32_t)p.seed, k1 = p.state ? p.state[1] : (uint32_t)(p.seed >> 32);
    const uint32_t step = p.state ? p.state[2] : p.step;
    randn_fill<NORMAL>((uint32_t*)p.dst, p.n, k0, k1, step, p.stream_id);
}

__global__ __launch_bounds__(64) void randn_advance_kernel(uint32_t* state) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[2] += 1u;
}

// per-image states (the contract is the comment of i2i_randn_batch_params): blockIdx.y walks the images, blockIdx.x the counters of one
// image -- no 64-bit division.  The 16-byte store is decided per image BASE (dst + b * per_image): with per_image % 4 != 0 or a dst
// that is only 4-byte aligned some bases are misaligned and those images take the element stores; the tail lanes are dropped per image.
constexpr int RANDN_BATCH_MAX_BLOCKS = 1024;               // workgroups of a fill over all images (4 per CU), as i2i_randn's cap

template <bool NORMAL>
__global__ __launch_bounds__(256) void randn_batch_kernel(const i2i_randn_batch_params p) {
    for (int b = (int)blockIdx.y; b < p.batch; b += (int)gridDim.y) {
        const uint32_t* st = p.states + 4 * (int64_t)b;
        randn_fill<NORMAL>((uint32_t*)p.dst + (int64_t)b * p.per_image, p.per_image, st[0], st[1], st[2], p.stream_id);
    }
}

__global__ __launch_bounds__(256) void randn_batch_advance_kernel(uint32_t* states, int batch) {
    for (int b = (int)(blockIdx.x * 256 + threadIdx.x); b < batch; b += (int)(gridDim.x * 256)) states[4 * (int64_t)b + 2] += 1u;
}

// ---- numerical health scan (the contract is the comment of i2i_scan_params).  Everything is done on bit patterns in the element's OWN
// format: a = pattern without the sign orders like |x|, a >= INF is Inf / NaN, and the host translates `limit` into the largest pattern
// `thr` whose value is <= limit (capped at the largest finite one), so "finite and |x| > limit" is a > thr and one unsigned max over a
// 16-byte chunk decides whether anything in it needs a second look: a healthy chunk costs an AND and a MAX per element.
constexpr int SCAN_THREADS = 256;       // 4 waves
constexpr int SCAN_UNROLL = 4;          // independent 16-byte loads per lane and iteration: a workgroup strides over 1024 chunks
constexpr int SCAN_MAX_GRID = 1024;     // 4 workgroups per CU; with the unroll 16 MiB of loads in flight chip-wide

template <typename T> struct ScanFmt;
template <> struct ScanFmt<float> { static constexpr uint32_t ABS = 0x7FFFFFFFu, INF = 0x7F800000u, SIGN = 0x80000000u; };
template <> struct ScanFmt<__bf16> { static constexpr uint32_t ABS = 0x7FFFu, INF = 0x7F80u, SIGN = 0x8000u; };
template <> struct ScanFmt<_Float16> { static constexpr uint32_t ABS = 0x7FFFu, INF = 0x7C00u, SIGN = 0x8000u; };

// fp32 pattern of a finite non-negative pattern of the element format (exact: integer arithmetic + one exact int -> float conversion)
template <typename T> __host__ __device__ inline uint32_t scan_widen(uint32_t a);
template <> __host__ __device__ inline uint32_t scan_widen<float>(uint32_t a) { return a; }
template <> __host__ __device__ inline uint32_t scan_widen<__bf16>(uint32_t a) { return a << 16; }
template <> __host__ __device__ inline uint32_t scan_widen<_Float16>(uint32_t a) {
    const uint32_t e = a >> 10, m = a & 0x3FFu;
    if (e) return ((e + 112u) << 23) | (m << 13);
    return __builtin_bit_cast(uint32_t, (float)m * 0x1p-24f);      // subnormal fp16 = m * 2^-24: a normal fp32 number (or 0)
}

struct ScanAcc { uint32_t nan, pinf, ninf, over, amax; };
// A row = `head` elements in front of the first 16-byte boundary, `nb` aligned 16-byte chunks, `tail` elements behind them -- the same split
// for every row (the host sees to that: a contiguous view arrives as ONE row, rows that do not all start on a 16-byte boundary as all tail).
struct ScanArgs {
    const char* x; int64_t rows, ld;
    int64_t head, nb, tail;
    uint64_t n_elems; uint32_t thr; uint64_t* rec;
};

template <typename T> __device__ __forceinline__ void scan_elem(uint32_t w, uint32_t thr, ScanAcc& c) {
    typedef ScanFmt<T> F;
    const uint32_t a = w & F::ABS;
    if (a >= F::INF) {
        if (a > F::INF) ++c.nan;
        else if (w & F::SIGN) ++c.ninf;
        else ++c.pinf;
    } else {
        c.amax = a > c.amax ? a : c.amax;
        c.over += a > thr ? 1u : 0u;
    }
}

template <typename T> __device__ __forceinline__ void scan_chunk(const u32x4 v, uint32_t thr, ScanAcc& c) {
    typedef ScanFmt<T> F;
    uint32_t mx = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (sizeof(T) == 4) {
            const uint32_t a = v[j] & F::ABS;
            mx = a > mx ? a : mx;
        } else {
            const uint32_t lo = v[j] & F::ABS, hi = (v[j] >> 16) & F::ABS;
            mx = lo > mx ? lo : mx;
            mx = hi > mx ? hi : mx;
        }
    }
    if (mx <= thr) {             // thr < INF: nothing here is Inf, NaN or over the limit
        c.amax = mx > c.amax ? mx : c.amax;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (sizeof(T) == 4) {
            scan_elem<T>(v[j], thr, c);
        } else {
            scan_elem<T>(v[j] & 0xFFFFu, thr, c);
            scan_elem<T>(v[j] >> 16, thr, c);
        }
    }
}

// hipcc otherwise waits for the first load before it issues the other three (it hoists the first chunk's arithmetic)
#ifdef I2I_EMU
__device__ __forceinline__ void scan_fence(u32x4 (&)[SCAN_UNROLL]) {}
#else
__device__ __forceinline__ void scan_fence(u32x4 (&v)[SCAN_UNROLL]) { asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])); }
static_assert(SCAN_UNROLL == 4, "scan_fence names four chunks");
#endif
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m);
    return v;
}

// Two grid-stride loops: the aligned chunks (SCAN_UNROLL independent 16-byte loads per lane, issued together), then the head / tail
// elements one per lane.  Nothing outside [0, cols) of a row is read.
// (ONE_ROW: the contiguous view, which is every tensor of a planned forward but one -- no 64-bit division per chunk)
template <typename T, bool ONE_ROW>
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(const ScanArgs a) {
    constexpr int ESZ = (int)sizeof(T), EPC = 16 / ESZ;
    typedef typename std::conditional<ESZ == 4, uint32_t, uint16_t>::type word_t;
    ScanAcc c = {0u, 0u, 0u, 0u, 0u};
    const int64_t step = (int64_t)gridDim.x * (SCAN_THREADS * SCAN_UNROLL);
    const int64_t items = a.rows * a.nb;
    const char* body = a.x + a.head * ESZ;
    auto chunk_at = [&](int64_t i) -> const u32x4* {
        if (ONE_ROW) return (const u32x4*)body + i;
        const int64_t row = i / a.nb, j = i - row * a.nb;
        return (const u32x4*)(body + row * a.ld * ESZ) + j;
    };
    int64_t i0 = (int64_t)blockIdx.x * (SCAN_THREADS * SCAN_UNROLL) + threadIdx.x;
    for (; i0 + (SCAN_UNROLL - 1) * SCAN_THREADS < items; i0 += step) {
        u32x4 v[SCAN_UNROLL];
#pragma unroll
        for (int u = 0; u < SCAN_UNROLL; ++u) v[u] = *chunk_at(i0 + u * SCAN_THREADS);
        scan_fence(v);      // all loads of the round are issued before the first is consumed
#pragma unroll
        for (int u = 0; u < SCAN_UNROLL; ++u) scan_chunk<T>(v[u], a.thr, c);
    }
    if (i0 < items) {               // the last, partial round of this lane (the rounds of a lane are SCAN_THREADS apart: at most one is cut)
        for (int u = 0; u < SCAN_UNROLL - 1; ++u) {
            const int64_t i = i0 + u * SCAN_THREADS;
            if (i < items) scan_chunk<T>(*chunk_at(i), a.thr, c);
        }
    }
    const int64_t edge = a.head + a.tail, n_edge = a.rows * edge;
    for (int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; i < n_edge; i += (int64_t)gridDim.x * SCAN_THREADS) {
        const int64_t row = ONE_ROW ? 0 : i / edge, e = i - row * edge;
        const int64_t col = e < a.head ? e : e + a.nb * EPC;
        scan_elem<T>(((const word_t*)a.x)[row * a.ld + col], a.thr, c);
    }
    // lanes -> wave (the counts only when some lane of the wave has one) -> workgroup through LDS -> at most one atomic per non-zero field
    uint32_t amax = c.amax;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = __shfl_xor(amax, m);
        amax = o > amax ? o : amax;
    }
    uint64_t cnt[4] = {c.nan, c.pinf, c.ninf, c.over};
    if (wave_any((c.nan | c.pinf | c.ninf | c.over) != 0u)) {
#pragma unroll
        for (int f = 0; f < 4; ++f) cnt[f] = wave_sum_u64(cnt[f]);
    }
    uint64_t* red = (uint64_t*)i2i_smem;          // [waves][5]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int f = 0; f < 4; ++f) red[wave * 5 + f] = cnt[f];
        red[wave * 5 + 4] = amax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tot[4] = {0, 0, 0, 0}, mx = 0;
        for (int w = 0; w < SCAN_THREADS / 64; ++w) {
            for (int f = 0; f < 4; ++f) tot[f] += red[w * 5 + f];
            mx = red[w * 5 + 4] > mx ? red[w * 5 + 4] : mx;
        }
        for (int f = 0; f < 4; ++f)
            if (tot[f]) agent_add_u64(a.rec + 1 + f, tot[f]);
        if (mx) agent_max_u64(a.rec + 5, (uint64_t)scan_widen<T>((uint32_t)mx));
        if (blockIdx.x == 0) {                    // exactly one lane of the launch
            agent_add_u64(a.rec + 0, 1);
            if (a.n_elems) agent_add_u64(a.rec + 6, a.n_elems);
        }
    }
}

// largest finite pattern of T's format whose value is <= limit (limit > 0 or +Inf): the patterns order like the values
template <typename T> uint32_t scan_threshold(float limit) {
    const uint32_t lb = __builtin_bit_cast(uint32_t, limit);
    uint32_t lo = 0, hi = ScanFmt<T>::INF - 1;                 // invariant: widen(lo) <= limit
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (scan_widen<T>(mid) <= lb) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename T> int scan_launch(const i2i_scan_params& p, hipStream_t s) {
    constexpr int64_t EPC = 16 / (int64_t)sizeof(T);
    if ((uintptr_t)p.x % sizeof(T)) return i2i::fail(I2I_ERR_BAD_ARG, "scan: x is not aligned to its element type");
    ScanArgs a;
    a.x = (const char*)p.x;
    a.n_elems = (uint64_t)p.rows * (uint64_t)p.cols;
    a.thr = scan_threshold<T>(p.limit);
    a.rec = p.rec;
    int64_t cols = p.cols;
    a.rows = p.rows, a.ld = p.ld;
    if (p.ld == p.cols || p.rows <= 1) cols = (int64_t)a.n_elems, a.rows = 1, a.ld = cols;       // contiguous: one long row
    const int64_t mis = (int64_t)(((uintptr_t)p.x & 15) / sizeof(T));                           // elements past a 16-byte boundary
    if (a.rows == 1) {
        a.head = mis ? (EPC - mis < cols ? EPC - mis : cols) : 0;
        a.nb = (cols - a.head) / EPC, a.tail = cols - a.head - a.nb * EPC;
    } else if (mis == 0 && a.ld % EPC == 0) {
        a.head = 0, a.nb = cols / EPC, a.tail = cols % EPC;                                      // every row starts on a 16-byte boundary
    } else {
        a.head = 0, a.nb = 0, a.tail = cols;                                                     // element loads throughout
    }
    // the grid is sized for the chunk loop (1024 chunks per workgroup and pass), or for the element loop where that one has more to do
    const int64_t per = SCAN_THREADS * SCAN_UNROLL, w1 = (a.rows * a.nb + per - 1) / per, w2 = (a.rows * (a.head + a.tail) + per - 1) / per;
    const int64_t want = w1 > w2 ? w1 : w2;
    const unsigned g = (unsigned)(want < 1 ? 1 : (want > SCAN_MAX_GRID ? SCAN_MAX_GRID : want));
    const size_t smem = (SCAN_THREADS / 64) * 5 * sizeof(uint64_t);
    if (a.rows == 1) hipLaunchKernelGGL((scan_kernel<T, true>), dim3(g), dim3(SCAN_THREADS), smem, s, a);
    else hipLaunchKernelGGL((scan_kernel<T, false>), dim3(g), dim3(SCAN_THREADS), smem, s, a);
    return i2i::check_launch("scan");
}

// ---- the scan over the images of a batch, one record per image (the contract is the comment of i2i_scan_batch_params).  The grid is
// (slices of an image, images); a workgroup works on ONE image at a time: it loops over the images of its y index, and per image over the
// chunks / edge elements of its x slice, with the classification (scan_chunk / scan_elem) and the reduction of scan_kernel.
constexpr int SCAN_BATCH_MAX_GRID = 1024;     // workgroups of one launch at most (as SCAN_MAX_GRID): grid y = min(images, this),
                                              // grid x = min(workgroups one image can use, this / grid y) slices per image

// The views of ALL images (the host sends a contiguous image down as ONE row of rows * cols elements).  The head / body / tail split is
// not here: images start img_stride elements apart, so each has its own misalignment, and the kernel derives the split from the image's
// start address.
struct ScanBatchArgs {
    const char* x; int32_t images; int64_t rows, cols, ld, img_stride;
    uint64_t n_elems; uint32_t thr; uint64_t* rec; int64_t rec_words;       // rec_words: uint64 words between two images' records
};

template <typename T, bool ONE_ROW>
__global__ __launch_bounds__(SCAN_THREADS) void scan_batch_kernel(const ScanBatchArgs a) {
    constexpr int ESZ = (int)sizeof(T), EPC = 16 / ESZ;
    typedef typename std::conditional<ESZ == 4, uint32_t, uint16_t>::type word_t;
    uint64_t* red = (uint64_t*)i2i_smem;          // [waves][5]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = (int)blockIdx.y; b < a.images; b += (int)gridDim.y) {
        const char* x = a.x + (int64_t)b * a.img_stride * ESZ;
        // this image's split, as scan_launch makes it for a single view: elements in front of the first 16-byte boundary, chunks, the rest
        const int64_t mis = (int64_t)(((uintptr_t)x & 15) / ESZ);
        int64_t head, nb, tail;
        if (ONE_ROW) {
            head = mis ? (EPC - mis < a.cols ? EPC - mis : a.cols) : 0;
            nb = (a.cols - head) / EPC, tail = a.cols - head - nb * EPC;
        } else if (mis == 0 && a.ld % EPC == 0) {
            head = 0, nb = a.cols / EPC, tail = a.cols % EPC;                // every row of this image starts on a 16-byte boundary
        } else {
            head = 0, nb = 0, tail = a.cols;                                 // element loads throughout
        }
        ScanAcc c = {0u, 0u, 0u, 0u, 0u};
        const int64_t step = (int64_t)gridDim.x * (SCAN_THREADS * SCAN_UNROLL);
        const int64_t items = a.rows * nb;
        const char* body = x + head * ESZ;
        auto chunk_at = [&](int64_t i) -> const u32x4* {
            if (ONE_ROW) return (const u32x4*)body + i;
            const int64_t row = i / nb, j = i - row * nb;
            return (const u32x4*)(body + row * a.ld * ESZ) + j;
        };
        int64_t i0 = (int64_t)blockIdx.x * (SCAN_THREADS * SCAN_UNROLL) + threadIdx.x;
        for (; i0 + (SCAN_UNROLL - 1) * SCAN_THREADS < items; i0 += step) {
            u32x4 v[SCAN_UNROLL];
#pragma unroll
            for (int u = 0; u < SCAN_UNROLL; ++u) v[u] = *chunk_at(i0 + u * SCAN_THREADS);
            scan_fence(v);
#pragma unroll
            for (int u = 0; u < SCAN_UNROLL; ++u) scan_chunk<T>(v[u], a.thr, c);
        }
        if (i0 < items) {               // the last, partial round of this lane
            for (int u = 0; u < SCAN_UNROLL - 1; ++u) {
                const int64_t i = i0 + u * SCAN_THREADS;
                if (i < items) scan_chunk<T>(*chunk_at(i), a.thr, c);
            }
        }
        const int64_t edge = head + tail, n_edge = a.rows * edge;
        for (int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; i < n_edge; i += (int64_t)gridDim.x * SCAN_THREADS) {
            const int64_t row = ONE_ROW ? 0 : i / edge, e = i - row * edge;
            const int64_t col = e < head ? e : e + nb * EPC;
            scan_elem<T>(((const word_t*)x)[row * a.ld + col], a.thr, c);
        }
        // scan_kernel's reduction, into this image's record
        uint32_t amax = c.amax;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t o = __shfl_xor(amax, m);
            amax = o > amax ? o : amax;
        }
        uint64_t cnt[4] = {c.nan, c.pinf, c.ninf, c.over};
        if (wave_any((c.nan | c.pinf | c.ninf | c.over) != 0u)) {
#pragma unroll
            for (int f = 0; f < 4; ++f) cnt[f] = wave_sum_u64(cnt[f]);
        }
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < 4; ++f) red[wave * 5 + f] = cnt[f];
            red[wave * 5 + 4] = amax;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t* rec = a.rec + (int64_t)b * a.rec_words;
            uint64_t tot[4] = {0, 0, 0, 0}, mx = 0;
            for (int w = 0; w < SCAN_THREADS / 64; ++w) {
                for (int f = 0; f < 4; ++f) tot[f] += red[w * 5 + f];
                mx = red[w * 5 + 4] > mx ? red[w * 5 + 4] : mx;
            }
            for (int f = 0; f < 4; ++f)
                if (tot[f]) agent_add_u64(rec + 1 + f, tot[f]);
            if (mx) agent_max_u64(rec + 5, (uint64_t)scan_widen<T>((uint32_t)mx));
            if (blockIdx.x == 0) {                    // exactly one lane of the launch per image
                agent_add_u64(rec + 0, 1);
                if (a.n_elems) agent_add_u64(rec + 6, a.n_elems);
            }
        }
        __syncthreads();                              // `red` is free again before the next image of this workgroup fills it
    }
}

template <typename T> int scan_batch_launch(const i2i_scan_batch_params& p, hipStream_t s) {
    constexpr int64_t EPC = 16 / (int64_t)sizeof(T);
    if ((uintptr_t)p.x % sizeof(T)) return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: x is not aligned to its element type");
    ScanBatchArgs a;
    a.x = (const char*)p.x, a.images = p.images, a.img_stride = p.img_stride;
    a.n_elems = (uint64_t)p.rows * (uint64_t)p.cols;
    a.thr = scan_threshold<T>(p.limit);
    a.rec = p.rec, a.rec_words = p.rec_stride / 8;
    a.rows = p.rows, a.cols = p.cols, a.ld = p.ld;
    if (p.ld == p.cols || p.rows <= 1) a.cols = (int64_t)a.n_elems, a.rows = 1, a.ld = a.cols;      // contiguous images: one long row each
    // slices per image: what the chunk loop of one image can use (1024 chunks per workgroup and pass), or the element loop where an image
    // has no chunks (upper bounds: the split depends on the image); then the cap on the whole grid
    const int64_t per = SCAN_THREADS * SCAN_UNROLL;
    const bool chunks = a.rows == 1 || a.ld % EPC == 0;
    const int64_t work = chunks ? a.rows * ((a.cols + EPC - 1) / EPC) : a.rows * a.cols, want = (work + per - 1) / per;
    const unsigned gy = (unsigned)(p.images < SCAN_BATCH_MAX_GRID ? p.images : SCAN_BATCH_MAX_GRID);
    const int64_t cap = SCAN_BATCH_MAX_GRID / gy;
    const unsigned gx = (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
    const size_t smem = (SCAN_THREADS / 64) * 5 * sizeof(uint64_t);
    if (a.rows == 1) hipLaunchKernelGGL((scan_batch_kernel<T, true>), dim3(gx, gy), dim3(SCAN_THREADS), smem, s, a);
    else hipLaunchKernelGGL((scan_batch_kernel<T, false>), dim3(gx, gy), dim3(SCAN_THREADS), smem, s, a);
    return i2i::check_launch("scan_batch");
}

// i2i_scan_verdict (the contract is the comment of i2i_scan_verdict_params)
__global__ __launch_bounds__(256) void scan_verdict_clear_kernel(uint64_t* rec, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) rec[i] = 0;
}

__global__ __launch_bounds__(256) void scan_verdict_judge_kernel(const uint64_t* rec, int taps, int images, uint32_t* verdict) {
    for (int b = (int)(blockIdx.x * 256 + threadIdx.x); b < images; b += (int)(gridDim.x * 256)) {      // the lane owns row b
        uint32_t first_bad = 0, first_over = 0;
        for (int t = taps - 1; t >= 0; --t) {
            const uint64_t* r = rec + ((int64_t)t * images + b) * 8;
            if (r[1] | r[2] | r[3]) first_bad = (uint32_t)t + 1u;
            if (r[4]) first_over = (uint32_t)t + 1u;
        }
        uint32_t* v = verdict + 4 * (int64_t)b;
        v[0] = first_bad, v[1] = first_over;
        v[2] += 1u;
        v[3] += first_bad ? 1u : 0u;
    }
}

// ---- i2i_digest (the contract, mixers included, is the comment of i2i_digest_params; tests/digest_ref.py restates it in numpy).  The scan's
// shape: grid (slices of an image, images), a workgroup works on one image at a time, per image the 16-byte chunks of its x slice
// (SCAN_UNROLL loads in flight per lane) and then the head / tail elements one per lane.  Elements are told apart by their size only (the
// value is the bit pattern): fp16 and bf16 share a kernel.
// Cost per element: the Weyl step g = j * DIGEST_W is ONE 64-bit multiply per chunk (or edge element) and a 64-bit add per further element
// of the chunk; what stays per element is three 64-bit multiplies by constants -- hipcc lowers each to one v_mad_u64_u32 and two
// v_mul_lo_u32, nine quarter-rate instructions per element -- plus about twenty shifts, xors and adds: the kernel is bound by the integer
// multiplies, not by the bytes it reads (DESIGN.md has the measured rates).
constexpr int DIGEST_MAX_GRID = 1024;          // workgroups of one launch at most, split as SCAN_BATCH_MAX_GRID is
constexpr uint64_t DIGEST_W = 0x9E3779B97F4A7C15ull, DIGEST_K1 = 0xFF51AFD7ED558CCDull, DIGEST_K2 = 0xC4CEB9FE1A85EC53ull,
                   DIGEST_K3 = 0xD6E8FEB86659FD93ull;

struct DigestArgs {
    const char* x; int32_t images; int64_t rows, cols, ld, img_stride;       // (a contiguous image arrives as ONE row of rows * cols elements)
    uint64_t n_elems, index0; uint64_t* rec;
};
struct DigestAcc { uint64_t s0, s1; };

// g = (index0 + p) * DIGEST_W of the element, v its zero-extended bit pattern
__device__ __forceinline__ void digest_elem(uint64_t g, uint32_t v, DigestAcc& c) {
    uint64_t m = g ^ (uint64_t)v;
    m ^= m >> 33;
    m *= DIGEST_K1;
    m ^= m >> 33;
    m *= DIGEST_K2;
    m ^= m >> 33;
    c.s0 += m;
    const uint64_t t = (m ^ (m >> 31)) * DIGEST_K3;
    c.s1 += t ^ (t >> 32);
}

// the 16 / ESZ elements of one chunk, in memory order; g0 belongs to the first
template <int ESZ> __device__ __forceinline__ void digest_chunk(const u32x4 v, uint64_t g0, DigestAcc& c) {
    constexpr int PER = 4 / ESZ;                 // elements per 32-bit word (little endian: the lowest bits come first)
    constexpr uint32_t MASK = ESZ == 4 ? 0xFFFFFFFFu : ((1u << (8 * (ESZ & 3))) - 1u);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            digest_elem(g0, ESZ == 4 ? v[w] : ((v[w] >> (8 * ESZ * e)) & MASK), c);
            g0 += DIGEST_W;
        }
    }
}

template <int ESZ, bool ONE_ROW>
__global__ __launch_bounds__(SCAN_THREADS) void digest_kernel(const DigestArgs a) {
    constexpr int EPC = 16 / ESZ;
    typedef typename std::conditional<ESZ == 4, uint32_t, typename std::conditional<ESZ == 2, uint16_t, uint8_t>::type>::type word_t;
    uint64_t* red = (uint64_t*)i2i_smem;          // [waves][2]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = (int)blockIdx.y; b < a.images; b += (int)gridDim.y) {
        const char* x = a.x + (int64_t)b * a.img_stride * ESZ;
        // this image's split, from ITS start address (as scan_batch_kernel): elements in front of the first 16-byte boundary, chunks, the rest
        const int64_t mis = (int64_t)(((uintptr_t)x & 15) / ESZ);
        int64_t head, nb, tail;
        if (ONE_ROW) {
            head = mis ? (EPC - mis < a.cols ? EPC - mis : a.cols) : 0;
            nb = (a.cols - head) / EPC, tail = a.cols - head - nb * EPC;
        } else if (mis == 0 && a.ld % EPC == 0) {
            head = 0, nb = a.cols / EPC, tail = a.cols % EPC;                // every row of this image starts on a 16-byte boundary
        } else {
            head = 0, nb = 0, tail = a.cols;                                 // element loads throughout
        }
        DigestAcc c = {0u, 0u};
        const int64_t step = (int64_t)gridDim.x * (SCAN_THREADS * SCAN_UNROLL);
        const int64_t items = a.rows * nb;
        const char* body = x + head * ESZ;
        auto chunk_at = [&](int64_t i) -> const u32x4* {
            if (ONE_ROW) return (const u32x4*)body + i;
            const int64_t row = i / nb, j = i - row * nb;
            return (const u32x4*)(body + row * a.ld * ESZ) + j;
        };
        auto g_of_chunk = [&](int64_t i) -> uint64_t {          // (index0 + element number of the chunk's first element) * W
            if (ONE_ROW) return (a.index0 + (uint64_t)(head + i * EPC)) * DIGEST_W;
            const int64_t row = i / nb, j = i - row * nb;
            return (a.index0 + (uint64_t)(row * a.cols + j * EPC)) * DIGEST_W;
        };
        int64_t i0 = (int64_t)blockIdx.x * (SCAN_THREADS * SCAN_UNROLL) + threadIdx.x;
        for (; i0 + (SCAN_UNROLL - 1) * SCAN_THREADS < items; i0 += step) {
            u32x4 v[SCAN_UNROLL];
#pragma unroll
            for (int u = 0; u < SCAN_UNROLL; ++u) v[u] = *chunk_at(i0 + u * SCAN_THREADS);
            scan_fence(v);      // all loads of the round are issued before the first is consumed
#pragma unroll
            for (int u = 0; u < SCAN_UNROLL; ++u) digest_chunk<ESZ>(v[u], g_of_chunk(i0 + u * SCAN_THREADS), c);
        }
        if (i0 < items) {               // the last, partial round of this lane
            for (int u = 0; u < SCAN_UNROLL - 1; ++u) {
                const int64_t i = i0 + u * SCAN_THREADS;
                if (i < items) digest_chunk<ESZ>(*chunk_at(i), g_of_chunk(i), c);
            }
        }
        const int64_t edge = head + tail, n_edge = a.rows * edge;
        for (int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; i < n_edge; i += (int64_t)gridDim.x * SCAN_THREADS) {
            const int64_t row = ONE_ROW ? 0 : i / edge, e = i - row * edge;
            const int64_t col = e < head ? e : e + nb * EPC;
            digest_elem((a.index0 + (uint64_t)(row * a.cols + col)) * DIGEST_W, (uint32_t)((const word_t*)x)[row * a.ld + col], c);
        }
        // lanes -> wave -> workgroup through LDS -> one add per sum, workgroup and image
        const uint64_t w0 = wave_sum_u64(c.s0), w1 = wave_sum_u64(c.s1);
        if (lane == 0) red[wave * 2 + 0] = w0, red[wave * 2 + 1] = w1;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t* rec = a.rec + (int64_t)b * 4;
            uint64_t t0 = 0, t1 = 0;
            for (int w = 0; w < SCAN_THREADS / 64; ++w) t0 += red[w * 2 + 0], t1 += red[w * 2 + 1];
            agent_add_u64(rec + 0, t0);
            agent_add_u64(rec + 1, t1);
            if (blockIdx.x == 0) agent_add_u64(rec + 2, a.n_elems);       // exactly one lane of the launch per image
        }
        __syncthreads();                              // `red` is free again before the next image of this workgroup fills it
    }
}

template <int ESZ> int digest_launch(const i2i_digest_params& p, hipStream_t s) {
    constexpr int64_t EPC = 16 / ESZ;
    DigestArgs a;
    a.x = (const char*)p.x, a.images = p.images, a.img_stride = p.img_stride;
    a.n_elems = (uint64_t)p.rows * (uint64_t)p.cols, a.index0 = p.index0, a.rec = p.rec;
    a.rows = p.rows, a.cols = p.cols, a.ld = p.ld;
    if (p.ld == p.cols || p.rows <= 1) a.cols = (int64_t)a.n_elems, a.rows = 1, a.ld = a.cols;      // contiguous images: one long row each
    // slices per image and the cap on the whole grid: scan_batch_launch's rule
    const int64_t per = SCAN_THREADS * SCAN_UNROLL;
    const bool chunks = a.rows == 1 || a.ld % EPC == 0;
    const int64_t work = chunks ? a.rows * ((a.cols + EPC - 1) / EPC) : a.rows * a.cols, want = (work + per - 1) / per;
    const unsigned gy = (unsigned)(p.images < DIGEST_MAX_GRID ? p.images : DIGEST_MAX_GRID);
    const int64_t cap = DIGEST_MAX_GRID / gy;
    const unsigned gx = (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
    const size_t smem = (SCAN_THREADS / 64) * 2 * sizeof(uint64_t);
    if (a.rows == 1) hipLaunchKernelGGL((digest_kernel<ESZ, true>), dim3(gx, gy), dim3(SCAN_THREADS), smem, s, a);
    else hipLaunchKernelGGL((digest_kernel<ESZ, false>), dim3(gx, gy), dim3(SCAN_THREADS), smem, s, a);
    return i2i::check_launch("digest");
}

inline unsigned grid_for(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// ---- repeat_interleave of up to 8 batch-outermost tensors in one launch (the contract is the comment of i2i_repeat_params).  A 1-D grid
// over the 16-byte vectors of all segments together: segment s owns the workgroups prefix[s] .. prefix[s + 1) and a workgroup copies
// REPEAT_CHUNK consecutive source vectors of it.  The segment of a workgroup is found from blockIdx alone (wave-uniform; the loop below is
// unrolled, so the by-value table is read at constant offsets of the kernel-argument segment).  Every source vector is loaded once -- the
// loads of a lane are issued together -- and stored V times.  All byte offsets are 64-bit; only the split of a vector's index into (image,
// vector in the image) runs in 32 bits: from the workgroup's first vector (one 64-bit division, uniform) a lane is less than
// vecs + REPEAT_CHUNK <= 2^31 + 1024 vectors away.
constexpr int REPEAT_THREADS = 256;
constexpr int REPEAT_UNROLL = 4;
constexpr int REPEAT_CHUNK = REPEAT_THREADS * REPEAT_UNROLL;       // source vectors per workgroup (16 KiB)

struct RepeatArgs {
    const u32x4* src[I2I_REPEAT_MAX_SEGMENTS];
    u32x4* dst[I2I_REPEAT_MAX_SEGMENTS];
    int64_t vecs[I2I_REPEAT_MAX_SEGMENTS];          // 16-byte vectors per image (>= 1 for every segment that owns a workgroup)
    int64_t total[I2I_REPEAT_MAX_SEGMENTS];         // batch * vecs
    uint32_t prefix[I2I_REPEAT_MAX_SEGMENTS + 1];   // first workgroup of segment s; an empty segment has prefix[s + 1] == prefix[s]
    int32_t n_seg, variations;
};

__global__ __launch_bounds__(REPEAT_THREADS) void repeat_kernel(const RepeatArgs a) {
    const uint32_t bid = blockIdx.x;
    const u32x4* src = a.src[0];
    u32x4* dst = a.dst[0];
    int64_t vecs = a.vecs[0], total = a.total[0];
    uint32_t first = a.prefix[0];
#pragma unroll
    for (int s = 1; s < I2I_REPEAT_MAX_SEGMENTS; ++s) {
        if (s < a.n_seg && a.prefix[s] <= bid) src = a.src[s], dst = a.dst[s], vecs = a.vecs[s], total = a.total[s], first = a.prefix[s];
    }
    const int64_t base = (int64_t)(bid - first) * REPEAT_CHUNK;     // first source vector of this workgroup (< total by construction)
    const int64_t b0 = base / vecs;
    const uint32_t r0 = (uint32_t)(base - b0 * vecs), vecs32 = (uint32_t)vecs;
    const int64_t V = a.variations;
    u32x4 v[REPEAT_UNROLL];
    int64_t out[REPEAT_UNROLL];
#pragma unroll
    for (int u = 0; u < REPEAT_UNROLL; ++u) {
        const uint32_t t = (uint32_t)(u * REPEAT_THREADS) + threadIdx.x;
        const int64_t i = base + t;
        out[u] = -1;
        if (i < total) {
            const uint32_t off = r0 + t, q = off / vecs32;          // (r0 < vecs <= 2^31, t < 1024: no wrap)
            out[u] = (b0 + q) * V * vecs + (off - q * vecs32);      // image-major: slot b * V + 0
            v[u] = src[i];
        }
    }
#pragma unroll
    for (int u = 0; u < REPEAT_UNROLL; ++u) {
        if (out[u] < 0) continue;
        u32x4* d = dst + out[u];
        for (int64_t k = 0; k < V; ++k, d += vecs) *d = v[u];
    }
}

}  // namespace

extern "C" int i2i_repeat(const i2i_repeat_params* p, int /*dtype*/, void* stream) {
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "repeat: null params");
    if (p->variations < 1) return i2i::fail(I2I_ERR_BAD_ARG, "repeat: variations = %d < 1", p->variations);
    if (p->batch < 0) return i2i::fail(I2I_ERR_BAD_ARG, "repeat: batch = %d < 0", p->batch);
    if (p->n_segments < 0 || p->n_segments > I2I_REPEAT_MAX_SEGMENTS)
        return i2i::fail(I2I_ERR_BAD_ARG, "repeat: n_segments = %d is outside 0 .. %d", p->n_segments, I2I_REPEAT_MAX_SEGMENTS);
    RepeatArgs a;
    memset(&a, 0, sizeof(a));
    a.n_seg = p->n_segments, a.variations = p->variations;
    uint64_t blocks = 0;
    for (int s = 0; s < p->n_segments; ++s) {
        const i2i_repeat_segment& g = p->seg[s];
        if (g.bytes_per_image < 0 || (g.bytes_per_image & 15) || g.bytes_per_image >= ((int64_t)1 << 35))
            return i2i::fail(I2I_ERR_BAD_ARG, "repeat: segment %d: bytes_per_image = %lld is not a multiple of 16 in 0 .. 2^35 - 16", s, (long long)g.bytes_per_image);
        if (!g.src || ((uintptr_t)g.src & 15)) return i2i::fail(I2I_ERR_BAD_ARG, "repeat: segment %d: src is null or not 16-byte aligned", s);
        if (!g.dst || ((uintptr_t)g.dst & 15)) return i2i::fail(I2I_ERR_BAD_ARG, "repeat: segment %d: dst is null or not 16-byte aligned", s);
        const int64_t big = (int64_t)1 << 61;
        if (p->batch > 0 && g.bytes_per_image > big / p->batch / p->variations)
            return i2i::fail(I2I_ERR_BAD_ARG, "repeat: segment %d: batch * variations * bytes_per_image = %d * %d * %lld is too large", s, p->batch, p->variations,
                             (long long)g.bytes_per_image);
        a.src[s] = (const u32x4*)g.src, a.dst[s] = (u32x4*)g.dst;
        a.vecs[s] = g.bytes_per_image / 16, a.total[s] = a.vecs[s] * p->batch;
        a.prefix[s] = (uint32_t)blocks;
        blocks += (uint64_t)((a.total[s] + REPEAT_CHUNK - 1) / REPEAT_CHUNK);
        if (blocks > 0x7FFFFFFFull) return i2i::fail(I2I_ERR_BAD_ARG, "repeat: segments 0 .. %d need more than 2^31 - 1 workgroups (bytes_per_image too large)", s);
    }
    for (int s = p->n_segments; s <= I2I_REPEAT_MAX_SEGMENTS; ++s) a.prefix[s] = (uint32_t)blocks;
    if (blocks == 0) return I2I_OK;
    hipLaunchKernelGGL(repeat_kernel, dim3((unsigned)blocks), dim3(REPEAT_THREADS), 0, (hipStream_t)stream, a);
    return i2i::check_launch("repeat");
}

extern "C" int i2i_digest(const i2i_digest_params* p, int dtype, void* stream) {
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "digest: null params");
    hipStream_t s = (hipStream_t)stream;
    if (p->kind == I2I_DIGEST_CLEAR) {
        if (!p->rec || ((uintptr_t)p->rec & 7)) return i2i::fail(I2I_ERR_BAD_ARG, "digest: rec is null or not 8-byte aligned");
        if (p->n_records < 0 || p->n_records > ((int64_t)1 << 40)) return i2i::fail(I2I_ERR_BAD_ARG, "digest: n_records = %lld", (long long)p->n_records);
        if (p->n_records == 0) return I2I_OK;
        hipLaunchKernelGGL(scan_verdict_clear_kernel, dim3(grid_for(p->n_records * 4)), dim3(256), 0, s, p->rec, p->n_records * 4);
        return i2i::check_launch("digest_clear");
    }
    if (p->kind != I2I_DIGEST_ADD) return i2i::fail(I2I_ERR_BAD_ARG, "digest: unknown kind %d", p->kind);
    const int esz = dtype == I2I_F32 ? 4 : (dtype == I2I_BF16 || dtype == I2I_F16) ? 2 : dtype == I2I_U8 ? 1 : 0;
    if (!esz) return i2i::fail(I2I_ERR_BAD_ARG, "digest: dtype %d is not one of u8 / f16 / bf16 / f32", dtype);
    if (p->images < 0) return i2i::fail(I2I_ERR_BAD_ARG, "digest: images = %d < 0", p->images);
    if (p->rows < 0 || p->cols < 0 || p->ld < p->cols)
        return i2i::fail(I2I_ERR_BAD_ARG, "digest: rows = %lld, cols = %d, ld = %lld", (long long)p->rows, p->cols, (long long)p->ld);
    const int64_t big = (int64_t)1 << 61;
    if (p->rows > 0 && p->ld > big / p->rows) return i2i::fail(I2I_ERR_BAD_ARG, "digest: rows * ld = %lld * %lld is too large", (long long)p->rows, (long long)p->ld);
    const int64_t extent = p->rows > 0 ? (p->rows - 1) * p->ld + p->cols : 0;      // elements from an image's first to behind its last
    if (p->images > 0 && (p->img_stride < extent || p->img_stride > big / p->images))
        return i2i::fail(I2I_ERR_BAD_ARG, "digest: img_stride = %lld (an image spans %lld elements, %d images)", (long long)p->img_stride, (long long)extent, p->images);
    if (p->images == 0 || p->rows == 0 || p->cols == 0) return I2I_OK;
    if (!p->x || !p->rec) return i2i::fail(I2I_ERR_BAD_ARG, "digest: null pointer");
    if ((uintptr_t)p->x % (uintptr_t)esz) return i2i::fail(I2I_ERR_BAD_ARG, "digest: x is not aligned to its element type");
    if ((uintptr_t)p->rec & 7) return i2i::fail(I2I_ERR_BAD_ARG, "digest: rec is not 8-byte aligned");
    return esz == 4 ? digest_launch<4>(*p, s) : esz == 2 ? digest_launch<2>(*p, s) : digest_launch<1>(*p, s);
}

extern "C" int i2i_nchw_to_nhwc(const i2i_nchw_to_nhwc_params* p, int dtype, void* stream) {
    if (!p || !p->x || !p->y || p->cpad < p->c) return i2i::fail(I2I_ERR_BAD_ARG, "nchw_to_nhwc: bad args");
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = grid_for((int64_t)p->n * p->h * p->w);
    if (p->src_dtype == I2I_U8) {
        switch (dtype) {
            case I2I_F32: hipLaunchKernelGGL((u8hwc_to_nhwc_kernel<float>), dim3(g), dim3(256), 0, s, *p); break;
            case I2I_BF16: hipLaunchKernelGGL((u8hwc_to_nhwc_kernel<__bf16>), dim3(g), dim3(256), 0, s, *p); break;
            case I2I_F16: hipLaunchKernelGGL((u8hwc_to_nhwc_kernel<_Float16>), dim3(g), dim3(256), 0, s, *p); break;
            default: return i2i::fail(I2I_ERR_BAD_ARG, "u8hwc_to_nhwc: bad dtype");
        }
        return i2i::check_launch("u8hwc_to_nhwc");
    }
    const bool src_f32 = p->src_dtype == I2I_F32;
    if (!src_f32 && p->src_dtype != dtype) return i2i::fail(I2I_ERR_BAD_ARG, "nchw_to_nhwc: src dtype must be f32 or the compute dtype");
    switch (dtype) {
        case I2I_F32: hipLaunchKernelGGL((nchw_to_nhwc_kernel<float, float>), dim3(g), dim3(256), 0, s, *p); break;
        case I2I_BF16:
            if (src_f32) hipLaunchKernelGGL((nchw_to_nhwc_kernel<__bf16, float>), dim3(g), dim3(256), 0, s, *p);
            else hipLaunchKernelGGL((nchw_to_nhwc_kernel<__bf16, __bf16>), dim3(g), dim3(256), 0, s, *p);
            break;
        case I2I_F16:
            if (src_f32) hipLaunchKernelGGL((nchw_to_nhwc_kernel<_Float16, float>), dim3(g), dim3(256), 0, s, *p);
            else hipLaunchKernelGGL((nchw_to_nhwc_kernel<_Float16, _Float16>), dim3(g), dim3(256), 0, s, *p);
            break;
        default: return i2i::fail(I2I_ERR_BAD_ARG, "nchw_to_nhwc: bad dtype");
    }
    return i2i::check_launch("nchw_to_nhwc");
}

extern "C" int i2i_nhwc_to_nchw(const i2i_nhwc_to_nchw_params* p, int dtype, void* stream) {
    if (!p || !p->x || !p->y || p->ldx < p->c) return i2i::fail(I2I_ERR_BAD_ARG, "nhwc_to_nchw: bad args");
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = grid_for((int64_t)p->n * p->h * p->w);
    if (p->dst_dtype == I2I_U8) {
        switch (dtype) {
            case I2I_F32: hipLaunchKernelGGL((nhwc_to_u8hwc_kernel<float>), dim3(g), dim3(256), 0, s, *p); break;
            case I2I_BF16: hipLaunchKernelGGL((nhwc_to_u8hwc_kernel<__bf16>), dim3(g), dim3(256), 0, s, *p); break;
            case I2I_F16: hipLaunchKernelGGL((nhwc_to_u8hwc_kernel<_Float16>), dim3(g), dim3(256), 0, s, *p); break;
            default: return i2i::fail(I2I_ERR_BAD_ARG, "nhwc_to_u8hwc: bad dtype");
        }
        return i2i::check_launch("nhwc_to_u8hwc");
    }
    const bool dst_f32 = p->dst_dtype == I2I_F32;
    if (!dst_f32 && p->dst_dtype != dtype) return i2i::fail(I2I_ERR_BAD_ARG, "nhwc_to_nchw: dst dtype must be f32 or the compute dtype");
    switch (dtype) {
        case I2I_F32: hipLaunchKernelGGL((nhwc_to_nchw_kernel<float, float>), dim3(g), dim3(256), 0, s, *p); break;
        case I2I_BF16:
            if (dst_f32) hipLaunchKernelGGL((nhwc_to_nchw_kernel<__bf16, float>), dim3(g), dim3(256), 0, s, *p);
            else hipLaunchKernelGGL((nhwc_to_nchw_kernel<__bf16, __bf16>), dim3(g), dim3(256), 0, s, *p);
            break;
        case I2I_F16:
            if (dst_f32) hipLaunchKernelGGL((nhwc_to_nchw_kernel<_Float16, float>), dim3(g), dim3(256), 0, s, *p);
            else hipLaunchKernelGGL((nhwc_to_nchw_kernel<_Float16, _Float16>), dim3(g), dim3(256), 0, s, *p);
            break;
        default: return i2i::fail(I2I_ERR_BAD_ARG, "nhwc_to_nchw: bad dtype");
    }
    return i2i::check_launch("nhwc_to_nchw");
}

extern "C" int i2i_posterior(const i2i_posterior_params* p, int dtype, void* stream) {
    if (!p || !p->moments || !p->eps || !p->u) return i2i::fail(I2I_ERR_BAD_ARG, "posterior: null pointer");
    if (p->ldm < 2 * p->lat || p->ldu < p->lat) return i2i::fail(I2I_ERR_BAD_ARG, "posterior: bad leading dims");
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = grid_for((int64_t)p->n * p->hw);
    switch (dtype) {
        case I2I_F32: hipLaunchKernelGGL((posterior_kernel<float>), dim3(g), dim3(256), 0, s, *p); break;
        case I2I_BF16: hipLaunchKernelGGL((posterior_kernel<__bf16>), dim3(g), dim3(256), 0, s, *p); break;
        case I2I_F16: hipLaunchKernelGGL((posterior_kernel<_Float16>), dim3(g), dim3(256), 0, s, *p); break;
        default: return i2i::fail(I2I_ERR_BAD_ARG, "posterior: bad dtype");
    }
    return i2i::check_launch("posterior");
}

extern "C" int i2i_ddpm_postquant(const i2i_ddpm_params* p, int dtype, void* stream) {
    if (!p || !p->u || !p->e || !p->y || !p->wpq || !p->bpq) return i2i::fail(I2I_ERR_BAD_ARG, "ddpm: null pointer");
    if (p->lat > 8 || p->ldy < p->lat) return i2i::fail(I2I_ERR_BAD_ARG, "ddpm: latent channels must be <= 8");
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = grid_for((int64_t)p->n * p->hw);
    switch (dtype) {
        case I2I_F32: hipLaunchKernelGGL((ddpm_kernel<float>), dim3(g), dim3(256), 0, s, *p); break;
        case I2I_BF16: hipLaunchKernelGGL((ddpm_kernel<__bf16>), dim3(g), dim3(256), 0, s, *p); break;
        case I2I_F16: hipLaunchKernelGGL((ddpm_kernel<_Float16>), dim3(g), dim3(256), 0, s, *p); break;
        default: return i2i::fail(I2I_ERR_BAD_ARG, "ddpm: bad dtype");
    }
    return i2i::check_launch("ddpm");
}

extern "C" int i2i_embed(const i2i_embed_params* p, int dtype, void* stream) {
    if (!p || !p->ids || !p->tok || !p->pos || !p->y || p->c % 8 || p->T < 1 || p->vocab < 1) return i2i::fail(I2I_ERR_BAD_ARG, "embed: bad args");
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = grid_for((int64_t)p->rows * (p->c / 4));
    switch (dtype) {
        case I2I_F32: hipLaunchKernelGGL((embed_kernel<float>), dim3(g), dim3(256), 0, s, *p); break;
        case I2I_BF16: hipLaunchKernelGGL((embed_kernel<__bf16>), dim3(g), dim3(256), 0, s, *p); break;
        case I2I_F16: hipLaunchKernelGGL((embed_kernel<_Float16>), dim3(g), dim3(256), 0, s, *p); break;
        default: return i2i::fail(I2I_ERR_BAD_ARG, "embed: bad dtype");
    }
    return i2i::check_launch("embed");
}

extern "C" int i2i_randn(const i2i_randn_params* p, int /*dtype*/, void* stream) {
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "randn: null params");
    hipStream_t s = (hipStream_t)stream;
    if (p->kind == I2I_RANDN_ADVANCE) {
        if (!p->state) return i2i::fail(I2I_ERR_BAD_ARG, "randn: advance needs the device state");
        hipLaunchKernelGGL(randn_advance_kernel, dim3(1), dim3(64), 0, s, (uint32_t*)p->state);
        return i2i::check_launch("randn_advance");
    }
    if (p->kind != I2I_RANDN_NORMAL && p->kind != I2I_RANDN_RAW) return i2i::fail(I2I_ERR_BAD_ARG, "randn: unknown kind %d", p->kind);
    if (p->n < 0) return i2i::fail(I2I_ERR_BAD_ARG, "randn: n = %lld < 0", (long long)p->n);
    if (p->n == 0) return I2I_OK;
    if (!p->dst || ((uintptr_t)p->dst & 3)) return i2i::fail(I2I_ERR_BAD_ARG, "randn: dst is null or not 4-byte aligned");
    // at most 1024 workgroups (4 per CU): 2^18 counters = 2^20 elements per pass of the grid-stride loop
    const int64_t b = (((p->n + 3) >> 2) + 255) / 256;
    const unsigned g = (unsigned)(b > 1024 ? 1024 : b);
    if (p->kind == I2I_RANDN_NORMAL) hipLaunchKernelGGL((randn_kernel<true>), dim3(g), dim3(256), 0, s, *p);
    else hipLaunchKernelGGL((randn_kernel<false>), dim3(g), dim3(256), 0, s, *p);
    return i2i::check_launch("randn");
}

extern "C" int i2i_randn_batch(const i2i_randn_batch_params* p, int /*dtype*/, void* stream) {
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "randn_batch: null params");
    if (!p->states || ((uintptr_t)p->states & 3)) return i2i::fail(I2I_ERR_BAD_ARG, "randn_batch: states is null or not 4-byte aligned");
    if (p->batch < 0 || p->per_image < 0) return i2i::fail(I2I_ERR_BAD_ARG, "randn_batch: batch = %d, per_image = %lld", p->batch, (long long)p->per_image);
    hipStream_t s = (hipStream_t)stream;
    if (p->kind == I2I_RANDN_ADVANCE) {
        if (p->batch == 0) return I2I_OK;
        const int g = (p->batch + 255) / 256;
        hipLaunchKernelGGL(randn_batch_advance_kernel, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(256), 0, s, (uint32_t*)p->states, p->batch);
        return i2i::check_launch("randn_batch_advance");
    }
    if (p->kind != I2I_RANDN_NORMAL && p->kind != I2I_RANDN_RAW) return i2i::fail(I2I_ERR_BAD_ARG, "randn_batch: unknown kind %d", p->kind);
    if (p->batch == 0 || p->per_image == 0) return I2I_OK;
    if (p->per_image > ((int64_t)1 << 61) / p->batch) return i2i::fail(I2I_ERR_BAD_ARG, "randn_batch: batch * per_image = %d * %lld is too large", p->batch, (long long)p->per_image);
    if (!p->dst || ((uintptr_t)p->dst & 3)) return i2i::fail(I2I_ERR_BAD_ARG, "randn_batch: dst is null or not 4-byte aligned");
    // grid (x, y) = (counters of an image, images), at most RANDN_BATCH_MAX_BLOCKS workgroups in all; both axes are grid-stride loops
    const unsigned gy = (unsigned)(p->batch > RANDN_BATCH_MAX_BLOCKS ? RANDN_BATCH_MAX_BLOCKS : p->batch);
    const int64_t b = (((p->per_image + 3) >> 2) + 255) / 256, cap = RANDN_BATCH_MAX_BLOCKS / gy;
    const unsigned gx = (unsigned)(b > cap ? cap : b);
    if (p->kind == I2I_RANDN_NORMAL) hipLaunchKernelGGL((randn_batch_kernel<true>), dim3(gx, gy), dim3(256), 0, s, *p);
    else hipLaunchKernelGGL((randn_batch_kernel<false>), dim3(gx, gy), dim3(256), 0, s, *p);
    return i2i::check_launch("randn_batch");
}

extern "C" int i2i_scan(const i2i_scan_params* p, int dtype, void* stream) {
    if (!p || !p->x || !p->rec) return i2i::fail(I2I_ERR_BAD_ARG, "scan: null pointer");
    if (!(p->limit > 0.f)) return i2i::fail(I2I_ERR_BAD_ARG, "scan: limit must be > 0");      // (a NaN limit fails the comparison too)
    if (p->rows < 0 || p->cols < 0 || p->ld < p->cols) return i2i::fail(I2I_ERR_BAD_ARG, "scan: rows = %lld, cols = %d, ld = %lld", (long long)p->rows, p->cols, (long long)p->ld);
    if ((uintptr_t)p->rec & 63) return i2i::fail(I2I_ERR_BAD_ARG, "scan: rec is not 64-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case I2I_F32: return scan_launch<float>(*p, s);
        case I2I_BF16: return scan_launch<__bf16>(*p, s);
        case I2I_F16: return scan_launch<_Float16>(*p, s);
        default: return i2i::fail(I2I_ERR_BAD_ARG, "scan: dtype %d is not a float type", dtype);
    }
}

extern "C" int i2i_scan_batch(const i2i_scan_batch_params* p, int dtype, void* stream) {
    if (!p || !p->x || !p->rec) return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: null pointer");
    if (p->images < 1) return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: images = %d < 1", p->images);
    if (!(p->limit > 0.f)) return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: limit must be > 0");      // (a NaN limit fails the comparison too)
    if (p->rows < 0 || p->cols < 0 || p->ld < p->cols)
        return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: rows = %lld, cols = %d, ld = %lld", (long long)p->rows, p->cols, (long long)p->ld);
    const int64_t big = (int64_t)1 << 61;
    if (p->rows > 0 && p->ld > big / p->rows) return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: rows * ld = %lld * %lld is too large", (long long)p->rows, (long long)p->ld);
    const int64_t extent = p->rows > 0 ? (p->rows - 1) * p->ld + p->cols : 0;      // elements from an image's first to behind its last
    if (p->img_stride < extent || p->img_stride > big / p->images)
        return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: img_stride = %lld (an image spans %lld elements, %d images)", (long long)p->img_stride, (long long)extent, p->images);
    if ((uintptr_t)p->rec & 63) return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: rec is not 64-byte aligned");
    if (p->rec_stride < 64 || (p->rec_stride & 63)) return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: rec_stride = %lld is not a multiple of 64 (>= 64)", (long long)p->rec_stride);
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case I2I_F32: return scan_batch_launch<float>(*p, s);
        case I2I_BF16: return scan_batch_launch<__bf16>(*p, s);
        case I2I_F16: return scan_batch_launch<_Float16>(*p, s);
        default: return i2i::fail(I2I_ERR_BAD_ARG, "scan_batch: dtype %d is not a float type", dtype);
    }
}

extern "C" int i2i_scan_verdict(const i2i_scan_verdict_params* p, int /*dtype*/, void* stream) {
    if (!p || !p->rec) return i2i::fail(I2I_ERR_BAD_ARG, "scan_verdict: null pointer");
    if ((uintptr_t)p->rec & 7) return i2i::fail(I2I_ERR_BAD_ARG, "scan_verdict: rec is not 8-byte aligned");
    if (p->taps < 0 || p->images < 1 || (int64_t)p->taps * p->images > ((int64_t)1 << 40))
        return i2i::fail(I2I_ERR_BAD_ARG, "scan_verdict: taps = %d, images = %d", p->taps, p->images);
    hipStream_t s = (hipStream_t)stream;
    if (p->mode == I2I_VERDICT_CLEAR) {
        const int64_t words = (int64_t)p->taps * p->images * 8;
        hipLaunchKernelGGL(scan_verdict_clear_kernel, dim3(grid_for(words)), dim3(256), 0, s, p->rec, words);
        return i2i::check_launch("scan_verdict_clear");
    }
    if (p->mode != I2I_VERDICT_JUDGE) return i2i::fail(I2I_ERR_BAD_ARG, "scan_verdict: unknown mode %d", p->mode);
    if (!p->verdict || ((uintptr_t)p->verdict & 3)) return i2i::fail(I2I_ERR_BAD_ARG, "scan_verdict: verdict is null or not 4-byte aligned");
    hipLaunchKernelGGL(scan_verdict_judge_kernel, dim3(grid_for(p->images)), dim3(256), 0, s, (const uint64_t*)p->rec, p->taps, p->images, p->verdict);
    return i2i::check_launch("scan_verdict_judge");
}

// PNG encoding of a ragged uint8 batch on the device (i2i_png_encode_u8; the contract -- Pillow's container and filter rule, this project's
// own deflate stream rule by rule, what is device state, the safety rule -- is the comment of i2i_png_image in include/i2i_turbo.h, and
// tests/png_ref.py is its integer restatement).  Included by resize.hip next to jpeg.inc, so both source lists reach it.
// The reference writes its result on the host: output_pil.save(...) (src/inference_paired.py:75, src/inference_unpaired.py:58) and
// canny_viz_inv.save(..._canny.png) (src/inference_paired.py:48-49).
//
// Six launches, grid y = image, grid x = a function of the capacity hint max_bytes only.  No kernel waits on another workgroup: what a
// stage needs from all workgroups of the one before (bits in front of a deflate block, the checksums) is stored per unit and reduced by
// every workgroup that needs it behind the launch boundary.
//   png_filter_kernel  a wave per row: the four costs of Pillow's rule, the choice, the filtered row into the stream F; zeroes the bit buffer
//   png_match_kernel   a thread per position of F: the longest match among the five candidate distances -> uint16 length | candidate << 9
//   png_code_kernel    a workgroup per deflate block of 16384 bytes: the greedy parse (a thread per segment of 64 positions: where a parse
//                      entering at each of its positions leaves the segment, then one lane hops over the segments, then every thread walks
//                      its segment from its entry), the two histograms (ds_add_u32), code lengths, canonical codes, the block header with
//                      its code-length code, the bit offset of every segment -> one record per block
//   png_pack_kernel    a workgroup per block: bits in front of the block (the second level), header words OR-ed in, every thread codes the
//                      tokens of its segment at its bit offset (LSB first; the first and last word shared with the neighbours: agent_or_u32
//                      into zeroed words, plain stores between), end-of-block
//   png_sum_kernel     per 1024 bytes: the Adler-32 terms of F and the CRC-32 register of the deflate bytes, each already carried to the end
//                      of its stream (A, B and the CRC are then plain sums / XORs)
//   png_emit_kernel    signature, IHDR, IDAT (zlib header, deflate bytes, Adler-32), IEND, length[b]; an image whose file does not fit its
//                      capacity is flagged here and nothing of it is written
// LDS of the parse: segment t at uint16 index 66 t (33 words): thread t's walk over its own segment lands in bank (33 t + const) mod 32, all
// different within each half wave.
namespace {
namespace png {

constexpr int BLOCK = I2I_PNG_BLOCK_BYTES;                   // bytes of F per deflate block
constexpr int SEG = 64, SEG_PITCH = 66;                      // positions per thread of the parse; uint16 per segment in LDS
constexpr int CHUNK = 1024;                                  // bytes per unit of the checksums and of the copy (four per thread)
constexpr int MAX_X = 1024;
constexpr int64_t MAX_BYTES = (int64_t)1 << 27;              // 16 bits per byte + 2301 per block < 2^32: bit offsets are uint32
constexpr int BLOCK_OVERHEAD_BITS = 2301;                    // 3 + 14 + 19 * 3 + 316 * 7 + 15 (i2i_png_bound)
constexpr int NLIT = 286, NDIST = 30, NCL = 19, NONE = 0xffff;
constexpr uint32_t ADLER = 65521, POLY = 0xedb88320u;
static_assert(BLOCK == 256 * SEG, "a thread per segment");

constexpr uint16_t LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t LEXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t DEXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
constexpr uint8_t CLORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
struct LenTab { uint8_t k[259]; };
constexpr LenTab make_lentab() {
    LenTab t{};
    for (int l = 3; l <= 258; ++l) {
        int k = 0;
        for (int i = 0; i < 29; ++i) if (LBASE[i] <= l) k = i;
        t.k[l] = (uint8_t)k;
    }
    return t;
}
constexpr LenTab LENTAB = make_lentab();

// ---- CRC-32 pieces (reflected polynomial): a * b mod P, x^(8 n) mod P, the register after some bytes
__host__ __device__ constexpr uint32_t gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ POLY : b >> 1;
    }
    return p;
}
struct PowTab { uint32_t v[32]; };
constexpr PowTab make_powtab() {                             // v[k] = x^(2^k)
    PowTab t{};
    t.v[0] = 0x40000000u;
    for (int k = 1; k < 32; ++k) t.v[k] = gf2_mul(t.v[k - 1], t.v[k - 1]);
    return t;
}
constexpr PowTab POWTAB = make_powtab();
// the register r carried over n further bytes of zeros-from-nothing: r * x^(8 n) mod P
__host__ __device__ __forceinline__ uint32_t crc_shift(uint32_t r, uint64_t n) {
    if (r == 0) return 0;
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1) r = gf2_mul(POWTAB.v[k & 31], r);
    return r;
}
__host__ __device__ __forceinline__ uint32_t crc_byte(uint32_t r, uint32_t byte) {
    r ^= byte;
    for (int i = 0; i < 8; ++i) r = (r & 1) ? (r >> 1) ^ POLY : r >> 1;
    return r;
}

// one record per deflate block, uint32 words
constexpr int REC_LIT = 0, REC_DIST = 288, REC_HDR = 320, HDR_WORDS = 76, REC_HDR_BITS = 396, REC_BITS = 397, REC_ENTRY = 400, REC_OFF = 656,
              REC_WORDS = 912;

// byte offsets inside an image's slot of the workspace, a function of max_bytes alone
struct Slot { int64_t f, tok, rec, stream, adler, crc, meta, total; int64_t blocks, words; };
__host__ __device__ __forceinline__ int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
__host__ __device__ __forceinline__ int64_t stream_words(int64_t bytes, int64_t blocks) { return ((16 * bytes + BLOCK_OVERHEAD_BITS * blocks + 31) / 32 + 4 + 3) & ~(int64_t)3; }
__host__ __device__ __forceinline__ Slot slot_layout(int64_t m) {
    Slot L;
    L.blocks = (m + BLOCK - 1) / BLOCK;
    L.f = 0;                                                 // uint8 [m]
    L.tok = up16(m);                                         // uint16 [m]
    L.rec = L.tok + up16(2 * m);                             // uint32 [blocks][REC_WORDS]
    L.stream = L.rec + L.blocks * REC_WORDS * 4;             // uint32 [words]
    L.words = stream_words(m, L.blocks);
    L.adler = L.stream + L.words * 4;                        // uint32 [chunks of F][2]
    L.crc = L.adler + (m + CHUNK - 1) / CHUNK * 8;           // uint32 [chunks of the stream]
    L.meta = L.crc + (L.words * 4 + CHUNK - 1) / CHUNK * 4;  // uint32: bits of the deflate stream
    L.total = up16(L.meta + 4);
    return L;
}

struct Geo { int wc, S; int64_t bytes, blocks; };

// Whether the descriptor may be worked on: the same verdict in every workgroup of every stage.  Sizes as quotients: no product can overflow.
__device__ __forceinline__ bool image_ok(const i2i_png_encode_u8_params& p, const i2i_png_image& d, Geo& g) {
    const bool ok = d.h >= 1 && d.h <= 65535 && d.w >= 1 && d.w <= 65535 && (d.c == 1 || d.c == 3) && d.src_off >= 0 && d.src_off <= p.src_bytes &&
                    d.dst_off >= 0 && d.dst_off <= p.dst_bytes && d.capacity >= 0 && d.capacity <= p.dst_bytes - d.dst_off;
    if (!ok) return false;
    if ((int64_t)d.h * d.w > (p.src_bytes - d.src_off) / d.c) return false;
    g.wc = d.w * d.c;
    g.S = 1 + g.wc;
    g.bytes = (int64_t)d.h * g.S;
    g.blocks = (g.bytes + BLOCK - 1) / BLOCK;
    return g.bytes <= p.max_bytes;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int cost_of(int v) { return v < 128 ? v : 256 - v; }
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// ------------------------------------------------------------------------------------------------------------------------ stage 1
__global__ __launch_bounds__(256) void png_filter_kernel(const i2i_png_encode_u8_params p) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Slot L = slot_layout(p.max_bytes);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_png_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) {
            if (p.bad_mask && blockIdx.x == 0 && tid == 0) agent_or_u32(p.bad_mask, 1u << (b & 31));
            continue;
        }
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        u32x4* zero = (u32x4*)(ws + L.stream);
        const int64_t nzero = stream_words(g.bytes, g.blocks) / 4;
        for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < nzero; i += (int64_t)gridDim.x * 256) zero[i] = u32x4{0, 0, 0, 0};
        const uint8_t* __restrict__ px = (const uint8_t*)p.src + d.src_off;
        uint8_t* F = (uint8_t*)(ws + L.f);
        const int inv = d.flags & 1, c = d.c;
        for (int r0 = (int)blockIdx.x * 4; r0 < d.h; r0 += (int)gridDim.x * 4) {
            const int y = r0 + wave;
            if (y >= d.h) continue;                          // (wave-uniform)
            const uint8_t* __restrict__ cur = px + (int64_t)y * g.wc;
            const uint8_t* __restrict__ abv = cur - g.wc;
            int c0 = 0, c1 = 0, c2 = 0, c4 = 0;
            for (int i = lane; i < g.wc; i += 64) {
                const int x = inv ? 255 - cur[i] : cur[i];
                const int a = i >= c ? (inv ? 255 - cur[i - c] : cur[i - c]) : 0;
                const int u = y > 0 ? (inv ? 255 - abv[i] : abv[i]) : 0;
                const int q = (y > 0 && i >= c) ? (inv ? 255 - abv[i - c] : abv[i - c]) : 0;
                const int pa = iabs(u - q), pb = iabs(a - q), pc = iabs(a + u - 2 * q);
                const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? u : q);
                c0 += cost_of(x);
                c1 += cost_of((x - a) & 255);
                c2 += cost_of((x - u) & 255);
                c4 += cost_of((x - pr) & 255);
            }
            c0 = wave_sum_i32(c0);
            c1 = wave_sum_i32(c1);
            c2 = wave_sum_i32(c2);
            c4 = wave_sum_i32(c4);
            int type = 0, best = c0;
            if (best > 0 && c2 < best) { type = 2; best = c2; }
            if (best > 0 && c1 < best) { type = 1; best = c1; }
            if (best > 0 && c4 < best) { type = 4; best = c4; }
            uint8_t* out = F + (int64_t)y * g.S;
            if (lane == 0) out[0] = (uint8_t)type;
            for (int i = lane; i < g.wc; i += 64) {
                const int x = inv ? 255 - cur[i] : cur[i];
                const int a = i >= c ? (inv ? 255 - cur[i - c] : cur[i - c]) : 0;
                const int u = y > 0 ? (inv ? 255 - abv[i] : abv[i]) : 0;
                const int q = (y > 0 && i >= c) ? (inv ? 255 - abv[i - c] : abv[i - c]) : 0;
                const int pa = iabs(u - q), pb = iabs(a - q), pc = iabs(a + u - 2 * q);
                const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? u : q);
                const int v = type == 0 ? x : (type == 1 ? x - a : (type == 2 ? x - u : x - pr));
                out[1 + i] = (uint8_t)(v & 255);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ stage 2
__device__ __forceinline__ void candidates(const Geo& g, int c, int (&dist)[5]) {
    dist[0] = 1; dist[1] = c; dist[2] = g.S; dist[3] = g.S - c; dist[4] = g.S + c;
}

__global__ __launch_bounds__(256) void png_match_kernel(const i2i_png_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    const Slot L = slot_layout(p.max_bytes);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_png_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) continue;
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const uint8_t* __restrict__ F = (const uint8_t*)(ws + L.f);
        uint16_t* tok = (uint16_t*)(ws + L.tok);
        int dist[5];
        candidates(g, d.c, dist);
        for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < g.bytes; q += (int64_t)gridDim.x * 256) {
            int64_t end = (q / BLOCK + 1) * BLOCK;
            end = end < g.bytes ? end : g.bytes;
            const int room = end - q < 258 ? (int)(end - q) : 258;
            int best = 0, cand = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int dd = dist[k];
                if (dd > 32768 || dd > q) continue;
                const uint8_t* __restrict__ s = F + q;
                int l = 0;
                while (l < room && s[l] == s[l - dd]) ++l;
                if (l > best) { best = l; cand = k; }
            }
            tok[q] = best >= 3 ? (uint16_t)(best | (cand << 9)) : (uint16_t)0;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ stage 3
// LDS of png_code_kernel, uint32 words behind the 256 * 66 uint16 of the parse
struct CodeLds {
    uint16_t* nxt;                                           // [256 * SEG_PITCH]
    uint32_t *entry, *lf, *df, *cf, *ll, *dl, *cl, *lc, *dc, *cc, *sw, *ss, *nodew, *lp, *np, *depth, *count, *rle, *hdr, *scan, *misc;
};
constexpr int CODE_LDS_WORDS = 256 * SEG_PITCH / 2 + 256 + 288 + 32 + 32 + 288 + 32 + 32 + 288 + 32 + 32 + 6 * 288 + 16 + 320 + HDR_WORDS + 256 + 16;
__device__ __forceinline__ CodeLds carve() {
    CodeLds s;
    uint32_t* w = (uint32_t*)i2i_smem;
    s.nxt = (uint16_t*)w; w += 256 * SEG_PITCH / 2;
    s.entry = w; w += 256;
    s.lf = w; w += 288;  s.df = w; w += 32;  s.cf = w; w += 32;
    s.ll = w; w += 288;  s.dl = w; w += 32;  s.cl = w; w += 32;
    s.lc = w; w += 288;  s.dc = w; w += 32;  s.cc = w; w += 32;
    s.sw = w; w += 288;  s.ss = w; w += 288;  s.nodew = w; w += 288;  s.lp = w; w += 288;  s.np = w; w += 288;  s.depth = w; w += 288;
    s.count = w; w += 16;
    s.rle = w; w += 320;
    s.hdr = w; w += HDR_WORDS;
    s.scan = w; w += 256;
    s.misc = w;
    return s;
}

// Code lengths of `nsym` <= 286 symbols from their frequencies, at most `limit` bits (the whole workgroup; the rule is in the contract):
// sorted by (frequency, symbol) with a rank per symbol, the two-queue merge and the repair by one lane, the lengths dealt by sorted order.
// misc[0] receives 1 if the repair ran.  Ends behind a barrier.
__device__ void build_lengths(const CodeLds& s, const uint32_t* freq, int nsym, int limit, uint32_t* lens) {
    const int tid = (int)threadIdx.x;
    const uint32_t f0 = tid < nsym ? freq[tid] : 0, f1 = tid + 256 < nsym ? freq[tid + 256] : 0;
    int n = 0, r0 = 0, r1 = 0;
    for (int k = 0; k < nsym; ++k) {
        const uint32_t f = freq[k];
        if (!f) continue;
        ++n;
        r0 += (f < f0 || (f == f0 && k < tid)) ? 1 : 0;
        r1 += (f < f1 || (f == f1 && k < tid + 256)) ? 1 : 0;
    }
    if (tid < nsym) lens[tid] = 0;
    if (tid + 256 < nsym) lens[tid + 256] = 0;
    if (f0) { s.sw[r0] = f0; s.ss[r0] = (uint32_t)tid; }
    if (f1) { s.sw[r1] = f1; s.ss[r1] = (uint32_t)(tid + 256); }
    __syncthreads();
    if (tid == 0) {
        s.misc[0] = 0;
        if (n == 1) {
            lens[s.ss[0]] = 1;
        } else if (n >= 2) {
            int i = 0, j = 0;
            for (int k = 0; k < n - 1; ++k) {
                uint32_t w = 0;
                for (int t = 0; t < 2; ++t) {
                    if (i < n && (j >= k || s.sw[i] <= s.nodew[j])) { w += s.sw[i]; s.lp[i] = (uint32_t)k; ++i; }
                    else { w += s.nodew[j]; s.np[j] = (uint32_t)k; ++j; }
                }
                s.nodew[k] = w;
            }
            s.depth[n - 2] = 0;
            for (int k = n - 3; k >= 0; --k) s.depth[k] = s.depth[s.np[k]] + 1;
            for (int l = 0; l <= limit; ++l) s.count[l] = 0;
            for (int x = 0; x < n; ++x) {
                const int dl = (int)s.depth[s.lp[x]] + 1;
                ++s.count[dl < limit ? dl : limit];
            }
            int64_t kraft = 0;
            for (int l = 1; l <= limit; ++l) kraft += (int64_t)s.count[l] << (limit - l);
            int64_t excess = kraft - ((int64_t)1 << limit);
            if (excess > 0) s.misc[0] = 1;
            for (; excess > 0; --excess) {                   // the deepest leaf above the limit row moves one down, a leaf of the limit row becomes its brother
                int l = limit - 1;
                while (l > 0 && s.count[l] == 0) --l;
                if (l == 0 || s.count[limit] == 0) break;     // (cannot happen: the excess is made of leaves in the limit row)
                --s.count[l];
                s.count[l + 1] += 2;
                --s.count[limit];
            }
            int r = 0;
            for (int l = limit; l >= 1; --l)
                for (uint32_t q = 0; q < s.count[l] && r < n; ++q) lens[s.ss[r++]] = (uint32_t)l;
        }
    }
    __syncthreads();
}

// canonical codes (RFC 1951 3.2.2) of the lengths, bit-reversed: code[s] = (reversed code << 8) | length.  Ends behind a barrier.
__device__ void build_codes(const uint32_t* lens, int nsym, uint32_t* code) {
    const int tid = (int)threadIdx.x;
    for (int sy = tid; sy < nsym; sy += 256) {
        const int len = (int)lens[sy];
        uint32_t v = 0;
        if (len) {
            uint32_t cnt[16];
#pragma unroll
            for (int l = 0; l < 16; ++l) cnt[l] = 0;
            uint32_t before = 0;
            for (int k = 0; k < nsym; ++k) {
                const int lk = (int)lens[k];
#pragma unroll
                for (int l = 1; l < 16; ++l) cnt[l] += (lk == l) ? 1 : 0;
                before += (lk == len && k < sy) ? 1 : 0;
            }
            uint32_t c = 0, first = 0;
#pragma unroll
            for (int l = 1; l < 16; ++l) {
                c = (c + cnt[l - 1]) << 1;
                if (l == len) first = c;
            }
            v = ((__builtin_bitreverse32(first + before) >> (32 - len)) << 8) | (uint32_t)len;
        }
        code[sy] = v;
    }
    __syncthreads();
}

// distance -> (symbol, extra bits, extra value)
__device__ __forceinline__ void dist_symbol(int dd, int& sym, int& eb, int& ev) {
    sym = 0;
    for (int i = 1; i < 30; ++i) if ((int)DBASE[i] <= dd) sym = i;
    eb = DEXTRA[sym];
    ev = dd - DBASE[sym];
}

// LSB-first writer into LDS words (the block header, one lane)
struct LocalBits { uint32_t* w; uint32_t n; };
__device__ __forceinline__ void put_local(LocalBits& o, uint32_t v, int len) {
    const uint32_t at = o.n >> 5, sh = o.n & 31;
    o.w[at] |= v << sh;
    if (sh + len > 32) o.w[at + 1] |= v >> (32 - sh);
    o.n += len;
}

__global__ __launch_bounds__(256) void png_code_kernel(const i2i_png_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    const CodeLds s = carve();
    const Slot L = slot_layout(p.max_bytes);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_png_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) continue;
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const uint8_t* __restrict__ F = (const uint8_t*)(ws + L.f);
        const uint16_t* __restrict__ tok = (const uint16_t*)(ws + L.tok);
        int dist[5], dsym[5], deb[5], dev[5];
        candidates(g, d.c, dist);
#pragma unroll
        for (int k = 0; k < 5; ++k) dist_symbol(dist[k] <= 32768 ? dist[k] : 1, dsym[k], deb[k], dev[k]);
        for (int64_t blk = blockIdx.x; blk < g.blocks; blk += gridDim.x) {
            const int64_t lo = blk * BLOCK;
            const int nb = g.bytes - lo < BLOCK ? (int)(g.bytes - lo) : BLOCK;
            uint32_t* rec = (uint32_t*)(ws + L.rec) + blk * REC_WORDS;
            // the tokens of the block into LDS, the histograms cleared
            for (int i = tid; i < BLOCK; i += 256) s.nxt[(i >> 6) * SEG_PITCH + (i & 63)] = i < nb ? tok[lo + i] : (uint16_t)0;
            for (int i = tid; i < 288; i += 256) s.lf[i] = 0;
            if (tid < 32) { s.df[tid] = 0; s.cf[tid] = 0; }
            s.entry[tid] = NONE;
            for (int i = tid; i < HDR_WORDS; i += 256) s.hdr[i] = 0;
            __syncthreads();
            // where a parse that enters the segment at position e leaves it (backwards, in place)
            {
                uint16_t* mine = s.nxt + tid * SEG_PITCH;
                const int base = tid * SEG;
                for (int e = SEG - 1; e >= 0; --e) {
                    const int l = mine[e] & 511;
                    const int nx = base + e + (l > 1 ? l : 1);
                    mine[e] = (uint16_t)(nx >= base + SEG ? nx : mine[nx - base]);
                }
            }
            __syncthreads();
            if (tid == 0) {
                int q = 0;
                while (q < nb) {
                    s.entry[q >> 6] = (uint32_t)q;
                    q = s.nxt[(q >> 6) * SEG_PITCH + (q & 63)];
                }
            }
            __syncthreads();
            const int entry = (int)s.entry[tid];
            const int seg_end = (tid + 1) * SEG < nb ? (tid + 1) * SEG : nb;
            if (entry != NONE) {
                for (int q = entry; q < seg_end;) {
                    const int t = tok[lo + q], l = t & 511;
                    if (l) {
                        lds_add_u32(s.lf + 257 + LENTAB.k[l], 1);
                        lds_add_u32(s.df + dsym[t >> 9], 1);
                        q += l;
                    } else {
                        lds_add_u32(s.lf + F[lo + q], 1);
                        ++q;
                    }
                }
            }
            if (tid == 0) lds_add_u32(s.lf + 256, 1);
            __syncthreads();
            build_lengths(s, s.lf, NLIT, 15, s.ll);
            build_lengths(s, s.df, NDIST, 15, s.dl);
            build_codes(s.ll, NLIT, s.lc);
            build_codes(s.dl, NDIST, s.dc);
            // the two length lists as one run-length coded sequence, its histogram
            if (tid == 0) {
                int nlit = NLIT, ndist = NDIST;
                while (nlit > 257 && s.ll[nlit - 1] == 0) --nlit;
                while (ndist > 1 && s.dl[ndist - 1] == 0) --ndist;
                const int n = nlit + ndist;
                int m = 0;
                for (int i = 0; i < n;) {
                    const uint32_t v = i < nlit ? s.ll[i] : s.dl[i - nlit];
                    int r = 1;
                    while (i + r < n && (i + r < nlit ? s.ll[i + r] : s.dl[i + r - nlit]) == v) ++r;
                    i += r;
                    if (v == 0) {
                        while (r >= 11) {
                            const int k = r < 138 ? r : 138;
                            s.rle[m++] = 18u | ((uint32_t)(k - 11) << 8) | (7u << 16);
                            r -= k;
                        }
                        if (r >= 3) {
                            s.rle[m++] = 17u | ((uint32_t)(r - 3) << 8) | (3u << 16);
                            r = 0;
                        }
                    } else {
                        s.rle[m++] = v;
                        --r;
                        while (r >= 3) {
                            const int k = r < 6 ? r : 6;
                            s.rle[m++] = 16u | ((uint32_t)(k - 3) << 8) | (2u << 16);
                            r -= k;
                        }
                    }
                    for (; r > 0; --r) s.rle[m++] = v;
                }
                for (int i = 0; i < m; ++i) ++s.cf[s.rle[i] & 255];
                s.misc[1] = (uint32_t)m;
                s.misc[2] = (uint32_t)nlit;
                s.misc[3] = (uint32_t)ndist;
            }
            __syncthreads();
            build_lengths(s, s.cf, NCL, 7, s.cl);
            build_codes(s.cl, NCL, s.cc);
            if (tid == 0) {
                const int m = (int)s.misc[1];
                int nclen = NCL;
                while (nclen > 4 && s.cl[CLORDER[nclen - 1]] == 0) --nclen;
                LocalBits o = {s.hdr, 0};
                put_local(o, blk == g.blocks - 1 ? 1 : 0, 1);
                put_local(o, 2, 2);
                put_local(o, s.misc[2] - 257, 5);
                put_local(o, s.misc[3] - 1, 5);
                put_local(o, (uint32_t)(nclen - 4), 4);
                for (int i = 0; i < nclen; ++i) put_local(o, s.cl[CLORDER[i]], 3);
                for (int i = 0; i < m; ++i) {
                    const uint32_t e = s.rle[i], cd = s.cc[e & 255];
                    put_local(o, cd >> 8, (int)(cd & 255));
                    if (e >> 16) put_local(o, (e >> 8) & 255, (int)(e >> 16));
                }
                s.misc[4] = o.n;
            }
            // bits of every segment, their exclusive scan
            uint32_t bits = 0;
            if (entry != NONE) {
                for (int q = entry; q < seg_end;) {
                    const int t = tok[lo + q], l = t & 511;
                    if (l) {
                        const int k = LENTAB.k[l];
                        bits += (s.lc[257 + k] & 255) + LEXTRA[k] + (s.dc[dsym[t >> 9]] & 255) + deb[t >> 9];
                        q += l;
                    } else {
                        bits += s.lc[F[lo + q]] & 255;
                        ++q;
                    }
                }
            }
            s.scan[tid] = bits;
            __syncthreads();
            for (int step = 1; step < 256; step <<= 1) {
                const uint32_t add = tid >= step ? s.scan[tid - step] : 0;
                __syncthreads();
                s.scan[tid] += add;
                __syncthreads();
            }
            for (int i = tid; i < 288; i += 256) rec[REC_LIT + i] = i < NLIT ? s.lc[i] : 0;
            if (tid < 32) rec[REC_DIST + tid] = tid < NDIST ? s.dc[tid] : 0;
            for (int i = tid; i < HDR_WORDS; i += 256) rec[REC_HDR + i] = s.hdr[i];
            rec[REC_ENTRY + tid] = (uint32_t)entry;
            rec[REC_OFF + tid] = s.misc[4] + s.scan[tid] - bits;
            if (tid == 0) {
                rec[REC_HDR_BITS] = s.misc[4];
                rec[REC_BITS] = s.misc[4] + s.scan[255] + (s.lc[256] & 255);
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ stage 4
// LSB-first bit writer into the 32-bit words of the stream: the word a unit starts in (if it does not start on a word boundary) and the word
// it ends in are shared with its neighbours and OR-ed into the zeroed buffer, the words between are the unit's own
struct BitSink { uint32_t* words; uint64_t acc; int n; bool shared; };
__device__ __forceinline__ void put(BitSink& o, uint32_t v, int len) {
    o.acc |= (uint64_t)v << o.n;
    o.n += len;
    if (o.n >= 32) {
        if (o.shared) agent_or_u32(o.words, (uint32_t)o.acc);
        else *o.words = (uint32_t)o.acc;
        o.shared = false;
        ++o.words;
        o.acc >>= 32;
        o.n -= 32;
    }
}
__device__ __forceinline__ BitSink sink_at(uint32_t* stream, uint32_t at) { return BitSink{stream + (at >> 5), 0, (int)(at & 31), (at & 31) != 0}; }
__device__ __forceinline__ void flush(BitSink& o) { if (o.n > 0) agent_or_u32(o.words, (uint32_t)o.acc); }

__global__ __launch_bounds__(256) void png_pack_kernel(const i2i_png_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    uint32_t* lc = (uint32_t*)i2i_smem;                      // [288], then dc [32], then red [256]
    uint32_t* dc = lc + 288;
    uint32_t* red = dc + 32;
    const Slot L = slot_layout(p.max_bytes);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_png_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) continue;
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const uint8_t* __restrict__ F = (const uint8_t*)(ws + L.f);
        const uint16_t* __restrict__ tok = (const uint16_t*)(ws + L.tok);
        uint32_t* stream = (uint32_t*)(ws + L.stream);
        const uint32_t most = (uint32_t)(16 * g.bytes + BLOCK_OVERHEAD_BITS * g.blocks);
        int dist[5], dsym[5], deb[5], dev[5];
        candidates(g, d.c, dist);
#pragma unroll
        for (int k = 0; k < 5; ++k) dist_symbol(dist[k] <= 32768 ? dist[k] : 1, dsym[k], deb[k], dev[k]);
        for (int64_t blk = blockIdx.x; blk < g.blocks; blk += gridDim.x) {
            const uint32_t* __restrict__ recs = (const uint32_t*)(ws + L.rec);
            const uint32_t* __restrict__ rec = recs + blk * REC_WORDS;
            uint32_t front = 0;                               // the second level: the bits in front of this block
            for (int64_t i = tid; i < blk; i += 256) front += recs[i * REC_WORDS + REC_BITS];
            red[tid] = front;
            for (int i = tid; i < 288; i += 256) lc[i] = rec[REC_LIT + i];
            if (tid < 32) dc[tid] = rec[REC_DIST + tid];
            __syncthreads();
            for (int step = 128; step > 0; step >>= 1) {
                if (tid < step) red[tid] += red[tid + step];
                __syncthreads();
            }
            front = red[0];
            const uint32_t hdr_bits = rec[REC_HDR_BITS], bits = rec[REC_BITS];
            const bool fits = front <= most && bits <= most - front;      // (what stage 3 wrote; never past the buffer)
            const int64_t lo = blk * BLOCK;
            const int nb = g.bytes - lo < BLOCK ? (int)(g.bytes - lo) : BLOCK;
            if (fits) {
                if (tid < HDR_WORDS && (uint32_t)tid * 32 < hdr_bits) {
                    const uint32_t at = front + 32 * tid, sh = at & 31, v = rec[REC_HDR + tid];
                    if (v) {
                        agent_or_u32(stream + (at >> 5), v << sh);
                        if (sh && (v >> (32 - sh))) agent_or_u32(stream + (at >> 5) + 1, v >> (32 - sh));
                    }
                }
                const int entry = (int)rec[REC_ENTRY + tid];
                const int seg_end = (tid + 1) * SEG < nb ? (tid + 1) * SEG : nb;
                if (entry != NONE && entry < seg_end && rec[REC_OFF + tid] <= bits) {
                    BitSink o = sink_at(stream, front + rec[REC_OFF + tid]);
                    for (int q = entry; q < seg_end;) {
                        const int t = tok[lo + q], l = t & 511;
                        if (l) {
                            const int k = LENTAB.k[l], cd = t >> 9;
                            put(o, lc[257 + k] >> 8, (int)(lc[257 + k] & 255));
                            if (LEXTRA[k]) put(o, (uint32_t)(l - LBASE[k]), LEXTRA[k]);
                            put(o, dc[dsym[cd]] >> 8, (int)(dc[dsym[cd]] & 255));
                            if (deb[cd]) put(o, (uint32_t)dev[cd], deb[cd]);
                            q += l;
                        } else {
                            const uint32_t e = lc[F[lo + q]];
                            put(o, e >> 8, (int)(e & 255));
                            ++q;
                        }
                    }
                    flush(o);
                }
                if (tid == 0) {
                    const uint32_t e = lc[256];
                    BitSink o = sink_at(stream, front + bits - (e & 255));
                    o.shared = true;
                    put(o, e >> 8, (int)(e & 255));
                    flush(o);
                }
            }
            if (tid == 0 && blk == g.blocks - 1) *(uint32_t*)(ws + L.meta) = fits ? front + bits : 0;
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ stages 5 and 6
// bytes of the deflate stream as the last two stages see them (what stage 4 wrote; never more than the buffer holds)
__device__ __forceinline__ int64_t deflate_bytes(const char* ws, const Slot& L, const Geo& g) {
    const uint32_t bits = *(const uint32_t*)(ws + L.meta);
    const int64_t most = stream_words(g.bytes, g.blocks) * 4 - 16;
    const int64_t n = ((int64_t)bits + 7) >> 3;
    return n < most ? n : most;
}

__global__ __launch_bounds__(256) void png_sum_kernel(const i2i_png_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    uint32_t* red = (uint32_t*)i2i_smem;                     // [512]
    const Slot L = slot_layout(p.max_bytes);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_png_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) continue;
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const uint8_t* __restrict__ F = (const uint8_t*)(ws + L.f);
        uint32_t* adler = (uint32_t*)(ws + L.adler);
        const int64_t fchunks = (g.bytes + CHUNK - 1) / CHUNK;
        for (int64_t ch = blockIdx.x; ch < fchunks; ch += gridDim.x) {
            const int64_t lo = ch * CHUNK, end = lo + CHUNK < g.bytes ? lo + CHUNK : g.bytes;
            uint32_t sum = 0, wsum = 0;                       // sum of the bytes; sum of (bytes from this one to the end of the chunk) * byte
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = lo + 4 * tid + k;
                if (i < end) {
                    sum += F[i];
                    wsum += (uint32_t)(end - i) * F[i];
                }
            }
            red[tid] = sum;
            red[256 + tid] = wsum;
            __syncthreads();
            for (int step = 128; step > 0; step >>= 1) {
                if (tid < step) {
                    red[tid] += red[tid + step];
                    red[256 + tid] += red[256 + tid + step];
                }
                __syncthreads();
            }
            if (tid == 0) {                                   // B counts every byte once for each byte from it to the end of F
                adler[2 * ch] = red[0];
                adler[2 * ch + 1] = (uint32_t)((red[256] % ADLER + (uint64_t)(red[0] % ADLER) * (uint64_t)((g.bytes - end) % ADLER)) % ADLER);
            }
            __syncthreads();
        }
        const int64_t nd = deflate_bytes(ws, L, g);
        const uint8_t* __restrict__ z = (const uint8_t*)(ws + L.stream);
        uint32_t* crc = (uint32_t*)(ws + L.crc);
        const int64_t zchunks = (nd + CHUNK - 1) / CHUNK;
        for (int64_t ch = blockIdx.x; ch < zchunks; ch += gridDim.x) {
            const int64_t lo = ch * CHUNK, end = lo + CHUNK < nd ? lo + CHUNK : nd;
            uint32_t r = 0;
            int64_t last = lo + 4 * tid;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = lo + 4 * tid + k;
                if (i < end) {
                    r = crc_byte(r, z[i]);
                    last = i + 1;
                }
            }
            red[tid] = crc_shift(r, (uint64_t)(nd - last));  // carried to the end of the deflate bytes
            __syncthreads();
            for (int step = 128; step > 0; step >>= 1) {
                if (tid < step) red[tid] ^= red[tid + step];
                __syncthreads();
            }
            if (tid == 0) crc[ch] = red[0];
            __syncthreads();
        }
    }
}

constexpr int FRONT = 43;                                    // signature 8, IHDR 25, IDAT length and type 8, zlib header 2
constexpr int BACK = 20;                                     // Adler-32 4, CRC 4, IEND 12

__global__ __launch_bounds__(256) void png_emit_kernel(const i2i_png_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    uint32_t* red = (uint32_t*)i2i_smem;                     // [768]
    const Slot L = slot_layout(p.max_bytes);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_png_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) {                            // (flagged by stage 1)
            if (blockIdx.x == 0 && tid == 0) p.length[b] = 0;
            continue;
        }
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const int64_t nd = deflate_bytes(ws, L, g);
        const int64_t total = FRONT + nd + BACK;
        if (total > d.capacity || nd == 0) {                 // the same verdict in every workgroup of the image: nothing is written
            if (blockIdx.x == 0 && tid == 0) {
                p.length[b] = 0;
                if (p.bad_mask) agent_or_u32(p.bad_mask, 1u << (b & 31));
            }
            continue;
        }
        uint8_t* out = (uint8_t*)p.dst + d.dst_off;
        const uint8_t* __restrict__ z = (const uint8_t*)(ws + L.stream);
        const int64_t zchunks = (nd + CHUNK - 1) / CHUNK;
        for (int64_t ch = blockIdx.x; ch < zchunks; ch += gridDim.x) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = ch * CHUNK + 4 * tid + k;
                if (i < nd) out[FRONT + i] = z[i];
            }
        }
        if (blockIdx.x != 0) continue;
        const uint32_t* __restrict__ adler = (const uint32_t*)(ws + L.adler);
        const uint32_t* __restrict__ crc = (const uint32_t*)(ws + L.crc);
        const int64_t fchunks = (g.bytes + CHUNK - 1) / CHUNK;
        uint64_t sa = 0, sb = 0;
        uint32_t x = 0;
        for (int64_t i = tid; i < fchunks; i += 256) {
            sa += adler[2 * i];
            sb += adler[2 * i + 1];
        }
        for (int64_t i = tid; i < zchunks; i += 256) x ^= crc[i];
        red[tid] = (uint32_t)(sa % ADLER);
        red[256 + tid] = (uint32_t)(sb % ADLER);
        red[512 + tid] = x;
        __syncthreads();
        for (int step = 128; step > 0; step >>= 1) {
            if (tid < step) {
                red[tid] += red[tid + step];                  // (256 values under 65521: no overflow)
                red[256 + tid] += red[256 + tid + step];
                red[512 + tid] ^= red[512 + tid + step];
            }
            __syncthreads();
        }
        if (tid == 0) {
            const uint32_t A = (1 + red[0]) % ADLER, B = (uint32_t)((g.bytes % ADLER + red[256]) % ADLER);
            const uint32_t ad = (B << 16) | A;
            const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
            for (int i = 0; i < 8; ++i) out[i] = sig[i];
            const uint8_t ihdr[21] = {0, 0, 0, 13, 'I', 'H', 'D', 'R', (uint8_t)(d.w >> 24), (uint8_t)(d.w >> 16), (uint8_t)(d.w >> 8), (uint8_t)d.w,
                                      (uint8_t)(d.h >> 24), (uint8_t)(d.h >> 16), (uint8_t)(d.h >> 8), (uint8_t)d.h, 8, (uint8_t)(d.c == 3 ? 2 : 0), 0, 0, 0};
            uint32_t r = 0xffffffffu;
            for (int i = 0; i < 21; ++i) {
                out[8 + i] = ihdr[i];
                if (i >= 4) r = crc_byte(r, ihdr[i]);
            }
            r = ~r;
            for (int i = 0; i < 4; ++i) out[29 + i] = (uint8_t)(r >> (24 - 8 * i));
            const uint32_t len = (uint32_t)(nd + 6);
            for (int i = 0; i < 4; ++i) out[33 + i] = (uint8_t)(len >> (24 - 8 * i));
            const uint8_t idat[6] = {'I', 'D', 'A', 'T', 0x78, 0x9c};
            r = 0xffffffffu;
            for (int i = 0; i < 6; ++i) {
                out[37 + i] = idat[i];
                r = crc_byte(r, idat[i]);
            }
            r = crc_shift(r, (uint64_t)nd) ^ red[512];
            uint8_t* tail = out + FRONT + nd;
            for (int i = 0; i < 4; ++i) {
                tail[i] = (uint8_t)(ad >> (24 - 8 * i));
                r = crc_byte(r, tail[i]);
            }
            r = ~r;
            for (int i = 0; i < 4; ++i) tail[4 + i] = (uint8_t)(r >> (24 - 8 * i));
            const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
            for (int i = 0; i < 12; ++i) tail[8 + i] = iend[i];
            p.length[b] = (uint32_t)total;
        }
        __syncthreads();
    }
}

constexpr int LDS_BYTES = CODE_LDS_WORDS * 4;                // stage 3
constexpr int LDS_SMALL = 768 * 4;                           // the other stages
static_assert(LDS_BYTES <= 64 * 1024 && LDS_SMALL >= (288 + 32 + 256) * 4, "LDS of the six stages");

unsigned grid_x(int64_t units, int64_t per) {
    const int64_t bx = (units + per - 1) / per;
    return (unsigned)(bx < 1 ? 1 : (bx < MAX_X ? bx : MAX_X));
}

}  // namespace png
}  // namespace

extern "C" size_t i2i_png_workspace_bytes(int n, int64_t max_bytes) {
    if (n < 0 || max_bytes < 1 || max_bytes > png::MAX_BYTES) return 0;
    return (size_t)(png::slot_layout(max_bytes).total * n);
}

extern "C" int64_t i2i_png_bound(int w, int h, int c) {
    if (w < 1 || w > 65535 || h < 1 || h > 65535 || (c != 1 && c != 3)) return i2i::fail(I2I_ERR_BAD_ARG, "png_bound: %d x %d x %d outside 1..65535, c 1 or 3", w, h, c);
    const int64_t n = (int64_t)h * (1 + (int64_t)w * c), blocks = (n + png::BLOCK - 1) / png::BLOCK;
    return png::FRONT + (png::BLOCK_OVERHEAD_BITS * blocks + 7) / 8 + 2 * n + png::BACK;
}

extern "C" int i2i_png_encode_u8(const i2i_png_encode_u8_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: null pointer");
    if (p->n < 0) return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: n = %d < 0", p->n);
    if (p->max_bytes < 1 || p->max_bytes > png::MAX_BYTES)
        return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: max_bytes = %lld outside 1..2^27", (long long)p->max_bytes);
    if (p->src_bytes < 0 || p->dst_bytes < 0) return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: negative src_bytes / dst_bytes");
    if (p->n == 0) return I2I_OK;
    if (!p->src || !p->dst || !p->images || !p->length || !p->ws) return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: null pointer (src, dst, images, length, ws)");
    if (((uintptr_t)p->length | (uintptr_t)p->bad_mask) & 3) return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: length and bad_mask must be 4-byte aligned");
    if ((uintptr_t)p->images & 7) return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: images must be 8-byte aligned");
    if ((uintptr_t)p->ws & 15) return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: ws must be 16-byte aligned");
    const png::Slot L = png::slot_layout(p->max_bytes);
    if (p->ws_bytes < L.total * p->n)
        return i2i::fail(I2I_ERR_BAD_ARG, "png_encode_u8: ws_bytes = %lld < %lld (i2i_png_workspace_bytes)", (long long)p->ws_bytes, (long long)(L.total * p->n));
    const unsigned gy = (unsigned)(p->n < 65535 ? p->n : 65535);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned per_pos = png::grid_x(p->max_bytes, 256), per_block = png::grid_x(L.blocks, 1), per_chunk = png::grid_x(L.words * 4, png::CHUNK);
    hipLaunchKernelGGL(png::png_filter_kernel, dim3(per_pos, gy), dim3(256), png::LDS_SMALL, st, *p);
    hipLaunchKernelGGL(png::png_match_kernel, dim3(per_pos, gy), dim3(256), png::LDS_SMALL, st, *p);
    hipLaunchKernelGGL(png::png_code_kernel, dim3(per_block, gy), dim3(256), png::LDS_BYTES, st, *p);
    hipLaunchKernelGGL(png::png_pack_kernel, dim3(per_block, gy), dim3(256), png::LDS_SMALL, st, *p);
    hipLaunchKernelGGL(png::png_sum_kernel, dim3(per_chunk, gy), dim3(256), png::LDS_SMALL, st, *p);
    hipLaunchKernelGGL(png::png_emit_kernel, dim3(per_chunk, gy), dim3(256), png::LDS_SMALL, st, *p);
    return i2i::check_launch("png_encode_u8");
}

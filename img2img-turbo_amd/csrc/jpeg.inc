// Baseline JPEG encoding of a ragged uint8 batch on the device, byte-identical to Pillow with libjpeg-turbo (i2i_jpeg_encode_u8; the
// contract -- every arithmetic rule, what is device state, the safety rule -- is the comment of i2i_jpeg_image in include/i2i_turbo.h).
// Included by resize.hip, where the other uint8 boundary ops live (so both source lists, csrc/build.py and tests/emu/build_emu.py, reach it).
// The reference writes its result on the host: output_pil.save(...) (src/inference_paired.py:75, src/inference_unpaired.py:58).
//
// Five launches, grid y = image, grid x = a function of the capacity hint max_blocks only.  No kernel waits on another workgroup: both
// prefix sums (bit offsets of the blocks, stuffed bytes in front of a chunk) are two-level with a launch boundary between the levels --
// the first launch scans inside a chunk and stores the chunk's sum, the next one has every workgroup reduce the sums in front of its chunk.
//   jpeg_dct_kernel    8 lanes per 8 x 8 block, lane r owns row r, then column r: colour conversion, edge replication, h2v2 downsample,
//                      jfdctint rows, transposition through LDS, jfdctint columns, quantisation, zigzag -> int16 [block in scan order][64];
//                      also zeroes the image's bit buffer
//   jpeg_bits_kernel   a thread per block: its Huffman code length (DC predictor: the previous block of the component, dummy blocks repeat
//                      the block before them), exclusive scan over the 256 blocks of a chunk
//   jpeg_pack_kernel   a thread per block: codes it again, now at its bit offset.  A block's first and last 32-bit word may be shared with
//                      its neighbours (agent_or_u32 into zeroed words), the words between are its own (plain stores)
//   jpeg_ff_kernel     0xFF bytes per chunk of 256 words of the packed stream (its length is known on the device only)
//   jpeg_emit_kernel   header from a template (quantisation tables from the descriptor's quality, h and w patched in), the stuffed scan, EOI,
//                      length[b]; an image whose file does not fit its capacity is flagged here and nothing of it is written
// LDS of the transposition: block j of a wave at word 72 j, element (row, col) at 9 row + col.  Both the row-major store (lanes = rows, one
// column per instruction) and the column-major load hit word 72 j + 9 r + const, i.e. bank (8 (j + r) + r + const) mod 64: the 64 lanes of a
// wave land in 64 different banks.
namespace {
namespace jpg {

constexpr int HEADER = I2I_JPEG_HEADER_BYTES;
constexpr int BLOCK_WORDS = 52;                              // a block codes to at most 22 + 63 * 26 = 1660 bits
constexpr int CHUNK_BLOCKS = 256;                            // blocks per chunk of the bit-offset prefix sum (a thread each)
constexpr int CHUNK_WORDS = 256;                             // stream words per chunk of the stuffed-byte prefix sum (a thread each)
constexpr int MAX_X = 1024;                                  // workgroups per image at most
constexpr int64_t MAX_BLOCKS = (int64_t)1 << 21;             // 2^21 * 1664 bits < 2^32: bit offsets are uint32

// ITU-T T.81 Annex K.1 (natural order), the zigzag sequence (position -> natural index), Annex K.3 (BITS, HUFFVAL; luminance then chrominance)
constexpr uint8_t K1[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// (code << 8) | length by symbol, by the procedure of Annex C; the DC symbols are 0 .. 11 in order in both tables
struct HuffTab { uint32_t dc[2][16]; uint32_t ac[2][256]; };
constexpr HuffTab make_huff() {
    HuffTab t{};
    for (int k = 0; k < 2; ++k) {
        uint32_t code = 0;
        int sym = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < DC_BITS[k][len - 1]; ++i) t.dc[k][sym++] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
        code = 0;
        sym = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < AC_BITS[k][len - 1]; ++i) t.ac[k][AC_VALS[k][sym++]] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
    }
    return t;
}
constexpr HuffTab HUFF = make_huff();
constexpr int HUFF_WORDS = sizeof(HuffTab) / 4;

// the header with the bytes that depend on the image left zero: the two tables (25 .. 88, 94 .. 157), h, w (163 .. 166), Y's sampling (169)
struct HeaderTab { uint8_t b[HEADER]; };
constexpr HeaderTab make_header() {
    HeaderTab t{};
    int n = 0;
    const uint8_t app0[20] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 20; ++i) t.b[n++] = app0[i];
    for (int k = 0; k < 2; ++k) {
        const uint8_t dqt[5] = {0xff, 0xdb, 0, 67, (uint8_t)k};
        for (int i = 0; i < 5; ++i) t.b[n++] = dqt[i];
        n += 64;
    }
    const uint8_t sof[19] = {0xff, 0xc0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0, 0, 2, 0x11, 1, 3, 0x11, 1};
    for (int i = 0; i < 19; ++i) t.b[n++] = sof[i];
    for (int k = 0; k < 2; ++k) {                            // DC k, AC k
        t.b[n++] = 0xff; t.b[n++] = 0xc4; t.b[n++] = 0; t.b[n++] = 19 + 12; t.b[n++] = (uint8_t)k;
        for (int i = 0; i < 16; ++i) t.b[n++] = DC_BITS[k][i];
        for (int i = 0; i < 12; ++i) t.b[n++] = (uint8_t)i;
        t.b[n++] = 0xff; t.b[n++] = 0xc4; t.b[n++] = 0; t.b[n++] = 19 + 162; t.b[n++] = (uint8_t)(0x10 | k);
        for (int i = 0; i < 16; ++i) t.b[n++] = AC_BITS[k][i];
        for (int i = 0; i < 162; ++i) t.b[n++] = AC_VALS[k][i];
    }
    const uint8_t sos[14] = {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (int i = 0; i < 14; ++i) t.b[n++] = sos[i];
    return t;
}
constexpr HeaderTab HEADER_TEMPLATE = make_header();
static_assert(20 + 2 * 69 + 19 + 2 * (33 + 183) + 14 == HEADER, "header layout");

// entry `nat` (natural order) of quantisation table `chroma` at `quality`
__host__ __device__ __forceinline__ int quant_entry(int quality, int chroma, int nat) {
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int v = ((int)K1[chroma][nat] * s + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}

__host__ __device__ __forceinline__ uint8_t header_byte(int i, int quality, int sub, int w, int h) {
    if (i >= 25 && i < 89) return (uint8_t)quant_entry(quality, 0, ZIGZAG[i - 25]);
    if (i >= 94 && i < 158) return (uint8_t)quant_entry(quality, 1, ZIGZAG[i - 94]);
    switch (i) {
        case 163: return (uint8_t)(h >> 8);
        case 164: return (uint8_t)(h & 255);
        case 165: return (uint8_t)(w >> 8);
        case 166: return (uint8_t)(w & 255);
        case 169: return sub == 2 ? 0x22 : 0x11;
        default: return HEADER_TEMPLATE.b[i];
    }
}

// byte offsets inside an image's slot of the workspace, a function of max_blocks alone
struct Slot { int64_t coef, off, sums, stream, ff, meta, total; int64_t words, ff_chunks; };
__host__ __device__ __forceinline__ Slot slot_layout(int64_t m) {
    Slot L;
    L.coef = 0;                                              // int16 [m][64]
    L.off = m * 128;                                         // uint32 [m]: bit offset of the block inside its chunk
    L.sums = L.off + m * 4;                                  // uint32 [chunks]: bits of the chunk
    L.stream = (L.sums + (m + CHUNK_BLOCKS - 1) / CHUNK_BLOCKS * 4 + 15) & ~(int64_t)15;
    L.words = m * BLOCK_WORDS + 4;                           // (a multiple of 4)
    L.ff = L.stream + L.words * 4;                           // uint32 [ff_chunks]: 0xFF bytes of the chunk
    L.ff_chunks = (L.words + CHUNK_WORDS - 1) / CHUNK_WORDS;
    L.meta = L.ff + L.ff_chunks * 4;                         // uint32: bits of the whole scan
    L.total = (L.meta + 4 + 15) & ~(int64_t)15;
    return L;
}

// geometry of an image in blocks: MCUs, the real (not dummy) extent of Y, blocks per MCU
struct Geo { int sub2, mx, my, rbx, rby, per; int64_t nblocks; };

// Whether the descriptor may be worked on: the same verdict in every workgroup of every stage (it depends on the descriptor and the launch
// parameters only).  Sizes as quotients: no product can overflow.
__device__ __forceinline__ bool image_ok(const i2i_jpeg_encode_u8_params& p, const i2i_jpeg_image& d, Geo& g) {
    const bool ok = d.h >= 1 && d.h <= 65535 && d.w >= 1 && d.w <= 65535 && (d.c == 1 || d.c == 3) && (d.subsampling == 0 || d.subsampling == 2) &&
                    d.src_off >= 0 && d.src_off <= p.src_bytes && d.dst_off >= 0 && d.dst_off <= p.dst_bytes && d.capacity >= 0 &&
                    d.capacity <= p.dst_bytes - d.dst_off;
    if (!ok) return false;
    if ((int64_t)d.h * d.w > (p.src_bytes - d.src_off) / d.c) return false;
    g.sub2 = d.subsampling == 2;
    g.rbx = (d.w + 7) >> 3;
    g.rby = (d.h + 7) >> 3;
    g.mx = g.sub2 ? (d.w + 15) >> 4 : g.rbx;
    g.my = g.sub2 ? (d.h + 15) >> 4 : g.rby;
    g.per = g.sub2 ? 6 : 3;
    g.nblocks = (int64_t)g.mx * g.my * g.per;
    return g.nblocks <= p.max_blocks;
}

// block s of the scan -> its MCU and its place in it
struct Where { int64_t m; int k, comp, by, bx; bool dummy; };
__device__ __forceinline__ Where where(const Geo& g, int64_t s) {
    Where q;
    q.m = s / g.per;
    q.k = (int)(s - q.m * g.per);
    const int my = (int)(q.m / g.mx), mx = (int)(q.m - (int64_t)my * g.mx);
    if (g.sub2 && q.k < 4) {
        q.comp = 0;
        q.by = 2 * my + (q.k >> 1);
        q.bx = 2 * mx + (q.k & 1);
        q.dummy = q.by >= g.rby || q.bx >= g.rbx;
    } else {
        q.comp = g.sub2 ? q.k - 3 : q.k;
        q.by = my;
        q.bx = mx;
        q.dummy = false;
    }
    return q;
}

// ------------------------------------------------------------------------------------------------------------------------ stage 1
// 8 pixels of row y from column x0 on, columns past the image replicate its last one.  Whole groups inside the row are read as seven
// aligned dwords (the arena base is 4-byte aligned; the read may run up to 4 bytes past the group, never past the arena), the rest bytewise.
__device__ __forceinline__ void fetch8(const uint8_t* __restrict__ base, int64_t src_bytes, const i2i_jpeg_image& d, int y, int x0, int (&r)[8], int (&g)[8],
                                       int (&b)[8]) {
    if (d.c == 3 && x0 + 8 <= d.w) {
        const int64_t a = d.src_off + ((int64_t)y * d.w + x0) * 3, a0 = a & ~(int64_t)3;
        if (a0 + 28 <= src_bytes) {
            const uint32_t* __restrict__ q = (const uint32_t*)(base + a0);
            const int sh = 8 * (int)(a & 3);
            uint32_t v[7], u[6];
#pragma unroll
            for (int j = 0; j < 7; ++j) v[j] = q[j];
#pragma unroll
            for (int j = 0; j < 6; ++j) u[j] = sh ? (v[j] >> sh) | (v[j + 1] << (32 - sh)) : v[j];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                r[i] = (int)((u[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255);
                g[i] = (int)((u[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255);
                b[i] = (int)((u[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255);
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int x = x0 + i < d.w ? x0 + i : d.w - 1;
        const int64_t a = d.src_off + ((int64_t)y * d.w + x) * d.c;
        r[i] = base[a];
        g[i] = d.c == 3 ? base[a + 1] : r[i];
        b[i] = d.c == 3 ? base[a + 2] : r[i];
    }
}

// component `comp` of a pixel, libjpeg's rgb_ycc_convert
__device__ __forceinline__ int ycc(int comp, int r, int g, int b) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2), in place; FIRST: the row pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    constexpr int N = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2] = descale(z1 + t13 * 6270, N);
    d[6] = descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = descale(u4 + z1 + z3, N);
    d[5] = descale(u5 + z2 + z4, N);
    d[3] = descale(u6 + z2 + z3, N);
    d[1] = descale(u7 + z1 + z4, N);
}

// samples - 128 of row r of block q (not a dummy block)
__device__ __forceinline__ void block_row(const i2i_jpeg_encode_u8_params& p, const i2i_jpeg_image& d, const Geo& g, const Where& q, int r, int (&v)[8]) {
    const uint8_t* __restrict__ base = (const uint8_t*)p.src;
    int R[8], G[8], B[8];
    if (q.comp == 0 || !g.sub2) {
        const int y = q.by * 8 + r < d.h ? q.by * 8 + r : d.h - 1;
        fetch8(base, p.src_bytes, d, y, q.bx * 8, R, G, B);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ycc(q.comp, R[i], G[i], B[i]) - 128;
    } else {                                                 // h2v2: the downsampled plane has ceil(h / 2) rows, its last one is replicated
        const int ch = (d.h + 1) >> 1;
        const int cy = q.by * 8 + r < ch ? q.by * 8 + r : ch - 1;
        const int y0 = 2 * cy, y1 = 2 * cy + 1 < d.h ? 2 * cy + 1 : d.h - 1;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            int s[8];
            fetch8(base, p.src_bytes, d, y0, q.bx * 16 + 8 * half, R, G, B);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] = ycc(q.comp, R[i], G[i], B[i]);
            fetch8(base, p.src_bytes, d, y1, q.bx * 16 + 8 * half, R, G, B);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] += ycc(q.comp, R[i], G[i], B[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * half + j] = ((s[2 * j] + s[2 * j + 1] + 1 + (j & 1)) >> 2) - 128;
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_dct_kernel(const i2i_jpeg_encode_u8_params p) {
    const int tid = (int)threadIdx.x, r = tid & 7;
    int32_t* blk = (int32_t*)i2i_smem + (tid >> 3) * 72;
    const Slot L = slot_layout(p.max_blocks);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_jpeg_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) {
            if (p.bad_mask && blockIdx.x == 0 && tid == 0) agent_or_u32(p.bad_mask, 1u << (b & 31));
            continue;
        }
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        u32x4* zero = (u32x4*)(ws + L.stream);
        const int64_t nzero = (g.nblocks * BLOCK_WORDS + 4) / 4;
        for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < nzero; i += (int64_t)gridDim.x * 256) zero[i] = u32x4{0, 0, 0, 0};
        int16_t* coef = (int16_t*)(ws + L.coef);
        for (int64_t s0 = (int64_t)blockIdx.x * 32; s0 < g.nblocks; s0 += (int64_t)gridDim.x * 32) {
            const int64_t s = s0 + (tid >> 3);
            const bool live = s < g.nblocks;
            const Where q = where(g, live ? s : 0);
            int v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0;
            if (live && !q.dummy) block_row(p, d, g, q, r, v);
            fdct8<true>(v);
#pragma unroll
            for (int i = 0; i < 8; ++i) blk[9 * r + i] = v[i];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = blk[9 * i + r];  // column r
            fdct8<false>(v);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int dq = 8 * quant_entry(d.quality, q.comp > 0, 8 * i + r);
                const int a = v[i] < 0 ? -v[i] : v[i];
                const int m = (a + (dq >> 1)) / dq;
                v[i] = v[i] < 0 ? -m : m;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) blk[9 * i + r] = v[i];
            __syncthreads();
            uint32_t w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {                    // zigzag positions 8 r .. 8 r + 7
                const int n0 = ZIGZAG[8 * r + 2 * i], n1 = ZIGZAG[8 * r + 2 * i + 1];
                w[i] = ((uint32_t)blk[9 * (n0 >> 3) + (n0 & 7)] & 0xffffu) | ((uint32_t)blk[9 * (n1 >> 3) + (n1 & 7)] << 16);
            }
            if (live) *(u32x4*)(coef + s * 64 + 8 * r) = q.dummy ? u32x4{0, 0, 0, 0} : u32x4{w[0], w[1], w[2], w[3]};
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ stages 2 and 3
// the DC a block contributes to the predictor chain: its own, or for a dummy block that of the block before it in the MCU (block 0 of an
// MCU is never a dummy)
__device__ __forceinline__ int chain_dc(const int16_t* __restrict__ coef, const Geo& g, int64_t s) {
    Where q = where(g, s);
    while (q.dummy) q = where(g, --s);
    return coef[s * 64];
}

// DC difference of block s: against the previous block of its component
__device__ __forceinline__ int dc_diff(const int16_t* __restrict__ coef, const Geo& g, int64_t s, const Where& q) {
    if (q.dummy) return 0;
    int pred = 0;
    if (g.sub2 && q.comp == 0) {
        if (q.k > 0) pred = chain_dc(coef, g, s - 1);
        else if (q.m > 0) pred = chain_dc(coef, g, s - 3);    // Y11 of the MCU before
    } else if (q.m > 0) {
        pred = coef[(s - g.per) * 64];
    }
    return (int)coef[s * 64] - pred;
}

__device__ __forceinline__ int bit_length(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

// MSB-first bit writer into 32-bit words: the word the block starts in (if it does not start on a word boundary) and the word it ends in are
// shared with its neighbours and OR-ed into the zeroed buffer, the words between are the block's own
struct BitSink { uint32_t* words; uint64_t acc; int n; bool shared; };
template <bool WRITE>
__device__ __forceinline__ void put(BitSink& s, uint32_t code, int len) {
    if (!WRITE) return;
    s.acc = (s.acc << len) | code;
    s.n += len;
    if (s.n >= 32) {
        s.n -= 32;
        const uint32_t w = (uint32_t)(s.acc >> s.n);
        if (s.shared) agent_or_u32(s.words, w);
        else *s.words = w;
        s.shared = false;
        ++s.words;
        s.acc &= ((uint64_t)1 << s.n) - 1;
    }
}

// Codes one block (64 coefficients in zigzag order, 16-byte aligned; `diff` replaces the DC) with table set t: returns its length in bits and,
// with WRITE, appends the bits to the sink.  huff: the HuffTab in LDS.
template <bool WRITE>
__device__ __forceinline__ uint32_t code_block(const int16_t* __restrict__ c, int diff, int t, const uint32_t* __restrict__ huff, BitSink& s) {
    const uint32_t* __restrict__ dc = huff + 16 * t;
    const uint32_t* __restrict__ ac = huff + 32 + 256 * t;
    uint32_t bits = 0;
    {
        int n = bit_length(diff < 0 ? -diff : diff);
        n = n < 11 ? n : 11;                                 // (8-bit samples never exceed category 11; the clamp keeps the 1660-bit bound unconditional)
        const uint32_t e = dc[n];
        bits += (e & 255) + n;
        put<WRITE>(s, e >> 8, (int)(e & 255));
        if (n) put<WRITE>(s, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1), n);
    }
    int run = 0;
    for (int k8 = 0; k8 < 8; ++k8) {
        const u32x4 w = *(const u32x4*)(c + 8 * k8);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (k8 == 0 && i == 0) continue;
            const int v = (int)(int16_t)(w[i >> 1] >> (16 * (i & 1)));
            if (v == 0) {
                ++run;
                continue;
            }
            while (run >= 16) {
                const uint32_t z = ac[0xf0];
                bits += z & 255;
                put<WRITE>(s, z >> 8, (int)(z & 255));
                run -= 16;
            }
            int n = bit_length(v < 0 ? -v : v);
            n = n < 10 ? n : 10;                             // (likewise: category 10 at most)
            const uint32_t e = ac[(run << 4) | n];
            bits += (e & 255) + n;
            put<WRITE>(s, e >> 8, (int)(e & 255));
            put<WRITE>(s, (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1), n);
            run = 0;
        }
    }
    if (run > 0) {
        const uint32_t e = ac[0];
        bits += e & 255;
        put<WRITE>(s, e >> 8, (int)(e & 255));
    }
    return bits;
}

// the Huffman tables into LDS words [0, HUFF_WORDS) (all 256 threads; the caller's next barrier publishes them)
__device__ __forceinline__ void load_huff(uint32_t* lds) {
    for (int i = (int)threadIdx.x; i < HUFF_WORDS; i += 256) lds[i] = i < 32 ? HUFF.dc[i >> 4][i & 15] : HUFF.ac[(i - 32) >> 8][(i - 32) & 255];
}

__global__ __launch_bounds__(256) void jpeg_bits_kernel(const i2i_jpeg_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    uint32_t* huff = (uint32_t*)i2i_smem;
    uint32_t* scan = huff + HUFF_WORDS;                      // [256]
    load_huff(huff);
    __syncthreads();
    const Slot L = slot_layout(p.max_blocks);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_jpeg_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) continue;
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const int16_t* __restrict__ coef = (const int16_t*)(ws + L.coef);
        uint32_t* off = (uint32_t*)(ws + L.off);
        uint32_t* sums = (uint32_t*)(ws + L.sums);
        const int64_t chunks = (g.nblocks + CHUNK_BLOCKS - 1) / CHUNK_BLOCKS;
        for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
            const int64_t s = ch * CHUNK_BLOCKS + tid;
            uint32_t bits = 0;
            if (s < g.nblocks) {
                const Where q = where(g, s);
                BitSink none = {nullptr, 0, 0, false};
                bits = code_block<false>(coef + s * 64, dc_diff(coef, g, s, q), q.comp > 0, huff, none);
            }
            scan[tid] = bits;
            __syncthreads();
            for (int step = 1; step < 256; step <<= 1) {     // inclusive scan over the chunk
                const uint32_t add = tid >= step ? scan[tid - step] : 0;
                __syncthreads();
                scan[tid] += add;
                __syncthreads();
            }
            if (s < g.nblocks) off[s] = scan[tid] - bits;
            if (tid == 255) sums[ch] = scan[255];
            __syncthreads();
        }
    }
}

// sum of v[0 .. n) and of v[0 .. k) over the workgroup (all 256 threads; red: 512 LDS words); returns {whole, front}
__device__ __forceinline__ void reduce2(const uint32_t* __restrict__ v, int64_t n, int64_t k, uint32_t* red, uint32_t& whole, uint32_t& front) {
    const int tid = (int)threadIdx.x;
    uint32_t a = 0, f = 0;
    for (int64_t i = tid; i < n; i += 256) {
        const uint32_t x = v[i];
        a += x;
        if (i < k) f += x;
    }
    red[tid] = a;
    red[256 + tid] = f;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) {
            red[tid] += red[tid + step];
            red[256 + tid] += red[256 + tid + step];
        }
        __syncthreads();
    }
    whole = red[0];
    front = red[256];
    __syncthreads();
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const i2i_jpeg_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    uint32_t* huff = (uint32_t*)i2i_smem;
    uint32_t* red = huff + HUFF_WORDS;                       // [512]
    load_huff(huff);
    __syncthreads();
    const Slot L = slot_layout(p.max_blocks);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_jpeg_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) continue;
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const int16_t* __restrict__ coef = (const int16_t*)(ws + L.coef);
        const uint32_t* __restrict__ off = (const uint32_t*)(ws + L.off);
        const uint32_t* __restrict__ sums = (const uint32_t*)(ws + L.sums);
        uint32_t* stream = (uint32_t*)(ws + L.stream);
        const int64_t chunks = (g.nblocks + CHUNK_BLOCKS - 1) / CHUNK_BLOCKS;
        for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
            uint32_t whole, front;                            // the second level: the bits in front of this chunk
            reduce2(sums, chunks, ch, red, whole, front);
            const int64_t s = ch * CHUNK_BLOCKS + tid;
            if (s < g.nblocks) {
                const Where q = where(g, s);
                const uint32_t at = front + off[s];
                BitSink sink = {stream + (at >> 5), 0, (int)(at & 31), (at & 31) != 0};
                const uint32_t bits = code_block<true>(coef + s * 64, dc_diff(coef, g, s, q), q.comp > 0, huff, sink);
                if (sink.n > 0) agent_or_u32(sink.words, (uint32_t)(sink.acc << (32 - sink.n)));
                if (s == g.nblocks - 1) *(uint32_t*)(ws + L.meta) = at + bits;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ stages 4 and 5
// the packed stream as the last two stages see it: `bytes` bytes, the last one padded with 1-bits
struct Stream { const uint32_t* words; int64_t bytes; uint32_t pad; };
__device__ __forceinline__ Stream stream_of(const char* ws, const Slot& L, const Geo& g) {
    uint32_t bits = *(const uint32_t*)(ws + L.meta);
    const uint32_t most = (uint32_t)(g.nblocks * (BLOCK_WORDS * 32));
    bits = bits < most ? bits : most;                         // (what stage 3 wrote; never more than the buffer holds)
    Stream t;
    t.words = (const uint32_t*)(ws + L.stream);
    t.bytes = ((int64_t)bits + 7) >> 3;
    t.pad = (1u << (8 * t.bytes - bits)) - 1;
    return t;
}
// the four bytes of word i in stream order; bytes past the end read as 0 (never 0xFF)
__device__ __forceinline__ uint32_t stream_word(const Stream& t, int64_t i) {
    if (4 * i >= t.bytes) return 0;
    uint32_t w = t.words[i];
    const int64_t last = t.bytes - 1;
    if ((last >> 2) == i) {
        const int sh = 24 - 8 * (int)(last & 3);
        w = (w | (t.pad << sh)) & ~((1u << sh) - 1);
    }
    return w;
}
__device__ __forceinline__ uint32_t count_ff(uint32_t w) {
    return (uint32_t)((w >> 24) == 255) + (uint32_t)(((w >> 16) & 255) == 255) + (uint32_t)(((w >> 8) & 255) == 255) + (uint32_t)((w & 255) == 255);
}

__global__ __launch_bounds__(256) void jpeg_ff_kernel(const i2i_jpeg_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    uint32_t* red = (uint32_t*)i2i_smem;                     // [256]
    const Slot L = slot_layout(p.max_blocks);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_jpeg_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) continue;
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const Stream t = stream_of(ws, L, g);
        uint32_t* ff = (uint32_t*)(ws + L.ff);
        const int64_t chunks = (t.bytes + 4 * CHUNK_WORDS - 1) / (4 * CHUNK_WORDS);
        for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
            red[tid] = count_ff(stream_word(t, ch * CHUNK_WORDS + tid));
            __syncthreads();
            for (int step = 128; step > 0; step >>= 1) {
                if (tid < step) red[tid] += red[tid + step];
                __syncthreads();
            }
            if (tid == 0) ff[ch] = red[0];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_emit_kernel(const i2i_jpeg_encode_u8_params p) {
    const int tid = (int)threadIdx.x;
    uint32_t* red = (uint32_t*)i2i_smem;                     // [512]
    uint32_t* scan = red + 512;                              // [256]
    const Slot L = slot_layout(p.max_blocks);
    for (int b = (int)blockIdx.y; b < p.n; b += (int)gridDim.y) {
        const i2i_jpeg_image d = p.images[b];
        Geo g;
        if (!image_ok(p, d, g)) {                            // (flagged by stage 1)
            if (blockIdx.x == 0 && tid == 0) p.length[b] = 0;
            continue;
        }
        char* ws = (char*)p.ws + (int64_t)b * L.total;
        const Stream t = stream_of(ws, L, g);
        const uint32_t* __restrict__ ff = (const uint32_t*)(ws + L.ff);
        const int64_t chunks = (t.bytes + 4 * CHUNK_WORDS - 1) / (4 * CHUNK_WORDS);
        uint32_t stuffed, front;
        reduce2(ff, chunks, 0, red, stuffed, front);
        const int64_t total = HEADER + t.bytes + stuffed + 2;
        if (total > d.capacity) {                            // the same verdict in every workgroup of the image: nothing is written
            if (blockIdx.x == 0 && tid == 0) {
                p.length[b] = 0;
                if (p.bad_mask) agent_or_u32(p.bad_mask, 1u << (b & 31));
            }
            continue;
        }
        uint8_t* out = (uint8_t*)p.dst + d.dst_off;
        if (blockIdx.x == 0) {
            for (int i = tid; i < HEADER; i += 256) out[i] = header_byte(i, d.quality, d.subsampling, d.w, d.h);
            if (tid == 0) {
                out[total - 2] = 0xff;
                out[total - 1] = 0xd9;
                p.length[b] = (uint32_t)total;
            }
        }
        for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
            reduce2(ff, chunks, ch, red, stuffed, front);     // the second level: the stuffed bytes in front of this chunk
            const int64_t i = ch * CHUNK_WORDS + tid;
            const uint32_t w = stream_word(t, i);
            const uint32_t mine = count_ff(w);
            scan[tid] = mine;
            __syncthreads();
            for (int step = 1; step < 256; step <<= 1) {
                const uint32_t add = tid >= step ? scan[tid - step] : 0;
                __syncthreads();
                scan[tid] += add;
                __syncthreads();
            }
            int64_t at = HEADER + 4 * i + front + (scan[tid] - mine);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (4 * i + k < t.bytes) {
                    const uint8_t v = (uint8_t)(w >> (24 - 8 * k));
                    out[at++] = v;
                    if (v == 255) out[at++] = 0;
                }
            }
        }
    }
}

constexpr int LDS_BYTES = 32 * 72 * 4;                       // the largest of the five kernels' needs: stage 1, 32 blocks of 72 words
static_assert(LDS_BYTES >= (HUFF_WORDS + 768) * 4, "LDS of stages 2 .. 5");

unsigned grid_x(int64_t units, int64_t per) {
    const int64_t bx = (units + per - 1) / per;
    return (unsigned)(bx < 1 ? 1 : (bx < MAX_X ? bx : MAX_X));
}

}  // namespace jpg
}  // namespace

extern "C" size_t i2i_jpeg_workspace_bytes(int n, int64_t max_blocks) {
    if (n < 0 || max_blocks < 1 || max_blocks > jpg::MAX_BLOCKS) return 0;
    return (size_t)(jpg::slot_layout(max_blocks).total * n);
}

extern "C" int i2i_jpeg_header(int quality, int subsampling, int w, int h, uint8_t* out) {
    if (!out) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_header: null pointer");
    if (subsampling != 0 && subsampling != 2) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_header: subsampling = %d (0 = 4:4:4, 2 = 4:2:0)", subsampling);
    if (w < 1 || w > 65535 || h < 1 || h > 65535) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_header: extent %d x %d outside 1..65535", w, h);
    for (int i = 0; i < jpg::HEADER; ++i) out[i] = jpg::header_byte(i, quality, subsampling, w, h);
    return jpg::HEADER;
}

extern "C" int i2i_jpeg_encode_u8(const i2i_jpeg_encode_u8_params* p, int dtype, void* stream) {
    (void)dtype;
    if (!p) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: null pointer");
    if (p->n < 0) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: n = %d < 0", p->n);
    if (p->max_blocks < 1 || p->max_blocks > jpg::MAX_BLOCKS)
        return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: max_blocks = %lld outside 1..2^21", (long long)p->max_blocks);
    if (p->src_bytes < 0 || p->dst_bytes < 0) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: negative src_bytes / dst_bytes");
    if (p->n == 0) return I2I_OK;
    if (!p->src || !p->dst || !p->images || !p->length || !p->ws) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: null pointer (src, dst, images, length, ws)");
    if (((uintptr_t)p->src | (uintptr_t)p->length | (uintptr_t)p->bad_mask) & 3)
        return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: src, length and bad_mask must be 4-byte aligned");
    if ((uintptr_t)p->images & 7) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: images must be 8-byte aligned");
    if ((uintptr_t)p->ws & 15) return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: ws must be 16-byte aligned");
    const jpg::Slot L = jpg::slot_layout(p->max_blocks);
    if (p->ws_bytes < L.total * p->n)
        return i2i::fail(I2I_ERR_BAD_ARG, "jpeg_encode_u8: ws_bytes = %lld < %lld (i2i_jpeg_workspace_bytes)", (long long)p->ws_bytes, (long long)(L.total * p->n));
    const unsigned gy = (unsigned)(p->n < 65535 ? p->n : 65535);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned per_chunk = jpg::grid_x(p->max_blocks, jpg::CHUNK_BLOCKS), per_words = jpg::grid_x(L.words, jpg::CHUNK_WORDS);
    hipLaunchKernelGGL(jpg::jpeg_dct_kernel, dim3(jpg::grid_x(p->max_blocks, 32), gy), dim3(256), jpg::LDS_BYTES, st, *p);
    hipLaunchKernelGGL(jpg::jpeg_bits_kernel, dim3(per_chunk, gy), dim3(256), jpg::LDS_BYTES, st, *p);
    hipLaunchKernelGGL(jpg::jpeg_pack_kernel, dim3(per_chunk, gy), dim3(256), jpg::LDS_BYTES, st, *p);
    hipLaunchKernelGGL(jpg::jpeg_ff_kernel, dim3(per_words, gy), dim3(256), jpg::LDS_BYTES, st, *p);
    hipLaunchKernelGGL(jpg::jpeg_emit_kernel, dim3(per_words, gy), dim3(256), jpg::LDS_BYTES, st, *p);
    return i2i::check_launch("jpeg_encode_u8");
}

"""Baseline JPEG encoder in integer numpy: the oracle of i2i_jpeg_encode_u8 (csrc/jpeg.inc; the contract is the comment of i2i_jpeg_image in
include/i2i_turbo.h).  ``encode(img, quality, subsampling)`` returns the complete file, byte for byte what Pillow with libjpeg-turbo writes for
``Image.fromarray(img).save(f, "JPEG", quality=q, subsampling=s)``: one interleaved baseline scan, the typical Huffman tables of the JPEG
standard (ITU-T T.81 Annex K.3), the Annex K.1 quantisation tables scaled the libjpeg way, libjpeg's integer colour conversion, h2v2
downsampling and "islow" forward DCT.  tests/test_jpeg_emu.py::test_oracle_matches_pillow pins it against the installed Pillow.

Everything is integer arithmetic; no tolerance exists anywhere.  ``parts()`` returns the header and the scan separately, ``stats()`` what the
tests assert about a case (stuffed bytes, ZRL symbols)."""
import numpy as np

# ITU-T T.81 Annex K.1, natural (row-major) order
K1_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K1_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# zigzag position -> natural index
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# ITU-T T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL of the four typical tables
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HEADER_BYTES = 623
SUBSAMPLINGS = {"4:4:4": 0, "4:2:0": 2, 0: 0, 2: 2}


def _codes(bits, vals):
    """{symbol: (code, length)} by the procedure of Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (_codes(*DC_LUMA), _codes(*DC_CHROMA))
AC_CODES = (_codes(*AC_LUMA), _codes(*AC_CHROMA))


def quant_tables(quality):
    """(luma, chroma) int arrays [64] in natural order."""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(t, dtype=np.int64) * s + 50) // 100, 1, 255) for t in (K1_LUMA, K1_CHROMA))


def header(quality, subsampling, w, h):
    """The 623 bytes in front of the scan."""
    sub = SUBSAMPLINGS[subsampling]
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate(quant_tables(quality)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(t[z]) for z in ZIGZAG)
    out += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22 if sub == 2 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls_id, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += b"\xff\xc4" + bytes([0, 19 + len(vals), cls_id]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One 1-D pass of jfdctint over the last axis of ``d`` (int64 [..., 8])."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def _blocks(plane):
    """int64 [8 * by, 8 * bx] samples -> DCT coefficients [by, bx, 8, 8] (unquantised)."""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128
    b = _fdct_pass(b, True)                                   # rows
    return _fdct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns


def _pad(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def coefficients(img, subsampling):
    """The unquantised DCT coefficients of the three components and the geometry: (Y, Cb, Cr) as [by, bx, 8, 8], (mcus_y, mcus_x)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    if img.shape[2] == 1:
        img = np.repeat(img, 3, axis=2)
    assert img.dtype == np.uint8 and img.shape[2] == 3
    h, w = img.shape[:2]
    r, g, b = (img[:, :, i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if SUBSAMPLINGS[subsampling] == 0:
        my, mx = -(-h // 8), -(-w // 8)
        return tuple(_blocks(_pad(p, 8 * my, 8 * mx)) for p in (y, cb, cr)), (my, mx)
    my, mx = -(-h // 16), -(-w // 16)
    planes = [_blocks(_pad(y, 16 * my, 16 * mx))]
    bias = np.tile(np.array([1, 2], dtype=np.int64), 4 * mx)
    for p in (cb, cr):
        p = _pad(p, h + (h & 1), 16 * mx)                       # columns in the input domain, rows to an even height
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias[None, :]) >> 2
        planes.append(_blocks(_pad(d, 8 * my, 8 * mx)))          # the DOWNSAMPLED plane's last row is what gets replicated
    return tuple(planes), (my, mx)


def _quantise(c, q):
    d = 8 * q.reshape(8, 8)
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out, self.zrl = 0, 0, bytearray(), 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _value_bits(v):
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def _code_block(bits, zz, pred, t):
    """One block of 64 quantised coefficients in zigzag order."""
    n, extra = _value_bits(zz[0] - pred)
    bits.put(*DC_CODES[t][n])
    if n:
        bits.put(extra, n)
    ac = AC_CODES[t]
    last = 0
    for k in (np.flatnonzero(zz[1:]) + 1).tolist():
        run = k - last - 1
        while run >= 16:
            bits.put(*ac[0xF0])
            bits.zrl += 1
            run -= 16
        n, extra = _value_bits(int(zz[k]))
        bits.put(*ac[(run << 4) | n])
        bits.put(extra, n)
        last = k
    if last != 63:
        bits.put(*ac[0x00])


def scan(img, quality, subsampling):
    """(the packed entropy-coded stream before byte stuffing, with the 1-padding of its last byte; number of ZRL symbols)."""
    (yc, cbc, crc), (my, mx) = coefficients(img, subsampling)
    h, w = np.asarray(img).shape[:2]
    ql, qc = quant_tables(quality)
    zig = np.array(ZIGZAG)
    comps = [_quantise(yc, ql).reshape(yc.shape[0], yc.shape[1], 64)[:, :, zig], _quantise(cbc, qc).reshape(my, mx, 64)[:, :, zig],
             _quantise(crc, qc).reshape(my, mx, 64)[:, :, zig]]
    bits, pred = _Bits(), [0, 0, 0]
    sub2 = SUBSAMPLINGS[subsampling] == 2
    real_by, real_bx = -(-h // 8), -(-w // 8)
    for m_y in range(my):
        for m_x in range(mx):
            ys = [(2 * m_y + dy, 2 * m_x + dx) for dy in (0, 1) for dx in (0, 1)] if sub2 else [(m_y, m_x)]
            prev_dc = 0
            for by, bx in ys:
                if by >= real_by or bx >= real_bx:             # a dummy block: no AC, the DC of the block before it in this MCU
                    zz = np.zeros(64, dtype=np.int64)
                    zz[0] = prev_dc
                else:
                    zz = comps[0][by, bx]
                _code_block(bits, zz, pred[0], 0)
                pred[0] = prev_dc = int(zz[0])
            for c in (1, 2):
                zz = comps[c][m_y, m_x]
                _code_block(bits, zz, pred[c], 1)
                pred[c] = int(zz[0])
    return bits.finish(), bits.zrl


def parts(img, quality=75, subsampling="4:2:0"):
    """(header, the stuffed scan, EOI)."""
    h, w = np.asarray(img).shape[:2]
    raw, _ = scan(img, quality, subsampling)
    return header(quality, subsampling, w, h), raw.replace(b"\xff", b"\xff\x00"), b"\xff\xd9"


def encode(img, quality=75, subsampling="4:2:0"):
    return b"".join(parts(img, quality, subsampling))


def stats(img, quality=75, subsampling="4:2:0"):
    """What the tests assert about a case: dict(raw = unstuffed scan bytes, stuffed = positions in the raw stream of its 0xFF bytes, zrl)."""
    raw, zrl = scan(img, quality, subsampling)
    return dict(raw=len(raw), stuffed=[i for i, b in enumerate(raw) if b == 255], zrl=zrl)

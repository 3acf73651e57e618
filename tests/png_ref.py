"""Integer oracle of i2i_png_encode_u8 (csrc/png.inc; the contract is the comment of i2i_png_image in include/i2i_turbo.h): the PNG file
the device writes for one uint8 image, byte for byte.  Container and filtered scanline stream are Pillow's (ZipEncode.c, ZIP_PNG without
optimize); the deflate stream is this project's own, fully specified by the contract and restated here step by step:

  filter   per row None / Up / Sub / Paeth by Pillow's rule: cost = sum(min(v, 256 - v)), start with None, then while the best cost is > 0
           try Up, Sub, Paeth in this order and take one only if strictly cheaper.  bpp = c, the row above row 0 is zeros.
  blocks   the filtered stream F (h rows of 1 + w c bytes) is cut every BLOCK = 16384 bytes; every piece is one BTYPE = 2 block.
  matches  position p looks at the distances 1, c, S, S - c, S + c (S = 1 + w c) in this order; a distance > 32768 or > p is dropped; the
           length is the run of equal bytes F[p + k] == F[p + k - d], at most 258, clipped at the end of p's block; the longest wins, ties
           go to the first; under 3 the position is a literal.  The parse is greedy from the block's first byte.
  lengths  code_lengths(): the used symbols sorted by (frequency, symbol); Huffman's two-queue merge (a leaf is taken before an internal
           node of equal weight); depths clipped at the limit; while the Kraft sum exceeds 1: the deepest leaf above the limit row moves
           one down and takes one leaf of the limit row as its brother; then the lengths are dealt by sorted order, longest to rarest.
           No used symbol: all zero (HDIST = 0 with one length of zero); one used symbol: length 1.
  header   HLIT / HDIST cut trailing zeros (at least 257 / 1), the two length lists are run-length coded as ONE sequence: zeros by 18
           (11 .. 138) while >= 11, then 17 (3 .. 10), then single zeros; a length v once, then 16 (3 .. 6) while >= 3 remain, then singles.
  bits     LSB first, Huffman codes bit-reversed, extra bits as they are; BFINAL on the last block; zero bits up to the byte boundary.
"""
import struct
import zlib

import numpy as np

BLOCK = 16384
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CANDIDATES = 5


def _hwc(a, invert):
    a = np.asarray(a)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] in (1, 3), (a.dtype, a.shape)
    return (255 - a) if invert else a


def filtered(a, invert=False):
    """(F as uint8 [h * (1 + w c)], the filter type of every row)."""
    a = _hwc(a, invert)
    h, w, c = a.shape
    raw = a.reshape(h, w * c).astype(np.int32)
    up = np.vstack([np.zeros((1, w * c), np.int32), raw[:-1]])
    left = np.hstack([np.zeros((h, c), np.int32), raw[:, :-c]]) if w > 1 else np.zeros_like(raw)
    ul = np.hstack([np.zeros((h, c), np.int32), up[:, :-c]]) if w > 1 else np.zeros_like(raw)
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    rows = {0: raw, 2: (raw - up) & 255, 1: (raw - left) & 255, 4: (raw - pred) & 255}
    cost = {t: np.where(f < 128, f, 256 - f).sum(axis=1) for t, f in rows.items()}
    out = np.zeros((h, 1 + w * c), np.uint8)
    types = []
    for y in range(h):
        best, bc = 0, int(cost[0][y])
        for t in (2, 1, 4):
            if bc > 0 and int(cost[t][y]) < bc:
                best, bc = t, int(cost[t][y])
        out[y, 0] = best
        out[y, 1:] = rows[best][y]
        types.append(best)
    return out.reshape(-1), types


def distances(w, c):
    s = 1 + w * c
    return [1, c, s, s - c, s + c]


def matches(F, w, c):
    """(length [n] (0: literal), candidate index [n]) of every position of F."""
    n = F.size
    pos = np.arange(n, dtype=np.int64)
    room = np.minimum(258, (pos // BLOCK + 1) * BLOCK - pos)
    room = np.minimum(room, n - pos)
    best = np.zeros(n, np.int64)
    cand = np.zeros(n, np.int64)
    for k, d in enumerate(distances(w, c)):
        if d > 32768 or d >= n + 1 or d < 1:
            continue
        diff = np.ones(n, bool)                                  # positions with p < d have no such candidate
        diff[d:] = F[d:] != F[:-d] if d < n else np.ones(0, bool)
        nxt = np.where(diff, pos, n)                             # the next mismatch at or behind p
        nxt = np.minimum.accumulate(nxt[::-1])[::-1]
        length = np.minimum(nxt - pos, room)
        take = length > best
        cand[take] = k
        best[take] = length[take]
    best[best < 3] = 0
    cand[best == 0] = 0
    return best, cand


def len_symbol(length):
    k = max(i for i in range(29) if LBASE[i] <= length)
    return 257 + k, length - LBASE[k], LEXTRA[k]


def dist_symbol(d):
    k = max(i for i in range(30) if DBASE[i] <= d)
    return k, d - DBASE[k], DEXTRA[k]


def code_lengths(freq, limit):
    """(the code length of every symbol, whether the length-limit repair ran)."""
    used = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    n = len(used)
    lens = [0] * len(freq)
    if n == 0:
        return lens, False
    if n == 1:
        lens[used[0][1]] = 1
        return lens, False
    leaf = [f for f, _ in used]
    node, leaf_parent, node_parent = [], [0] * n, [0] * (n - 1)
    i = j = 0
    for k in range(n - 1):
        wsum = 0
        for _ in range(2):
            if i < n and (j >= len(node) or leaf[i] <= node[j]):
                wsum += leaf[i]
                leaf_parent[i] = k
                i += 1
            else:
                wsum += node[j]
                node_parent[j] = k
                j += 1
        node.append(wsum)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    count = [0] * (limit + 1)
    for x in range(n):
        count[min(depth[leaf_parent[x]] + 1, limit)] += 1
    excess = sum(count[l] << (limit - l) for l in range(1, limit + 1)) - (1 << limit)
    assert excess >= 0
    for _ in range(excess):
        l = max(x for x in range(1, limit) if count[x] > 0)
        count[l] -= 1
        count[l + 1] += 2
        count[limit] -= 1
        assert count[limit] >= 0
    assert sum(count[l] << (limit - l) for l in range(1, limit + 1)) == 1 << limit and sum(count) == n
    r = 0
    for l in range(limit, 0, -1):
        for _ in range(count[l]):
            lens[used[r][1]] = l
            r += 1
    return lens, excess > 0


def canonical(lens):
    """RFC 1951 3.2.2: the code of every symbol, bit-reversed (as it goes into the LSB-first stream)."""
    top = max(lens) if lens else 0
    count = [0] * (top + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (top + 2), 0
    for l in range(1, top + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(0)
            continue
        v = nxt[l]
        nxt[l] += 1
        out.append(int(format(v, "0%db" % l)[::-1], 2))
    return out


def rle_lengths(seq):
    """The code-length sequence -> [(symbol, extra value, extra bits)]."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11, 7))
                r -= k
            if r >= 3:
                out.append((17, r - 3, 3))
                r = 0
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3, 2))
                r -= k
        out += [(v, 0, 0)] * r
    return out


class Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        self.total += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def finish(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def deflate(F, w, c, st=None):
    """The deflate stream of F (without the zlib header and the Adler-32)."""
    n = F.size
    length, cand = matches(F, w, c)
    dist = distances(w, c)
    dsym = [dist_symbol(d) if 1 <= d <= 32768 else None for d in dist]
    bits = Bits()
    nblk = (n + BLOCK - 1) // BLOCK
    fixed_bits = 0
    for b in range(nblk):
        lo, hi = b * BLOCK, min(n, (b + 1) * BLOCK)
        tokens, lf, df = [], [0] * 286, [0] * 30
        p = lo
        while p < hi:
            l = int(length[p])
            if l:
                k = int(cand[p])
                tokens.append((l, k))
                lf[len_symbol(l)[0]] += 1
                df[dsym[k][0]] += 1
                if st is not None:
                    st["max_match"] = max(st["max_match"], l)
                    st["taken"][k] += 1
                    st["cross_border"] = st["cross_border"] or p - dist[k] < lo
                p += l
            else:
                tokens.append((0, int(F[p])))
                lf[int(F[p])] += 1
                p += 1
        lf[256] += 1
        ll, rep_l = code_lengths(lf, 15)
        dl, rep_d = code_lengths(df, 15)
        nlit = max(257, max(s for s in range(286) if ll[s]) + 1)
        ndist = max([1] + [s + 1 for s in range(30) if dl[s]])
        rle = rle_lengths(ll[:nlit] + dl[:ndist])
        cf = [0] * 19
        for s, _, _ in rle:
            cf[s] += 1
        cl, rep_c = code_lengths(cf, 7)
        nclen = max(4, max(i for i in range(19) if cl[CLORDER[i]]) + 1)
        lc, dc, cc = canonical(ll), canonical(dl), canonical(cl)
        bits.put(1 if b == nblk - 1 else 0, 1)
        bits.put(2, 2)
        bits.put(nlit - 257, 5)
        bits.put(ndist - 1, 5)
        bits.put(nclen - 4, 4)
        for i in range(nclen):
            bits.put(cl[CLORDER[i]], 3)
        for s, v, e in rle:
            bits.put(cc[s], cl[s])
            if e:
                bits.put(v, e)
        for l, k in tokens:
            if l:
                s, v, e = len_symbol(l)
                bits.put(lc[s], ll[s])
                if e:
                    bits.put(v, e)
                s2, v2, e2 = dsym[k]
                bits.put(dc[s2], dl[s2])
                if e2:
                    bits.put(v2, e2)
                fixed_bits += (7 if s < 280 else 8) + e + 5 + e2
            else:
                bits.put(lc[k], ll[k])
                fixed_bits += 8 if k < 144 else 9
        bits.put(lc[256], ll[256])
        fixed_bits += 3 + 7
        if st is not None:
            used_d = sum(1 for f in df if f)
            st["blocks"] += 1
            st["no_match_blocks"] += used_d == 0
            st["one_dist_blocks"] += used_d == 1
            st["all_literals"] = st["all_literals"] or all(lf[:256])
            st["litlen_repair"] += rep_l
            st["dist_repair"] += rep_d
            st["cl_repair"] += rep_c
            st["tokens"] += len(tokens)
    if st is not None:
        st["fixed_bytes"] = (fixed_bits + 7) // 8
        st["deflate_bits"] = bits.total
    return bits.finish()


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(a, invert=False, st=None):
    """The whole file."""
    a = _hwc(a, invert)
    h, w, c = a.shape
    F, types = filtered(a)
    if st is not None:
        st["filters"] = set(types)
    body = b"\x78\x9c" + deflate(F, w, c, st) + struct.pack(">I", zlib.adler32(F.tobytes()) & 0xFFFFFFFF)
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)) + chunk(b"IDAT", body) + chunk(b"IEND", b"")


def stats(a, invert=False):
    """What the cases are there for (tests/png_cases.py): counts over the blocks of one image."""
    a = _hwc(a, invert)
    h, w, c = a.shape
    st = dict(max_match=0, taken=[0] * CANDIDATES, cross_border=False, blocks=0, no_match_blocks=0, one_dist_blocks=0, all_literals=False,
              litlen_repair=0, dist_repair=0, cl_repair=0, tokens=0)
    data = encode(a, st=st)
    n = h * (1 + w * c)
    st["stream"] = n
    st["stride_dropped"] = 1 + w * c > 32768
    st["idat"] = len(data) - 8 - 25 - 12 - 12
    st["fixed_idat"] = 2 + st["fixed_bytes"] + 4
    st["stored_idat"] = 2 + n + 5 * ((n + 65534) // 65535) + 4
    st["file"] = len(data)
    return st


def bound(w, h, c):
    """i2i_png_bound: no file of the contract is larger.  A literal costs at most 15 bits for one byte, a match at most 15 + 5 + 15 + 13 = 48
    bits for at least 3 bytes: 16 bits per byte of F.  A block adds 3 + 14 + 19 * 3 header bits, at most 7 bits per code length (a run symbol
    with its extra bits covers at least 3 lengths in at most 14 bits) for 286 + 30 lengths, and 15 bits of end-of-block: 2301 bits."""
    n = h * (1 + w * c)
    nblk = (n + BLOCK - 1) // BLOCK
    return 8 + 25 + 12 + 2 + (2301 * nblk + 7) // 8 + 2 * n + 4 + 12


def chunks(data):
    """[(kind, payload, crc ok)] of a PNG file."""
    assert data[:8] == SIGNATURE
    out, i = [], 8
    while i < len(data):
        n, = struct.unpack(">I", data[i:i + 4])
        kind, payload = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        crc, = struct.unpack(">I", data[i + 8 + n:i + 12 + n])
        out.append((kind, payload, crc == (zlib.crc32(kind + payload) & 0xFFFFFFFF)))
        i += 12 + n
    assert i == len(data)
    return out

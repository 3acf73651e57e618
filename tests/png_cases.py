"""Cases and backend-independent checks shared by tests/test_png_emu.py (CPU emulator) and tests/test_png_gpu.py (MI355X): PNG encoding on
the device -- i2i_png_encode_u8, i2i_png_workspace_bytes, i2i_png_bound (csrc/png.inc; the contract is the comment of i2i_png_image in
include/i2i_turbo.h), image_ops.png_encode_u8 and ``png=`` / ``return_edges="png"`` of the models' forward_u8.  The oracle is
tests/png_ref.py (integer numpy); device against oracle is ``==`` on whole files, oracle against Pillow is ``==`` on the container and on
the decompressed (filtered) scanline stream.  No tolerance exists."""
import ctypes as C
import functools
import io
import zlib

import numpy as np
import torch

import png_ref

FILL = 0xA5
GUARD = 64               # bytes in front of and behind every slot of the output pool
PARENT_SIZEOF_OP = 368

# csrc/png.inc: a deflate block is BLOCK = 16384 bytes of the filtered stream; the checksums, the copy of the deflate bytes and their
# second-level reductions work on chunks of CHUNK = 1024 bytes (of the filtered stream for Adler-32, of the deflate stream for CRC-32); the
# bit offsets of a block's 256 segments are scanned inside the workgroup and the blocks in front are the second level.  BIG = 136 x 168: RGB
# 136 * 505 = 68680 bytes = 5 blocks, grey 136 * 169 = 22984 bytes = 2 blocks (so BIG_GREY = 300 x 168 = 50700 bytes = 4 blocks stands in for
# grey); the noise and smooth contents keep their deflate stream over three chunks (asserted in check_big_spans_three).
BLOCK, CHUNK = 16384, 1024
BIG = (136, 168)
BIG_GREY = (300, 168)
SIZES = [(1, 1), (1, 40), (3, 5), (17, 23), (9, 50), (64, 72), (2, 11000), BIG]
CONTENTS = ["noise", "binary", "ramp", "flat", "smooth"]
CHANNELS = [3, 1]


@functools.lru_cache(maxsize=None)
def image(content, h, w, c, seed=0):
    rng = np.random.RandomState(1000 * seed + 7 * h + w + 31 * CONTENTS.index(content) + c)
    if content == "noise":
        a = rng.randint(0, 256, (h, w, c))
    elif content == "binary":                                # an edge map: grey replicated
        a = np.repeat((rng.rand(h, w, 1) < 0.1).astype(np.int64) * 255, c, axis=2)
    elif content == "ramp":
        a = (np.arange(h)[:, None, None] * 3 + np.arange(w)[None, :, None] * 2 + np.arange(c)[None, None, :] * 7) % 256
    elif content == "flat":
        a = np.full((h, w, c), 200)
    else:                                                    # a smooth random walk, as a generated photograph is locally
        a = np.clip(np.cumsum(rng.randint(-3, 4, (h, w, c)), axis=1) + np.cumsum(rng.randint(-3, 4, (h, 1, c)), axis=0) + 128, 0, 255)
    a = a.astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def steep():
    """Byte frequencies whose Huffman tree is a chain 17 deep, so the limit-15 repair of the literal/length code has to run: six values
    twice (with the end-of-block symbol the bushy bottom of the tree, about 20 in all), then 20, 22 and on with every count 2 above the sum
    of all counts two places below it -- the chain holds while what gathers at the bottom stays under 22, which leaves room for a few
    stray symbols.  75 x 200 grey pixels, one deflate block; the values are small, so None stays the cheapest filter; the seeded order is
    mended (a pixel of every match swapped with a random one) until no three bytes repeat at a candidate distance: length symbols with
    middling counts would flatten the tree."""
    w = [20, 22]
    below = 40                                               # the sum of everything under w[-1]
    while 12 + sum(w) + below + 2 <= 15000:
        below, nxt = below + w[-1], below + 2
        w.append(nxt)
    order = sorted([2] * 6 + w, reverse=True)
    vals = np.concatenate([np.full(f, ((r + 1) // 2) * (1 if r % 2 else -1) % 256, np.int64) for r, f in enumerate(order)])
    h, wd = 75, 200
    vals = np.concatenate([vals, np.zeros(h * wd - vals.size, np.int64)])
    rng = np.random.RandomState(5)
    a = rng.permutation(vals).reshape(h, wd)
    for _ in range(200):
        F, _types = png_ref.filtered(a.astype(np.uint8)[:, :, None])
        hit = np.flatnonzero(png_ref.matches(F, wd, 1)[0])
        if hit.size == 0:
            break
        for p in hit:
            for q in (p, p + 1, p + 2):
                y, x = divmod(int(q), 1 + wd)
                if x == 0 or y >= h:
                    continue
                y2, x2 = rng.randint(h), rng.randint(wd)
                a[y, x - 1], a[y2, x2] = a[y2, x2], a[y, x - 1]
                break
    a = a.astype(np.uint8)[:, :, None]
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cl_repair_image():
    """An image whose code-length alphabet needs its limit-7 repair, searched with fixed seeds at first use: byte values with roughly
    geometric frequencies give headers with a few frequent and many rare length symbols.  None if the search finds nothing."""
    for seed in range(8):
        rng = np.random.RandomState(4000 + seed)
        k, base = int(rng.randint(8, 60)), rng.uniform(1.15, 1.9)
        counts = np.minimum(np.floor(base ** np.arange(k) * rng.uniform(0.6, 1.4, k)), 6000).astype(np.int64) + 1
        vals = np.concatenate([np.full(int(f), int(v), np.int64) for v, f in zip(rng.permutation(256)[:k], counts)])[-16000:]
        h = 8
        w = max(1, vals.size // h)
        a = rng.permutation(vals)[:h * w].reshape(h, w, 1).astype(np.uint8)
        if png_ref.stats(a)["cl_repair"]:
            a.setflags(write=False)
            return a
    return None


def grid():
    return [(content, h, w, c) for (h, w) in SIZES for c in CHANNELS for content in CONTENTS]


@functools.lru_cache(maxsize=None)
def want(content, h, w, c, invert=False):
    """The oracle's file for a case of the grid, computed once and shared."""
    return png_ref.encode(image(content, h, w, c), invert)


@functools.lru_cache(maxsize=None)
def stats(content, h, w, c):
    return png_ref.stats(image(content, h, w, c))


def pillow_bytes(a):
    from PIL import Image
    f = io.BytesIO()
    a = np.asarray(a)
    Image.fromarray(a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a).save(f, "PNG")
    return f.getvalue()


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def check_file_against_pillow(data, a, what):
    """Container and filtered stream are Pillow's, every CRC holds, the file decodes to the array, the size is under the bound."""
    a = np.asarray(a)
    pil = pillow_bytes(a)
    mine, theirs = png_ref.chunks(data), png_ref.chunks(pil)
    assert data[:8] == pil[:8] == png_ref.SIGNATURE, what
    assert [k for k, _, _ in mine] == [b"IHDR", b"IDAT", b"IEND"], (what, [k for k, _, _ in mine])
    assert all(ok for _, _, ok in mine), (what, "a CRC-32 is wrong")
    assert {k for k, _, _ in theirs} == {b"IHDR", b"IDAT", b"IEND"}, what
    assert mine[0] == theirs[0] and mine[-1] == theirs[-1], what
    body = mine[1][1]
    assert body[:2] == b"\x78\x9c", what
    assert zlib.decompress(body) == zlib.decompress(b"".join(p for k, p, _ in theirs if k == b"IDAT")), (what, "the filtered stream differs")
    got = decode(data)
    assert got.shape == (a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a).shape and (got.reshape(a.shape) == a).all(), what
    h, w = a.shape[:2]
    assert len(data) <= png_ref.bound(w, h, 1 if a.ndim == 2 else a.shape[2]), what


def check_oracle_matches_pillow(h, w):
    for c in CHANNELS:
        for content in CONTENTS:
            check_file_against_pillow(want(content, h, w, c), image(content, h, w, c), "%s %dx%dx%d" % (content, h, w, c))
    if (h, w) == BIG:
        check_file_against_pillow(png_ref.encode(steep()), steep(), "steep")
        check_file_against_pillow(png_ref.encode(image("noise", *BIG_GREY, 1)), image("noise", *BIG_GREY, 1), "big grey")
        check_file_against_pillow(png_ref.encode(image("binary", 17, 23, 3), invert=True), 255 - image("binary", 17, 23, 3), "invert")
        a = cl_repair_image()
        if a is not None:
            check_file_against_pillow(png_ref.encode(a), a, "cl repair")


def check_case_properties():
    """What the cases are there for, asserted through the oracle's stats()."""
    all_stats = {k: stats(*k) for k in grid()}
    assert stats("noise", 1, 1, 3)["no_match_blocks"] == 1
    assert any(s["one_dist_blocks"] for k, s in all_stats.items() if k[0] == "flat")
    assert any(s["max_match"] == 258 for s in all_stats.values())
    assert any(s["cross_border"] for s in all_stats.values())
    assert any(s["all_literals"] for k, s in all_stats.items() if k[0] == "noise")
    assert any(s["taken"][2] for s in all_stats.values()), "the row-stride candidate is never taken"
    assert all(any(s["taken"][k] for s in all_stats.values()) for k in (0, 3, 4))
    assert any(s["taken"][1] for k, s in all_stats.items() if k[3] == 3), "distance c is never taken on RGB"
    for content in CONTENTS:
        s = all_stats[(content, 2, 11000, 3)]
        assert s["stride_dropped"] and s["taken"][2] == s["taken"][3] == s["taken"][4] == 0
    filters = set()
    for s in all_stats.values():
        filters |= s["filters"]
    assert filters == {0, 1, 2, 4}
    for (content, h, w, c), s in all_stats.items():
        if (content == "smooth" and h * w >= 17 * 23) or (content == "ramp" and h * w >= 64 * 72):   # (a dynamic header is some 20 bytes: the ramp, all zeros after Sub / Paeth, beats the fixed code only once the stream has a few KB)
            assert s["idat"] < s["fixed_idat"], (content, h, w, c, s["idat"], s["fixed_idat"])
        if content in ("flat", "binary") and h * w >= 17 * 23:
            assert s["idat"] < s["stored_idat"], (content, h, w, c, s["idat"], s["stored_idat"])


def check_litlen_repair_case():
    """The limit-15 repair of the literal/length code runs on an image (steep(): no match, filter None, one block)."""
    st = png_ref.stats(steep())
    assert st["litlen_repair"] >= 1, "the length-limit repair of the literal/length code never runs on an image"
    assert st["filters"] == {0} and st["blocks"] == 1 and sum(st["taken"]) == 0


def check_repair_rule():
    """code_lengths on exact Fibonacci frequencies: the limit-15 repair runs, the lengths stay a complete prefix code within the limit."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    for n in (17, 19, 22):
        lens, repaired = png_ref.code_lengths(fib[:n] + [0] * (286 - n), 15)
        assert repaired and max(lens) == 15 and sum(1 << (15 - l) for l in lens if l) == 1 << 15
        assert all(lens[i] >= lens[i + 1] for i in range(n - 1))            # the rarest symbols hold the longest codes


def check_cl_repair_case():
    """The limit-7 repair of the code-length alphabet: a seeded search (cl_repair_image)."""
    a = cl_repair_image()
    assert a is not None, "no image of the search needs the limit-7 repair of the code-length alphabet: that repair is uncovered"
    assert png_ref.stats(a)["cl_repair"] >= 1


def check_big_spans_three():
    for c, (h, w) in ((3, BIG), (1, BIG_GREY)):
        for content in ("noise", "smooth"):
            s = png_ref.stats(image(content, h, w, c))
            assert s["blocks"] >= 3 and s["stream"] > 2 * BLOCK, (content, c, s["blocks"])
            assert s["stream"] > 2 * CHUNK and s["idat"] - 6 > 2 * CHUNK, (content, c, s["idat"])


# ---------------------------------------------------------------------------------------------------------------- the raw entry
def to_dev(a, device):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(device)


def sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def stream_of(device):
    return torch.cuda.current_stream().cuda_stream if device != "cpu" else 0


def stream_bytes(a):
    h, w = a.shape[:2]
    return h * (1 + w * (1 if a.ndim == 2 else a.shape[2]))


class Batch:
    """One ragged batch in caller-owned, FILL-ed buffers: the pixel arena, the output pool with a guard in front of and behind every slot,
    descriptors packed here (not by image_ops), lengths and the flag word.  ``caps``: bytes per slot (default: the oracle's length)."""

    def __init__(self, lib, device, imgs, *, inverts=None, caps=None, max_bytes=None, expect=None):
        from img2img_turbo_amd import image_ops, ops as O
        self.lib, self.device, self.n = lib, device, len(imgs)
        inverts = inverts if inverts is not None else [False] * self.n
        self.expect = expect if expect is not None else [png_ref.encode(a, v) for a, v in zip(imgs, inverts)]
        self.caps = caps if caps is not None else [len(e) for e in self.expect]
        self.desc = np.zeros(self.n, dtype=image_ops.PNG_IMAGE_DTYPE)
        src_off, dst_off, arena = 0, GUARD, []
        for b, (a, v, cap) in enumerate(zip(imgs, inverts, self.caps)):
            h, w = a.shape[:2]
            c = 1 if a.ndim == 2 else a.shape[2]
            self.desc[b] = (src_off, dst_off, h, w, c, 1 if v else 0, cap, (0, 0, 0))
            flat = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
            arena.append(np.concatenate([flat, np.full(1 + b % 3, FILL, dtype=np.uint8)]))      # (no alignment is asked of the pixels)
            src_off += arena[-1].size
            dst_off += cap + GUARD
        self.largest = max(stream_bytes(a) for a in imgs)
        self.max_bytes = max_bytes or self.largest
        self.arena = to_dev(np.concatenate(arena), device)
        self.pool = torch.full((dst_off,), FILL, dtype=torch.uint8, device=device)
        self.length = torch.full((self.n,), 77, dtype=torch.int32, device=device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=device)
        self.ws = torch.full((max(lib.png_workspace_bytes(self.n, self.max_bytes), 16),), FILL, dtype=torch.uint8, device=device)   # needs no initialisation
        self.desc_dev = torch.zeros(self.n * 6, dtype=torch.int64, device=device)
        self.O = O

    def params(self):
        self.desc_dev.copy_(torch.from_numpy(self.desc.view(np.int64).reshape(-1).copy()))
        return self.O.png_encode_u8(self.arena, self.pool, self.desc_dev, self.length, self.ws, n=self.n, max_bytes=self.max_bytes, bad_mask=self.bad)

    def run(self):
        p = self.params()
        self.lib.check(self.lib.lib.i2i_png_encode_u8(C.addressof(p), 0, C.c_void_p(stream_of(self.device))))
        sync(self.device)
        return self

    def mask(self):
        return int(self.bad.cpu().numpy().view(np.uint32)[0])

    def files(self):
        pool, lens = self.pool.cpu().numpy(), self.length.cpu().numpy()
        return [pool[int(o):int(o) + int(l)].tobytes() for o, l in zip(self.desc["dst_off"], lens)]

    def check(self, flagged=(), what=""):
        """Every image not in ``flagged`` is the oracle's file; a flagged one has length 0 and its bit set; every byte of the pool outside
        the files that were written still holds FILL."""
        pool, lens = self.pool.cpu().numpy(), self.length.cpu().numpy()
        untouched = np.ones(pool.size, dtype=bool)
        for b in range(self.n):
            o = int(self.desc["dst_off"][b])
            if b in flagged:
                assert lens[b] == 0, (what, b, lens[b])
                continue
            got = pool[o:o + int(lens[b])].tobytes()
            assert got == self.expect[b], explain(got, self.expect[b], "%s image %d" % (what, b))
            untouched[o:o + len(got)] = False
        assert (pool[untouched] == FILL).all(), (what, "pool", np.flatnonzero(untouched & (pool != FILL))[:8])
        want_mask = 0
        for b in flagged:
            want_mask |= 1 << (b & 31)
        assert self.mask() == want_mask, (what, hex(self.mask()), hex(want_mask))


def explain(got, ref, what):
    if len(got) < 45:
        return "%s: %d bytes against %d" % (what, len(got), len(ref))
    first = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
    part = "the front (signature, IHDR, IDAT length)" if first < 43 else "the deflate stream / trailer"
    return "%s: differs from byte %d on, in %s (%d vs %d bytes)" % (what, first, part, len(got), len(ref))


def check_grid(lib, device, h, w):
    """Contents x channel counts at one size as ONE ragged call (RGB and grey descriptors side by side): every file equals the oracle's and
    the guards hold."""
    cases = [(content, c) for c in CHANNELS for content in CONTENTS]
    imgs = [image(content, h, w, c) for content, c in cases]
    expect = [want(content, h, w, c) for content, c in cases]
    if (h, w) == BIG:
        extra = [steep(), image("noise", *BIG_GREY, 1), image("smooth", *BIG_GREY, 1)] + ([cl_repair_image()] if cl_repair_image() is not None else [])
        imgs += extra
        expect += [png_ref.encode(a) for a in extra]
    Batch(lib, device, imgs, expect=expect).run().check(what="%dx%d" % (h, w))


RAGGED = [((1, 1), "noise", 3), ((17, 23), "binary", 1), ((9, 50), "smooth", 3), ((64, 72), "noise", 1), ((3, 5), "flat", 3), ((1, 40), "ramp", 1),
          ((64, 72), "smooth", 3), ((136, 168), "binary", 3)]


def check_ragged_batch(lib, device):
    """Eight images of different sizes and channel counts in one call == eight single-image calls == the oracle; through
    image_ops.png_encode_u8 forwards and reversed (per channel count: one call shares c), a stacked tensor, HW tensors, return_tensors."""
    from img2img_turbo_amd import image_ops
    imgs = [image(content, h, w, c) for (h, w), content, c in RAGGED]
    expect = [want(content, h, w, c) for (h, w), content, c in RAGGED]
    together = Batch(lib, device, imgs, expect=expect).run()
    together.check(what="ragged")
    files = together.files()
    for k in range(len(RAGGED)):
        alone = Batch(lib, device, imgs[k:k + 1], expect=expect[k:k + 1]).run()
        alone.check(what="alone %d" % k)
        assert alone.files()[0] == files[k]
    rev = Batch(lib, device, imgs[::-1], expect=expect[::-1]).run()
    rev.check(what="reversed")
    for c in CHANNELS:
        sel = [k for k in range(len(RAGGED)) if RAGGED[k][2] == c]
        dev = [to_dev(imgs[k], device) for k in sel]
        assert image_ops.png_encode_u8(dev, lib=lib) == [expect[k] for k in sel]
        assert image_ops.png_encode_u8(dev[::-1], lib=lib) == [expect[k] for k in sel][::-1]
    stack = np.stack([image("noise", 9, 50, 3), image("smooth", 9, 50, 3)])
    assert image_ops.png_encode_u8(to_dev(stack, device), lib=lib) == [png_ref.encode(a) for a in stack]
    grey = image("smooth", 17, 23, 1)
    assert image_ops.png_encode_u8([to_dev(grey[:, :, 0], device)], lib=lib) == [png_ref.encode(grey)]
    dev = [to_dev(imgs[k], device) for k in range(len(RAGGED)) if RAGGED[k][2] == 3]
    pool, offs, lens, bad = image_ops.png_encode_u8(dev, lib=lib, return_tensors=True)
    sync(device)
    assert int(bad.cpu()[0]) == 0
    assert [pool[o:o + int(l)].cpu().numpy().tobytes() for o, l in zip(offs, lens.cpu().tolist())] == [expect[k] for k in range(len(RAGGED)) if RAGGED[k][2] == 3]


def check_invert(lib, device):
    """flags bit 0: the file of 255 - x, per image (a batch may mix), and image_ops' invert=."""
    from img2img_turbo_amd import image_ops
    imgs = [image("binary", 17, 23, 3), image("binary", 17, 23, 3), image("smooth", 9, 50, 1), image("binary", 64, 72, 1)]
    inv = [True, False, True, True]
    b = Batch(lib, device, imgs, inverts=inv).run()
    b.check(what="invert")
    files = b.files()
    assert files[0] != files[1]
    for f, a, v in zip(files, imgs, inv):
        assert (decode(f).reshape(a.shape) == (255 - a if v else a)).all()
    assert image_ops.png_encode_u8([to_dev(imgs[0], device), to_dev(imgs[1], device)], invert=[True, False], lib=lib) == files[:2]
    assert image_ops.png_encode_u8([to_dev(imgs[0], device)], invert=True, lib=lib) == [png_ref.encode(255 - imgs[0])]


def check_grid_independence(lib, device):
    """The capacity hint sizes grids and workspace slots only: the smallest legal one and one 64 times larger give the same bytes."""
    imgs = [image(content, h, w, c) for (h, w), content, c in RAGGED] + [image("noise", *BIG, 3)]
    res = []
    for scale in (1, 64):
        b = Batch(lib, device, imgs)
        b.max_bytes = b.largest * scale
        b.ws = torch.full((lib.png_workspace_bytes(b.n, b.max_bytes),), FILL, dtype=torch.uint8, device=device)
        b.run().check(what="max_bytes x%d" % scale)
        res.append(b.files())
    assert res[0] == res[1]


def check_overflow(lib, device):
    """A capacity one byte short of the file: the image's bit is set, its length is 0, NOTHING of its slot or of the guards around it is
    written, and the other images of the batch are the oracle's files."""
    import pytest
    from img2img_turbo_amd import _capi, image_ops
    sel = [2, 6, 7, 4]
    imgs = [image(RAGGED[k][1], *RAGGED[k][0], RAGGED[k][2]) for k in sel]
    expect = [png_ref.encode(a) for a in imgs]
    for victim in (0, 2):
        caps = [len(e) for e in expect]
        caps[victim] -= 1
        Batch(lib, device, imgs, caps=caps, expect=expect).run().check(flagged=(victim,), what="overflow %d" % victim)
    with pytest.raises(_capi.I2IError) as e:
        image_ops.png_encode_u8([to_dev(a, device) for a in imgs], lib=lib, capacity=[len(x) for x in expect[:2]] + [len(expect[2]) - 1, len(expect[3])])
    assert "image 2" in str(e.value)


REJECTS = ["an offset beyond the arena", "w = 0", "h beyond 65535", "a slot beyond the pool", "a stream longer than max_bytes", "five channels"]


def check_rejection(lib, device, what):
    """EMULATOR ONLY (the GPU tests use valid descriptors): image 1 of four has a wrong descriptor.  It is flagged, gets length 0, nothing
    of the pool is written for it, and its neighbours are the oracle's files."""
    imgs = [image(RAGGED[k][1], *RAGGED[k][0], RAGGED[k][2]) for k in (2, 6, 1, 4)]
    b = Batch(lib, device, imgs)
    d = b.desc
    if what == "an offset beyond the arena":
        d["src_off"][1] = b.arena.numel() - 16
    elif what == "w = 0":
        d["w"][1] = 0
    elif what == "h beyond 65535":
        d["h"][1] = 65536
    elif what == "a slot beyond the pool":
        d["dst_off"][1] = b.pool.numel() - 8
    elif what == "a stream longer than max_bytes":
        d["h"][1], d["w"][1], d["c"][1] = 1, b.max_bytes, 1     # (inside the arena: one row of max_bytes grey pixels is max_bytes + 1 bytes of stream)
        b.arena = torch.cat([b.arena, torch.zeros(b.max_bytes, dtype=torch.uint8, device=b.arena.device)])
    elif what == "five channels":
        d["c"][1] = 5
    else:
        raise AssertionError(what)
    b.run().check(flagged=(1,), what=what)


def check_bad_args(lib, device):
    """Every host-side error of the contract returns I2I_ERR_BAD_ARG with a message and launches nothing; n == 0 is a successful no-op."""
    b = Batch(lib, device, [image("noise", 3, 5, 3)])
    entry = lib.lib.i2i_png_encode_u8
    p = b.params()
    for kw in (dict(src=0), dict(dst=0), dict(images=0), dict(length=0), dict(ws=0), dict(length=p.length + 2), dict(bad_mask=p.bad_mask + 1),
               dict(images=p.images + 4), dict(ws=p.ws + 8), dict(n=-1), dict(max_bytes=0), dict(max_bytes=(1 << 27) + 1), dict(src_bytes=-1),
               dict(dst_bytes=-1), dict(ws_bytes=p.ws_bytes - 1)):
        q = b.params()
        for k, v in kw.items():
            setattr(q, k, v)
        assert entry(C.addressof(q), 0, C.c_void_p(stream_of(device))) == -1, kw
        msg = lib.lib.i2i_last_error().decode()
        assert msg.startswith("png_encode_u8:") and len(msg) > 15, (kw, msg)
    assert entry(None, 0, C.c_void_p(stream_of(device))) == -1
    q = b.params()
    q.n = 0
    assert entry(C.addressof(q), 0, C.c_void_p(stream_of(device))) == 0
    sync(device)
    assert (b.pool.cpu().numpy() == FILL).all() and b.mask() == 0
    assert lib.png_workspace_bytes(1, 0) == 0 and lib.png_workspace_bytes(-1, 8) == 0 and lib.png_workspace_bytes(1, (1 << 27) + 1) == 0
    assert lib.png_workspace_bytes(2, 800) == 2 * lib.png_workspace_bytes(1, 800) > 0


# ---------------------------------------------------------------------------------------------------------------- the ABI and the host code
def check_abi(lib):
    """Additive: the version is 14, sizeof(i2i_op) did not grow, no opcode was added, the new symbols are there, the descriptor is 48 bytes
    in both bindings."""
    from img2img_turbo_amd import _capi as K, image_ops
    assert lib.lib.i2i_sizeof_op() == C.sizeof(K.Op) == PARENT_SIZEOF_OP
    assert lib.lib.i2i_abi_version() == K.ABI_VERSION == 14
    assert max(v for k, v in vars(K).items() if k.startswith("OP_") and isinstance(v, int)) == K.OP_TILE_BLEND_U8 == 28
    for name in ("i2i_png_encode_u8", "i2i_png_workspace_bytes", "i2i_png_bound"):
        assert hasattr(lib.lib, name) and name in K.EXPORTS
    assert C.sizeof(K.PngImage) == 48 == image_ops.PNG_IMAGE_DTYPE.itemsize
    assert ([image_ops.PNG_IMAGE_DTYPE.fields[n][1] for n, _ in K.PngImage._fields_] == [getattr(K.PngImage, n).offset for n, _ in K.PngImage._fields_])
    assert K.PNG_BLOCK_BYTES == png_ref.BLOCK == BLOCK


def check_bound(lib):
    """i2i_png_bound (plain host code) == the oracle's formula, no file of the grid exceeds it, and its refusals."""
    for (h, w) in SIZES + [(65535, 65535), (512, 512), (1, 16383), (1, 16384)]:
        for c in CHANNELS:
            assert lib.png_bound(w, h, c) == png_ref.bound(w, h, c), (w, h, c)
    for content, h, w, c in grid():
        assert len(want(content, h, w, c)) <= lib.png_bound(w, h, c)
    for args in ((0, 8, 3), (8, 65536, 3), (8, 8, 2), (-1, 8, 1), (8, 8, 4)):
        assert lib.lib.i2i_png_bound(*args) == -1, args
        assert lib.lib.i2i_last_error().decode().startswith("png_bound:")


# ---------------------------------------------------------------------------------------------------------------- the models
def check_forward_png(lib, device, kind, dtype=torch.float32, light=False):
    """forward_u8(png=True) on the tiny synthetic model: the files decode with Pillow to exactly the uint8 output of the same call without
    png= and equal image_ops.png_encode_u8 of it -- plain, with variations=2 (pix2pix), with tile= on two requests of different sizes, with
    return_edges="png" (files that decode to 255 - edges); png= beside jpeg= is refused with no plan built.  ``light`` (the emulator, where a
    forward is a minute): the refusals and the plain call only."""
    import pytest
    import tile_cases as tc
    from img2img_turbo_amd import image_ops
    model = tc.make_pix2pix(lib, device, dtype) if kind == "pix2pix" else tc.make_cyclegan(lib, device, dtype)
    try:
        cap = tc.caption(device)
        base = dict(caption_enc=cap) if kind == "pix2pix" else dict(direction="a2b", caption_emb=cap)
        x = torch.stack([tc.to_dev(tc.photo(32, 40, i), device) for i in range(2)])
        eps = torch.randn(2, 4, 4, 5, generator=torch.Generator().manual_seed(3)).to(device)

        def same(files, outs):
            outs = list(outs)
            assert isinstance(files, list) and len(files) == len(outs) and all(isinstance(f, bytes) for f in files)
            for f, o in zip(files, outs):
                assert (decode(f) == o.cpu().numpy()).all()
            assert files == image_ops.png_encode_u8(outs, lib=lib)

        for bad in (dict(png=True, jpeg=90), dict(png=True, jpeg=True), dict(png=3), dict(png="yes")):
            with pytest.raises(ValueError):
                model.forward_u8(x, eps=eps, **bad, **base)
        assert not model._plans
        plain = model.forward_u8(x, eps=eps, **base)
        files = model.forward_u8(x, eps=eps, png=True, **base)
        same(files, plain)
        assert files == [png_ref.encode(o.cpu().numpy()) for o in plain]
        assert torch.equal(model.forward_u8(x, eps=eps, png=None, **base), plain)
        if light:
            return
        if kind == "pix2pix":
            out = model.forward_u8(x, seed=[[1, 2], [3, 4]], variations=2, **base)
            files = model.forward_u8(x, seed=[[1, 2], [3, 4]], variations=2, png=True, **base)
            assert out.shape[0] == 4
            same(files, out)
            out, edges = model.forward_u8(x, eps=eps, canny=(100, 200), return_edges=True, **base)
            files, efiles = model.forward_u8(x, eps=eps, canny=(100, 200), return_edges="png", png=True, **base)
            same(files, out)
            assert len(efiles) == 2 and efiles == image_ops.png_encode_u8(edges, invert=True, lib=lib)
            for f, e in zip(efiles, edges):
                assert (decode(f) == 255 - e.cpu().numpy()).all()
            out2, efiles2 = model.forward_u8(x, eps=eps, canny=(100, 200), return_edges="png", **base)
            assert torch.equal(out2, out) and efiles2 == efiles
            out3, edges3 = model.forward_u8(x, eps=eps, canny=(100, 200), return_edges=True, png=True, **base)
            assert torch.equal(edges3, edges) and out3 == files
        reqs = [tc.to_dev(tc.photo(h, w, 5 + i), device) for i, (h, w) in enumerate([(56, 72), (32, 40)])]
        kw = dict(tile=tc.MODEL_TILE, tile_overlap=8, tile_batch=4, seed=[7, 8], **base)
        outs = model.forward_u8(reqs, **kw)
        files = model.forward_u8(reqs, png=True, **kw)
        assert [tuple(o.shape) for o in outs] == [(56, 72, 3), (32, 40, 3)]
        same(files, outs)
    finally:
        model.release_plans()

"""Cases and backend-independent checks shared by tests/test_jpeg_emu.py (CPU emulator) and tests/test_jpeg_gpu.py (MI355X): JPEG encoding on
the device -- i2i_jpeg_encode_u8, i2i_jpeg_workspace_bytes, i2i_jpeg_header (csrc/jpeg.inc; the contract is the comment of i2i_jpeg_image in
include/i2i_turbo.h), image_ops.jpeg_encode_u8 and ``jpeg=`` of the two models' forward_u8.  The oracle is tests/jpeg_ref.py (integer numpy);
every comparison is ``==`` on bytes, against the oracle AND, where PIL.features.check("jpg") holds, against Pillow itself.  No tolerance
exists: the encoder is integer arithmetic and bit packing."""
import ctypes as C
import functools
import io

import numpy as np
import torch

import jpeg_ref

FILL = 0xA5
GUARD = 64               # bytes in front of and behind every slot of the output pool
PARENT_SIZEOF_OP = 368

# The chunk sizes of the two prefix sums (csrc/jpeg.inc): CHUNK_BLOCKS = 256 blocks per chunk of the bit offsets, CHUNK_WORDS = 256 words =
# 1024 bytes of packed stream per chunk of the stuffed-byte counts.  BIG = 136 x 168 has 17 * 21 * 3 = 1071 blocks in 4:4:4 (five chunks) and
# 9 * 11 * 6 = 594 in 4:2:0 (three chunks, the last one partial; 136 = 8 * 16 + 8 also gives a bottom row of dummy Y blocks); its stream on
# noise at quality 75 is over 10 KB, ten chunks and more (asserted in check_big_has_three_chunks).  Flat content cannot fill three stream
# chunks at any size worth testing: an EOB-only block is a byte.
CHUNK_BLOCKS, CHUNK_BYTES = 256, 1024
BIG = (136, 168)
SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (24, 40), (40, 24), (33, 16), (9, 50), (25, 7), (64, 72), BIG]
CONTENTS = ["noise", "binary", "ramp", "flat"]
QUALITIES = [1, 25, 50, 75, 90, 95, 100]
SUBSAMPLINGS = ["4:4:4", "4:2:0"]


def have_pillow_jpeg():
    try:
        from PIL import features
        return bool(features.check("jpg"))
    except Exception:
        return False


@functools.lru_cache(maxsize=None)
def image(content, h, w, seed=0):
    rng = np.random.RandomState(1000 * seed + 7 * h + w + 31 * CONTENTS.index(content))
    if content == "noise":
        a = rng.randint(0, 256, (h, w, 3))
    elif content == "binary":                                # the largest magnitudes, many 0xFF bytes in the stream
        a = rng.randint(0, 2, (h, w, 3)) * 255
    elif content == "ramp":                                  # smooth: long zero runs between the few coefficients that survive
        a = np.stack([np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256, np.add.outer(np.arange(h), np.arange(w) * 5) % 256,
                      np.add.outer(np.arange(h) * 2, np.arange(w)) % 256], axis=-1)
    else:
        a = np.full((h, w, 3), 255)
    a = a.astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(content, h, w, q, s):
    """The oracle's file for a case of the grid, computed once and shared."""
    return jpeg_ref.encode(image(content, h, w), q, s)


def pillow_bytes(img, q, s):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.asarray(img)).save(f, "JPEG", quality=q, subsampling=jpeg_ref.SUBSAMPLINGS[s])
    return f.getvalue()


def markers(data):
    """[(marker byte, segment bytes)] of a file's header up to and including SOS."""
    out, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        n = (data[i + 2] << 8) | data[i + 3]
        out.append((data[i + 1], bytes(data[i:i + 2 + n])))
        i += 2 + n
        if out[-1][0] == 0xDA:
            break
    return out, i


def explain(got, ref, what):
    """The message of a mismatch: which header marker differs, or that the header agrees and the scan does not."""
    (mg, ig), (mr, ir) = markers(got), markers(ref)
    for k, (a, b) in enumerate(zip(mg, mr)):
        if a != b:
            return "%s: header segment %d differs: marker 0x%02X %s vs 0x%02X %s" % (what, k, a[0], a[1].hex(), b[0], b[1].hex())
    if len(mg) != len(mr) or ig != ir:
        return "%s: the headers hold %d vs %d segments (%d vs %d bytes)" % (what, len(mg), len(mr), ig, ir)
    first = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
    return "%s: the headers agree; the scans differ from byte %d on (%d vs %d bytes)" % (what, first - ig, len(got) - ig, len(ref) - ir)


def check_oracle_matches_pillow(h, w):
    """tests/jpeg_ref.py == the installed Pillow, whole files, over contents x qualities x subsamplings at one size."""
    for content in CONTENTS:
        for q in QUALITIES:
            for s in SUBSAMPLINGS:
                ref, pil = want(content, h, w, q, s), pillow_bytes(image(content, h, w), q, s)
                assert ref == pil, explain(ref, pil, "oracle vs Pillow, %s %dx%d q%d %s" % (content, h, w, q, s))


def check_case_properties():
    """What the contents are there for, asserted through the oracle: stuffed bytes, a stuffed byte at the very end of a scan or within 4 bytes
    of a chunk boundary of the packed stream, a ZRL symbol on the ramp."""
    st = jpeg_ref.stats(image("binary", 64, 72), 100, "4:4:4")
    assert len(st["stuffed"]) >= 1
    edge = False
    for (h, w) in SIZES:
        for q in QUALITIES:
            for s in SUBSAMPLINGS:
                t = jpeg_ref.stats(image("binary", h, w), q, s)
                edge = edge or any(p == t["raw"] - 1 or p % CHUNK_BYTES < 4 or p % CHUNK_BYTES >= CHUNK_BYTES - 4 for p in t["stuffed"])
    assert edge, "no case of the binary content has a stuffed byte at the end of its scan or beside a chunk boundary"
    assert any(jpeg_ref.stats(image("ramp", h, w), q, s)["zrl"] > 0 for (h, w) in SIZES for q in QUALITIES for s in SUBSAMPLINGS)
    flat = want("flat", 16, 16, 75, "4:2:0")
    assert len(flat) - jpeg_ref.HEADER_BYTES - 2 < 16                           # EOB-only blocks


def check_big_has_three_chunks():
    from img2img_turbo_amd import image_ops
    for s in SUBSAMPLINGS:
        assert image_ops.jpeg_blocks(BIG[0], BIG[1], s) > 2 * CHUNK_BLOCKS
        assert jpeg_ref.stats(image("noise", *BIG), 75, s)["raw"] > 2 * CHUNK_BYTES


# ---------------------------------------------------------------------------------------------------------------- the raw entry
def to_dev(a, device):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(device)


def sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def stream_of(device):
    return torch.cuda.current_stream().cuda_stream if device != "cpu" else 0


class Batch:
    """One ragged batch in caller-owned, FILL-ed buffers: the pixel arena, the output pool with a guard in front of and behind every slot,
    descriptors packed here (not by image_ops), lengths and the flag word.  ``caps``: bytes per slot (default: the oracle's length)."""

    def __init__(self, lib, device, imgs, quals, subs, *, caps=None, max_blocks=None, expect=None):
        from img2img_turbo_amd import image_ops, ops as O
        self.lib, self.device, self.n = lib, device, len(imgs)
        self.expect = expect if expect is not None else [jpeg_ref.encode(a, q, s) for a, q, s in zip(imgs, quals, subs)]
        self.caps = caps if caps is not None else [len(e) for e in self.expect]
        self.desc = np.zeros(self.n, dtype=image_ops.JPEG_IMAGE_DTYPE)
        src_off, dst_off, arena = 0, GUARD, []
        for b, (a, q, s, cap) in enumerate(zip(imgs, quals, subs, self.caps)):
            h, w = a.shape[:2]
            c = 1 if a.ndim == 2 else a.shape[2]
            self.desc[b] = (src_off, dst_off, h, w, c, q, jpeg_ref.SUBSAMPLINGS[s], cap, (0, 0))
            flat = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
            arena.append(np.concatenate([flat, np.full((-flat.size) % 4, FILL, dtype=np.uint8)]))
            src_off += arena[-1].size
            dst_off += cap + GUARD
        self.blocks = max(image_ops.jpeg_blocks(a.shape[0], a.shape[1], s) for a, s in zip(imgs, subs))
        self.max_blocks = max_blocks or self.blocks
        self.arena = to_dev(np.concatenate(arena), device)
        self.pool = torch.full((dst_off,), FILL, dtype=torch.uint8, device=device)
        self.length = torch.full((self.n,), 77, dtype=torch.int32, device=device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=device)
        self.ws = torch.full((max(lib.jpeg_workspace_bytes(self.n, self.max_blocks), 16),), FILL, dtype=torch.uint8, device=device)   # needs no initialisation
        self.desc_dev = torch.zeros(self.n * 6, dtype=torch.int64, device=device)
        self.O = O

    def params(self):
        self.desc_dev.copy_(torch.from_numpy(self.desc.view(np.int64).reshape(-1).copy()))
        return self.O.jpeg_encode_u8(self.arena, self.pool, self.desc_dev, self.length, self.ws, n=self.n, max_blocks=self.max_blocks, bad_mask=self.bad)

    def run(self):
        p = self.params()
        self.lib.check(self.lib.lib.i2i_jpeg_encode_u8(C.addressof(p), 0, C.c_void_p(stream_of(self.device))))
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


def grid_of(h, w):
    return [(c, q, s) for c in CONTENTS for q in QUALITIES for s in SUBSAMPLINGS]


def check_grid(lib, device, h, w, contents=CONTENTS):
    """Contents x qualities x subsamplings at one size as ONE ragged call: every file equals the oracle's (and Pillow's), the guards hold."""
    cases = [(c, q, s) for c in contents for q in QUALITIES for s in SUBSAMPLINGS]
    expect = [want(c, h, w, q, s) for c, q, s in cases]
    b = Batch(lib, device, [image(c, h, w) for c, _, _ in cases], [q for _, q, _ in cases], [s for _, _, s in cases], expect=expect).run()
    b.check(what="%dx%d" % (h, w))
    if have_pillow_jpeg():
        for (c, q, s), got in zip(cases, b.files()):
            pil = pillow_bytes(image(c, h, w), q, s)
            assert got == pil, explain(got, pil, "device vs Pillow, %s %dx%d q%d %s" % (c, h, w, q, s))


RAGGED = [((8, 8), "noise", 75, "4:2:0"), ((17, 23), "binary", 100, "4:4:4"), ((24, 40), "ramp", 25, "4:2:0"), ((40, 24), "noise", 90, "4:4:4"),
          ((33, 16), "flat", 50, "4:2:0"), ((9, 50), "binary", 95, "4:2:0"), ((25, 7), "ramp", 1, "4:4:4"), ((64, 72), "noise", 100, "4:2:0")]


def check_ragged_batch(lib, device):
    """Eight images of eight sizes with their own qualities and subsamplings in one call == eight single-image calls == the oracle: the
    file of an image does not depend on its slot or on its neighbours.  Also through image_ops.jpeg_encode_u8, forwards and reversed."""
    from img2img_turbo_amd import image_ops
    imgs = [image(c, h, w) for (h, w), c, _, _ in RAGGED]
    quals, subs = [q for _, _, q, _ in RAGGED], [s for _, _, _, s in RAGGED]
    expect = [want(c, h, w, q, s) for (h, w), c, q, s in RAGGED]
    together = Batch(lib, device, imgs, quals, subs, expect=expect).run()
    together.check(what="ragged")
    files = together.files()
    for k in range(len(RAGGED)):
        alone = Batch(lib, device, imgs[k:k + 1], quals[k:k + 1], subs[k:k + 1], expect=expect[k:k + 1]).run()
        alone.check(what="alone %d" % k)
        assert alone.files()[0] == files[k]
    dev = [to_dev(a, device) for a in imgs]
    assert image_ops.jpeg_encode_u8(dev, quals, subs, lib=lib) == expect
    assert image_ops.jpeg_encode_u8(dev[::-1], quals[::-1], subs[::-1], lib=lib) == expect[::-1]
    # a stacked tensor with Pillow's defaults: what Image.save(f, "JPEG") with no arguments writes
    stack = np.stack([image("noise", 24, 40), image("ramp", 24, 40)])
    got = image_ops.jpeg_encode_u8(to_dev(stack, device), lib=lib)
    assert got == [jpeg_ref.encode(a) for a in stack]
    if have_pillow_jpeg():
        from PIL import Image
        for a, g in zip(stack, got):
            f = io.BytesIO()
            Image.fromarray(a).save(f, "JPEG")
            assert g == f.getvalue()
    # a grey source is replicated, as convert("RGB") does
    grey = image("noise", 17, 23)[:, :, :1]
    assert image_ops.jpeg_encode_u8([to_dev(grey, device)], 90, "4:4:4", lib=lib) == [jpeg_ref.encode(np.repeat(grey, 3, axis=2), 90, "4:4:4")]
    # return_tensors: the pool, the offsets, the lengths, no synchronisation inside
    pool, offs, lens, bad = image_ops.jpeg_encode_u8(dev, quals, subs, lib=lib, return_tensors=True)
    sync(device)
    assert int(bad.cpu()[0]) == 0
    assert [pool[o:o + int(l)].cpu().numpy().tobytes() for o, l in zip(offs, lens.cpu().tolist())] == expect


def check_grid_independence(lib, device):
    """The capacity hint sizes grids and workspace slots only: the smallest legal one and one 64 times larger give the same bytes."""
    imgs = [image(c, h, w) for (h, w), c, _, _ in RAGGED] + [image("noise", *BIG)]
    quals, subs = [q for _, _, q, _ in RAGGED] + [75], [s for _, _, _, s in RAGGED] + ["4:4:4"]
    res = []
    for scale in (1, 64):
        b = Batch(lib, device, imgs, quals, subs)
        b.max_blocks = b.blocks * scale
        b.ws = torch.full((lib.jpeg_workspace_bytes(b.n, b.max_blocks),), FILL, dtype=torch.uint8, device=device)
        b.run().check(what="max_blocks x%d" % scale)
        res.append(b.files())
    assert res[0] == res[1]


def check_overflow(lib, device):
    """A capacity one byte short of the file: the image's bit is set, its length is 0, NOTHING of its slot or of the guards around it is
    written, and the other images of the batch are the oracle's files."""
    from img2img_turbo_amd import _capi, image_ops
    imgs = [image(c, h, w) for (h, w), c, _, _ in RAGGED[:4]]
    quals, subs = [q for _, _, q, _ in RAGGED[:4]], [s for _, _, _, s in RAGGED[:4]]
    expect = [want(c, h, w, q, s) for (h, w), c, q, s in RAGGED[:4]]
    for victim in (0, 2):
        caps = [len(e) for e in expect]
        caps[victim] -= 1
        Batch(lib, device, imgs, quals, subs, caps=caps, expect=expect).run().check(flagged=(victim,), what="overflow %d" % victim)
    import pytest
    with pytest.raises(_capi.I2IError) as e:
        image_ops.jpeg_encode_u8([to_dev(a, device) for a in imgs], quals, subs, lib=lib, capacity=[len(x) for x in expect[:2]] + [len(expect[2]) - 1, len(expect[3])])
    assert "image 2" in str(e.value)


REJECTS = ["an offset beyond the arena", "w = 0", "h beyond 65535", "a slot beyond the pool", "more blocks than max_blocks", "five channels"]


def check_rejection(lib, device, what):
    """EMULATOR ONLY (the GPU tests use valid descriptors): image 1 of four has a wrong descriptor.  It is flagged, gets length 0, nothing
    of the pool is written for it, and its neighbours are the oracle's files."""
    imgs = [image(c, h, w) for (h, w), c, _, _ in RAGGED[:4]]
    quals, subs = [q for _, _, q, _ in RAGGED[:4]], [s for _, _, _, s in RAGGED[:4]]
    b = Batch(lib, device, imgs, quals, subs)
    d = b.desc
    if what == "an offset beyond the arena":
        d["src_off"][1] = b.arena.numel() - 16
    elif what == "w = 0":
        d["w"][1] = 0
    elif what == "h beyond 65535":
        d["h"][1] = 65536
    elif what == "a slot beyond the pool":
        d["dst_off"][1] = b.pool.numel() - 8
    elif what == "more blocks than max_blocks":
        d["h"][1], d["w"][1] = 1, 8 * b.max_blocks               # (inside the arena: one row of pixels; too many blocks for the workspace slot)
        b.arena = torch.cat([b.arena, torch.zeros(3 * 8 * b.max_blocks, dtype=torch.uint8, device=b.arena.device)])
    elif what == "five channels":
        d["c"][1] = 5
    else:
        raise AssertionError(what)
    b.run().check(flagged=(1,), what=what)


def check_bad_args(lib, device):
    """Every host-side error of the contract returns I2I_ERR_BAD_ARG with a message and launches nothing; n == 0 is a successful no-op."""
    b = Batch(lib, device, [image("noise", 8, 8)], [75], ["4:2:0"])
    entry = lib.lib.i2i_jpeg_encode_u8
    p = b.params()
    for kw in (dict(src=0), dict(dst=0), dict(images=0), dict(length=0), dict(ws=0), dict(src=p.src + 2), dict(length=p.length + 2), dict(bad_mask=p.bad_mask + 1),
               dict(images=p.images + 4), dict(ws=p.ws + 8), dict(n=-1), dict(max_blocks=0), dict(max_blocks=(1 << 21) + 1), dict(src_bytes=-1),
               dict(dst_bytes=-1), dict(ws_bytes=p.ws_bytes - 1)):
        q = b.params()
        for k, v in kw.items():
            setattr(q, k, v)
        assert entry(C.addressof(q), 0, C.c_void_p(stream_of(device))) == -1, kw
        msg = lib.lib.i2i_last_error().decode()
        assert msg.startswith("jpeg_encode_u8:") and len(msg) > 16, (kw, msg)
    assert entry(None, 0, C.c_void_p(stream_of(device))) == -1
    q = b.params()
    q.n = 0
    assert entry(C.addressof(q), 0, C.c_void_p(stream_of(device))) == 0
    sync(device)
    assert (b.pool.cpu().numpy() == FILL).all() and b.mask() == 0
    assert lib.jpeg_workspace_bytes(1, 0) == 0 and lib.jpeg_workspace_bytes(-1, 8) == 0 and lib.jpeg_workspace_bytes(2, 8) == 2 * lib.jpeg_workspace_bytes(1, 8) > 0


# ---------------------------------------------------------------------------------------------------------------- the ABI and the host code
def check_abi(lib):
    """Additive: the version is 14, sizeof(i2i_op) did not grow, no opcode was added, the new symbols are there, the descriptor is 48 bytes
    in both bindings."""
    from img2img_turbo_amd import _capi as K, image_ops
    assert lib.lib.i2i_sizeof_op() == C.sizeof(K.Op) == PARENT_SIZEOF_OP
    assert lib.lib.i2i_abi_version() == K.ABI_VERSION == 14
    assert max(v for k, v in vars(K).items() if k.startswith("OP_") and isinstance(v, int)) == K.OP_TILE_BLEND_U8 == 28
    for name in ("i2i_jpeg_encode_u8", "i2i_jpeg_workspace_bytes", "i2i_jpeg_header"):
        assert hasattr(lib.lib, name) and name in K.EXPORTS
    assert C.sizeof(K.JpegImage) == 48 == image_ops.JPEG_IMAGE_DTYPE.itemsize
    assert ([image_ops.JPEG_IMAGE_DTYPE.fields[n][1] for n, _ in K.JpegImage._fields_] == [getattr(K.JpegImage, n).offset for n, _ in K.JpegImage._fields_])


def check_header(lib):
    """i2i_jpeg_header (plain host code) == the oracle's header, every quality, both subsamplings; and its refusals."""
    for q in list(range(1, 101)) + [0, -5, 101, 1000]:
        for s in SUBSAMPLINGS:
            for w, h in ((1, 1), (23, 17), (65535, 65535), (512, 300)):
                assert lib.jpeg_header(q, jpeg_ref.SUBSAMPLINGS[s], w, h) == jpeg_ref.header(q, s, w, h), (q, s, w, h)
    out = (C.c_uint8 * 623)(*([77] * 623))
    for args in ((75, 1, 8, 8), (75, 0, 0, 8), (75, 0, 8, 65536), (75, 2, -1, 8)):
        assert lib.lib.i2i_jpeg_header(*args, C.addressof(out)) == -1 and all(v == 77 for v in out), args
        assert lib.lib.i2i_last_error().decode().startswith("jpeg_header:")
    assert lib.lib.i2i_jpeg_header(75, 0, 8, 8, None) == -1


# ---------------------------------------------------------------------------------------------------------------- the models
def check_forward_jpeg(lib, device, kind, dtype=torch.float32, light=False):
    """forward_u8(jpeg=...) on the tiny synthetic model: the files decode with Pillow and equal jpeg_encode_u8 of the uint8 output of the same
    call without jpeg= -- plain, with per-image (quality, subsampling), with variations=2 (pix2pix), with tile= on two requests of different
    sizes (each request encoded at its own size), and beside return_edges=True.  ``light`` (the emulator, where a forward is a minute): the
    plain call against one per-image list and the refusals only."""
    import tile_cases as tc
    from img2img_turbo_amd import image_ops
    model = tc.make_pix2pix(lib, device, dtype) if kind == "pix2pix" else tc.make_cyclegan(lib, device, dtype)
    try:
        cap = tc.caption(device)
        base = dict(caption_enc=cap) if kind == "pix2pix" else dict(direction="a2b", caption_emb=cap)
        x = torch.stack([tc.to_dev(tc.photo(32, 40, i), device) for i in range(2)])
        eps = torch.randn(2, 4, 4, 5, generator=torch.Generator().manual_seed(3)).to(device)

        def decoded(files, shapes):
            if have_pillow_jpeg():
                from PIL import Image
                for f, (h, w) in zip(files, shapes):
                    im = Image.open(io.BytesIO(f))
                    im.load()
                    assert im.size == (w, h) and im.mode == "RGB"

        import pytest
        for bad in ([90], "high", (90, "4:2:2"), 3.5):                            # refused before any forward runs
            with pytest.raises(ValueError):
                model.forward_u8(x, eps=eps, jpeg=bad, **base)
        assert not model._plans
        plain = model.forward_u8(x, eps=eps, **base)
        for jpeg, (quals, subs) in (((True, (75, "4:2:0")), (90, (90, "4:2:0")), ((50, "4:4:4"), (50, "4:4:4"))) if not light else ()) + (
                                    ([(95, "4:4:4"), 30], ([95, 30], ["4:4:4", "4:2:0"])),):
            files = model.forward_u8(x, eps=eps, jpeg=jpeg, **base)
            assert isinstance(files, list) and len(files) == 2 and all(isinstance(f, bytes) for f in files)
            assert files == image_ops.jpeg_encode_u8(plain, quals, subs, lib=lib), jpeg
            decoded(files, [(32, 40)] * 2)
        assert files != image_ops.jpeg_encode_u8(plain, lib=lib)                  # (the settings reach the encoder)
        if light:
            return
        if kind == "pix2pix":
            out = model.forward_u8(x, seed=[[1, 2], [3, 4]], variations=2, **base)
            files = model.forward_u8(x, seed=[[1, 2], [3, 4]], variations=2, jpeg=[80, (60, "4:4:4")], **base)
            assert out.shape[0] == 4 and len(files) == 4                           # image-major: entry b serves slots b * V .. b * V + V - 1
            assert files == image_ops.jpeg_encode_u8(out, [80, 80, 60, 60], ["4:2:0", "4:2:0", "4:4:4", "4:4:4"], lib=lib)
            decoded(files, [(32, 40)] * 4)
            out, edges = model.forward_u8(x, eps=eps, canny=(100, 200), return_edges=True, **base)
            files, edges2 = model.forward_u8(x, eps=eps, canny=(100, 200), return_edges=True, jpeg=85, **base)
            assert torch.equal(edges, edges2) and files == image_ops.jpeg_encode_u8(out, 85, lib=lib)
        reqs = [tc.to_dev(tc.photo(h, w, 5 + i), device) for i, (h, w) in enumerate([(56, 72), (32, 40)])]
        kw = dict(tile=tc.MODEL_TILE, tile_overlap=8, tile_batch=4, seed=[7, 8], **base)
        outs = model.forward_u8(reqs, **kw)
        files = model.forward_u8(reqs, jpeg=[(90, "4:2:0"), (75, "4:4:4")], **kw)
        assert [tuple(o.shape) for o in outs] == [(56, 72, 3), (32, 40, 3)] and len(files) == 2
        assert files == image_ops.jpeg_encode_u8(outs, [90, 75], ["4:2:0", "4:4:4"], lib=lib)
        assert files == [jpeg_ref.encode(o.cpu().numpy(), q, s) for o, q, s in zip(outs, [90, 75], ["4:2:0", "4:4:4"])]
        decoded(files, [(56, 72), (32, 40)])
    finally:
        model.release_plans()

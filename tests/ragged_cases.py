"""Cases and backend-independent checks shared by tests/test_ragged_emu.py (CPU emulator) and tests/test_ragged_gpu.py (MI355X): the ragged
LANCZOS resize -- i2i_resize_u8_ragged and i2i_lanczos_tables (csrc/resize.hip, the contract is the comment of i2i_resize_u8_ragged_params
in include/i2i_turbo.h), image_ops.lanczos_resize_u8_ragged and the list forms of the two models' forward_u8.

Two oracles, both bit-exact: the existing single-size path (image_ops.lanczos_resize_u8 on each image alone, same library) for c = 1 .. 4,
and Pillow itself (Image.resize(size, Image.LANCZOS)) for c = 1 ("L") and c = 3 ("RGB").  "RGBA" is no oracle for c = 4: Pillow premultiplies
alpha.  Every comparison is np.array_equal: integer arithmetic has no tolerance."""
import ctypes as C

import numpy as np
import torch

# ragged in, c = 3, sources (h, w) -> width 24, height 16
SRC_HW = [(5, 7),        # 105 bytes: the next image's offset is padded to 108
          (16, 24),      # identity in both passes
          (16, 50),      # identity vertically only
          (40, 24),      # identity horizontally only
          (33, 64), (64, 33),      # mixed downscales
          (3, 100),      # up vertically, 4x down horizontally
          (1, 1)]        # the smallest image
TARGET = (24, 16)        # (width, height), as PIL takes it
OTHER_C_HW = [(5, 7), (16, 24), (33, 64)]                  # the c = 1 and c = 4 batches
REAL_HW = [(720, 1280), (561, 843), (512, 512)]            # the realistic GPU case, to 512 x 512 and back
TABLE_PAIRS = [(7, 24), (24, 7), (561, 560), (1280, 512), (512, 1280), (4096, 16), (16, 4096), (1, 1), (512, 512)]
FILL = 0xA5
TAIL = 64                # bytes behind the last image in the arenas the write-bound checks allocate
PARENT_SIZEOF_OP = 368


def image(h, w, c, seed):
    """uint8 [h, w, c]: noise on even seeds, hard 0 / 255 blocks on odd ones (LANCZOS overshoots there: both ends of clip8)."""
    rng = np.random.RandomState(1000 + seed)
    if seed % 2 == 0:
        return rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    blocks = rng.randint(0, 2, ((h + 2) // 3, (w + 2) // 3, c)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 3, axis=0), 3, axis=1)[:h, :w])


def images(hw, c):
    return [image(h, w, c, i) for i, (h, w) in enumerate(hw)]


def to_dev(a, device):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(device)           # (a copy: a slice of a batch may start off a dword)


def sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def stream_of(device):
    return torch.cuda.current_stream().cuda_stream if device != "cpu" else 0


def pillow(a, size):
    """Image.resize(size, LANCZOS) of an [h, w, 1] / [h, w, 3] array."""
    from PIL import Image
    c = a.shape[-1]
    assert c in (1, 3)
    im = Image.fromarray(a[..., 0], "L") if c == 1 else Image.fromarray(a, "RGB")
    return np.asarray(im.resize(size, Image.LANCZOS)).reshape(size[1], size[0], c)


_SINGLE = {}


def single(lib, device, a, size):
    """The existing path on one image alone (computed once per library, image and size; never modified)."""
    from img2img_turbo_amd import image_ops
    key = (lib.path, a.shape, a.tobytes(), tuple(size))
    if key not in _SINGLE:
        got = image_ops.lanczos_resize_u8(to_dev(a[None], device), size, lib=lib)[0].cpu().numpy().copy()
        got.setflags(write=False)
        _SINGLE[key] = got
    return _SINGLE[key]


def check_against_oracles(lib, device, srcs, sizes, got):
    """got[b] (numpy) == lanczos_resize_u8 on image b alone == Pillow (c = 1, 3)."""
    for b, (a, size) in enumerate(zip(srcs, sizes)):
        assert got[b].shape == (size[1], size[0], a.shape[-1]), (b, got[b].shape)
        want = single(lib, device, a, size)
        assert np.array_equal(got[b], want), ("lanczos_resize_u8", b, a.shape, size, int((got[b] != want).sum()))
        if a.shape[-1] in (1, 3):
            ref = pillow(a, size)
            assert np.array_equal(got[b], ref), ("pillow", b, a.shape, size, int((got[b] != ref).sum()))


# ---------------------------------------------------------------------------------------------------------------- the ABI
def check_struct_size(lib):
    from img2img_turbo_amd import _capi as K
    assert lib.lib.i2i_sizeof_op() == C.sizeof(K.Op) == PARENT_SIZEOF_OP
    assert C.sizeof(K.ResizeImage) == 48 and C.sizeof(K.ResizeU8RaggedParams) <= C.sizeof(K.IgemmParams)
    assert lib.lib.i2i_abi_version() == K.ABI_VERSION == 14 and K.OP_RESIZE_U8_RAGGED == 21
    from img2img_turbo_amd import image_ops
    assert image_ops.RAGGED_IMAGE_DTYPE.itemsize == 48
    assert [image_ops.RAGGED_IMAGE_DTYPE.fields[n][1] for n, _ in K.ResizeImage._fields_] == [getattr(K.ResizeImage, n).offset for n, _ in K.ResizeImage._fields_]


# ---------------------------------------------------------------------------------------------------------------- tables
def check_tables(lib, pair):
    """i2i_lanczos_ksize / i2i_lanczos_tables (host code of the library) == image_ops.lanczos_coeffs, bit for bit; a larger row capacity pads
    with zeros; the error cases write nothing."""
    from img2img_turbo_amd import image_ops
    n_in, n_out = pair
    ksize, bounds, coeffs = image_ops.lanczos_coeffs(n_in, n_out)
    assert lib.lib.i2i_lanczos_ksize(n_in, n_out) == ksize
    got_k, got_b, got_c = lib.lanczos_tables(n_in, n_out)
    assert got_k == ksize and got_b.dtype == np.int32 and got_c.dtype == np.int32
    assert np.array_equal(got_b, bounds), pair
    assert np.array_equal(got_c, coeffs), (pair, int((got_c != coeffs).sum()))
    if n_out <= 512:
        wide_k, wide_b, wide_c = lib.lanczos_tables(n_in, n_out, ksize + 3)
        assert wide_k == ksize and np.array_equal(wide_b, bounds) and np.array_equal(wide_c[:, :ksize], coeffs) and not wide_c[:, ksize:].any()


def check_tables_errors(lib):
    b = np.full((4, 2), 77, dtype=np.int32)
    c = np.full((4, 16), 77, dtype=np.int32)
    f = lib.lib.i2i_lanczos_tables
    assert lib.lib.i2i_lanczos_ksize(0, 4) == -1 and lib.lib.i2i_lanczos_ksize(4, 0) == -1 and lib.lib.i2i_lanczos_ksize(-3, 4) == -1
    assert lib.lib.i2i_lanczos_ksize(8, 4) == 13 and lib.lib.i2i_lanczos_ksize(4, 8) == 7
    for args in ((8, 4, None, c.ctypes.data, 16), (8, 4, b.ctypes.data, None, 16), (0, 4, b.ctypes.data, c.ctypes.data, 16),
                 (8, 0, b.ctypes.data, c.ctypes.data, 16), (8, 4, b.ctypes.data, c.ctypes.data, 12)):
        assert f(*args) == -1, args
        assert lib.lib.i2i_last_error().decode().startswith("lanczos_"), args
        assert (b == 77).all() and (c == 77).all(), args
    assert f(8, 4, b.ctypes.data, c.ctypes.data, 16) == 13 and not (b == 77).any()


def check_identity_tables():
    """Pillow's same-size table is an exact identity: one tap of weight 2^22 on the coordinate itself (why an image that changes along
    one axis only may run both passes)."""
    from img2img_turbo_amd import image_ops
    for n in (1, 2, 16, 24, 513):
        ksize, bounds, coeffs = image_ops.lanczos_coeffs(n, n)
        for o in range(n):
            first, cnt = bounds[o]
            row = np.zeros(n, dtype=np.int64)
            row[first:first + cnt] = coeffs[o, :cnt]
            assert row[o] == 1 << 22 and row.sum() == 1 << 22 and not coeffs[o, cnt:].any(), (n, o)


# ---------------------------------------------------------------------------------------------------------------- the eager form
def check_ragged_in(lib, device):
    """Eight sources of eight sizes -> one stacked [8, 16, 24, 3]."""
    from img2img_turbo_amd import image_ops
    srcs = images(SRC_HW, 3)
    got = image_ops.lanczos_resize_u8_ragged([to_dev(a, device) for a in srcs], TARGET, lib=lib)
    assert torch.is_tensor(got) and got.dtype == torch.uint8 and got.shape == (len(srcs), TARGET[1], TARGET[0], 3) and got.is_contiguous()
    check_against_oracles(lib, device, srcs, [TARGET] * len(srcs), got.cpu().numpy())
    return got


def check_ragged_out(lib, device):
    """A stacked [8, 16, 24, 3] back to the eight sizes -> a list."""
    from img2img_turbo_amd import image_ops
    batch = np.stack(images([(TARGET[1], TARGET[0])] * len(SRC_HW), 3))
    sizes = [(w, h) for h, w in SRC_HW]
    got = image_ops.lanczos_resize_u8_ragged(to_dev(batch, device), sizes, lib=lib)
    assert isinstance(got, list) and len(got) == len(SRC_HW)
    check_against_oracles(lib, device, list(batch), sizes, [g.cpu().numpy() for g in got])
    # a stacked input whose images are not a multiple of 4 bytes takes the packing path; a list of sizes of the wrong length is refused
    import pytest
    odd = np.stack(images([(5, 7)] * 2, 3))
    got = image_ops.lanczos_resize_u8_ragged(to_dev(odd, device), (3, 5), lib=lib)           # 45 bytes per output: not an arena view
    assert got.shape == (2, 5, 3, 3)
    check_against_oracles(lib, device, list(odd), [(3, 5)] * 2, got.cpu().numpy())
    with pytest.raises(ValueError):
        image_ops.lanczos_resize_u8_ragged(to_dev(odd, device), [(3, 5)], lib=lib)
    with pytest.raises(ValueError):
        image_ops.lanczos_resize_u8_ragged([to_dev(odd[0], device), to_dev(odd[1][..., :1], device)], (3, 5), lib=lib)


def check_channels(lib, device, c):
    from img2img_turbo_amd import image_ops
    srcs = images(OTHER_C_HW, c)
    got = image_ops.lanczos_resize_u8_ragged([to_dev(a, device) for a in srcs], TARGET, lib=lib)
    check_against_oracles(lib, device, srcs, [TARGET] * len(srcs), got.cpu().numpy())
    back = image_ops.lanczos_resize_u8_ragged(got, [(w, h) for h, w in OTHER_C_HW], lib=lib)
    host = got.cpu().numpy()
    check_against_oracles(lib, device, list(host), [(w, h) for h, w in OTHER_C_HW], [g.cpu().numpy() for g in back])


# ---------------------------------------------------------------------------------------------------------------- the raw entry
class Request:
    """One ragged resize laid out in caller-owned, FILL-ed arenas (what a host with fixed-capacity buffers does)."""

    def __init__(self, lib, device, srcs, sizes, c, *, capacity=None, tables_of=None):
        from img2img_turbo_amd import image_ops
        self.lib, self.device, self.srcs, self.sizes, self.c = lib, device, srcs, sizes, c
        self.layout = L = image_ops.ragged_layout([a.shape[:2] for a in srcs], sizes, c, tables_of=tables_of or lib.lanczos_tables)
        cap = capacity or dict(src=L.src_bytes + TAIL, mid=L.mid_bytes + TAIL, dst=L.dst_bytes + TAIL, tables=L.tables.size, n=L.n)
        assert L.n <= cap["n"] and L.src_bytes <= cap["src"] and L.mid_bytes <= cap["mid"] and L.dst_bytes <= cap["dst"] and L.tables.size <= cap["tables"]
        self.cap = cap
        self.src = torch.full((cap["src"],), FILL, dtype=torch.uint8, device=device)
        self.mid = torch.full((cap["mid"],), FILL, dtype=torch.uint8, device=device)
        self.dst = torch.full((cap["dst"],), FILL, dtype=torch.uint8, device=device)
        self.desc = torch.zeros(2 * cap["n"] * 6, dtype=torch.int64, device=device)
        self.tables = torch.zeros(cap["tables"], dtype=torch.int32, device=device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=device)
        self.write(L, srcs)

    def write(self, layout, srcs, desc=None):
        """Descriptors (padded with empty slots up to the capacity), tables and pixels, in place."""
        from img2img_turbo_amd import image_ops
        self.layout, self.srcs = layout, srcs
        n = self.cap["n"]
        d = np.zeros((2, n), dtype=image_ops.RAGGED_IMAGE_DTYPE)
        d[:, :layout.n] = layout.desc if desc is None else desc
        self.desc.copy_(torch.from_numpy(d.view(np.int64).reshape(-1).copy()))
        self.tables[:layout.tables.size].copy_(torch.from_numpy(layout.tables.copy()))
        host = np.full(self.cap["src"], FILL, dtype=np.uint8)
        for a, off in zip(srcs, layout.src_off.tolist()):
            host[off:off + a.size] = a.reshape(-1)
        self.src.copy_(torch.from_numpy(host))
        self.host_desc = d

    def ops(self, units=None):
        from img2img_turbo_amd import ops as O
        uh, uv = units or (self.layout.units_h, self.layout.units_v)
        n = self.cap["n"]
        return [O.resize_u8_ragged(self.src, self.mid, self.desc, self.tables, n=n, c=self.c, axis=1, grid_units=uh, bad_mask=self.bad),
                O.resize_u8_ragged(self.mid, self.dst, self.desc, self.tables, n=n, c=self.c, axis=0, grid_units=uv, bad_mask=self.bad, first_image=n)]

    def run(self, units=None):
        for _, p in self.ops(units):
            self.lib.check(self.lib.lib.i2i_resize_u8_ragged(C.addressof(p), 0, C.c_void_p(stream_of(self.device))))
        sync(self.device)
        return self

    def results(self):
        """(mid arena, dst arena, bad mask) on the host."""
        return self.mid.cpu().numpy(), self.dst.cpu().numpy(), int(self.bad.cpu().numpy().view(np.uint32)[0])

    def check(self, skipped=()):
        """Every image not in ``skipped`` equals the oracles; every other byte of both result arenas -- skipped images, the padding between
        images, the tail -- still holds FILL."""
        mid, dst, _ = self.results()
        L = self.layout
        untouched_mid, untouched_dst = np.ones(mid.size, dtype=bool), np.ones(dst.size, dtype=bool)
        got, srcs, sizes = [], [], []
        for b, (a, (ow, oh)) in enumerate(zip(self.srcs, self.sizes)):
            if b in skipped:
                continue
            h = a.shape[0]
            mo, do = int(L.mid_off[b]), int(L.dst_off[b])
            untouched_mid[mo:mo + h * ow * self.c] = False
            untouched_dst[do:do + oh * ow * self.c] = False
            got.append(dst[do:do + oh * ow * self.c].reshape(oh, ow, self.c))
            srcs.append(a)
            sizes.append((ow, oh))
        assert (mid[untouched_mid] == FILL).all(), ("mid", np.flatnonzero(untouched_mid & (mid != FILL))[:8])
        assert (dst[untouched_dst] == FILL).all(), ("dst", np.flatnonzero(untouched_dst & (dst != FILL))[:8])
        check_against_oracles(self.lib, self.device, srcs, sizes, got)


def first_request(lib, device, **kw):
    return Request(lib, device, images(SRC_HW, 3), [TARGET] * len(SRC_HW), 3, **kw)


def check_write_bounds(lib, device):
    """The eight images through the raw entry in FILL-ed arenas with a tail: padding and tail untouched.  Then slot 4 emptied (hin = 0 in
    both passes, the other fields left as they were): its bytes stay FILL too, nobody is flagged."""
    r = first_request(lib, device).run()
    r.check()
    assert r.results()[2] == 0
    assert int(r.layout.src_off[1]) == 108                                       # (5 * 7 * 3 = 105 bytes padded)
    e = first_request(lib, device)
    d = e.layout.desc.copy()
    d["hin"][:, 4] = 0
    e.write(e.layout, e.srcs, desc=d)
    e.run().check(skipped=(4,))
    assert e.results()[2] == 0
    w = first_request(lib, device)                                               # win = 0 is an empty slot as well
    d = w.layout.desc.copy()
    d["win"][:, 6] = 0
    w.write(w.layout, w.srcs, desc=d)
    w.run().check(skipped=(6,))
    assert w.results()[2] == 0


def check_grid_independence(lib, device):
    """grid_units = 1 (one workgroup per image striding over everything) and the exact unit count: the same bytes."""
    a = first_request(lib, device).run(units=(1, 1))
    b = first_request(lib, device).run()
    c = first_request(lib, device).run(units=(1 << 40, 1 << 40))                 # (the grid is capped)
    a.check()
    for other in (b, c):
        assert np.array_equal(a.results()[0], other.results()[0]) and np.array_equal(a.results()[1], other.results()[1])


def check_python_tables_too(lib, device):
    """The same request with image_ops.lanczos_coeffs as the table source (the two are bit-equal, so are the images)."""
    from img2img_turbo_amd import image_ops
    first_request(lib, device, tables_of=image_ops.lanczos_coeffs).run().check()


SECOND_HW = [(9, 31), (24, 16), (2, 2), (47, 5), (16, 24)]
SECOND_TARGET = (20, 12)


def check_graph(lib, device):
    """One captured graph over the two passes with fixed-capacity buffers serves two requests: launch, rewrite descriptors, tables and
    pixels in place for other sizes (and fewer images: the rest become empty slots), launch again."""
    from img2img_turbo_amd import _capi as K, image_ops
    cap = dict(src=64 << 10, mid=64 << 10, dst=64 << 10, tables=16 << 10, n=8)
    r = first_request(lib, device, capacity=cap)
    prog = K.Program()
    for i, (opcode, params) in enumerate(r.ops(units=(64 * 64, 64 * 64))):
        prog.add(opcode, K.F32, params, "ragged.%s" % "hv"[i])
    prog.freeze()
    g = lib.graph_create(prog)
    try:
        lib.graph_launch(g, stream_of(device))
        sync(device)
        r.check()
        srcs = images(SECOND_HW, 3)
        sizes = [SECOND_TARGET] * len(srcs)
        layout = image_ops.ragged_layout([a.shape[:2] for a in srcs], sizes, 3, tables_of=lib.lanczos_tables)
        r.mid.fill_(FILL)
        r.dst.fill_(FILL)
        r.sizes = sizes
        r.write(layout, srcs)
        lib.graph_launch(g, stream_of(device))
        sync(device)
        r.check()
        assert r.results()[2] == 0
    finally:
        sync(device)
        lib.graph_destroy(g)
    # the same program through i2i_run (capi.hip's dispatch)
    r.mid.fill_(FILL)
    r.dst.fill_(FILL)
    lib.run(prog, stream_of(device))
    sync(device)
    r.check()


# ---------------------------------------------------------------------------------------------------------------- errors
def call(lib, device, r, **kw):
    """i2i_resize_u8_ragged (horizontal pass of request r) with fields overridden; returns the status."""
    p = r.ops()[0][1]
    null = kw.pop("null_params", False)
    for k, v in kw.items():
        setattr(p, k, v)
    status = lib.lib.i2i_resize_u8_ragged(None if null else C.addressof(p), 0, C.c_void_p(stream_of(device)))
    sync(device)
    return status


def check_bad_args(lib, device):
    """Every host-side error of the contract returns I2I_ERR_BAD_ARG with a message and launches nothing; n == 0 is a successful no-op."""
    import pytest
    from img2img_turbo_amd import _capi as K
    r = first_request(lib, device)
    p = r.ops()[0][1]
    bad = [dict(null_params=True), dict(src=0), dict(dst=0), dict(images=0), dict(tables=0),
           dict(src=p.src + 2), dict(dst=p.dst + 1), dict(tables=p.tables + 2), dict(images=p.images + 4), dict(bad_mask=p.bad_mask + 2),
           dict(c=0), dict(c=5), dict(n=-1), dict(axis=2), dict(axis=-1), dict(grid_units=0), dict(grid_units=-5),
           dict(src_bytes=-1), dict(dst_bytes=-1), dict(tables_len=-1)]
    for kw in bad:
        status = call(lib, device, r, **kw)
        assert status == -1, (kw, status)
        msg = lib.lib.i2i_last_error().decode()
        assert msg.startswith("resize_u8_ragged:") and len(msg) > len("resize_u8_ragged: "), (kw, msg)
        with pytest.raises(K.I2IError):
            lib.check(status)
    assert call(lib, device, r, n=0) == 0 and call(lib, device, r, n=0, src=0, dst=0, images=0, tables=0) == 0
    mid, dst, mask = r.results()
    assert (mid == FILL).all() and (dst == FILL).all() and mask == 0


REJECTS = ["dst_off past dst_bytes", "unaligned src_off", "bounds_off past tables_len", "coeffs_off past tables_len", "negative hin",
           "a table entry past the source", "a tap count above ksize"]


def check_rejection(lib, device, what):
    """EMULATOR ONLY (the GPU tests use valid descriptors): image 2's descriptor or table is wrong.  Its destination stays FILL in both
    passes' arenas, its bit is set in bad_mask, the other images are bit-exact."""
    r = first_request(lib, device)
    L = r.layout
    d = L.desc.copy()
    tables = L.tables.copy()
    victims = (2,)
    if what == "dst_off past dst_bytes":
        d["dst_off"][1, 2] = (r.cap["dst"] & ~3) - 8            # the vertical pass's 16 * 24 * 3 bytes do not fit behind it
        d["dst_off"][0, 2] = (r.cap["mid"] & ~3) + 4            # the horizontal pass: starts behind the arena
    elif what == "unaligned src_off":
        d["src_off"][:, 2] += 2
    elif what == "bounds_off past tables_len":
        d["bounds_off"][:, 2] = r.cap["tables"] - 1
    elif what == "coeffs_off past tables_len":
        d["coeffs_off"][:, 2] = r.cap["tables"] - 3
    elif what == "negative hin":
        d["hin"][:, 2] = -16
    elif what == "a table entry past the source":
        # the horizontal table of image 2 (50 -> 24) is its own (no other image has that pair): last row's first tap moved past the row
        tables[int(d["bounds_off"][0, 2]) + 2 * 23] = 1 << 20
    elif what == "a tap count above ksize":
        tables[int(d["bounds_off"][0, 2]) + 2 * 5 + 1] = int(d["ksize"][0, 2]) + 1
    else:
        raise AssertionError(what)
    L = L._replace(tables=tables)
    r.write(L, r.srcs, desc=d)
    r.run()
    mid, dst, mask = r.results()
    assert mask == 1 << 2, (what, hex(mask))
    if what.startswith("a t"):
        # only the horizontal pass is rejected: the vertical pass then resizes the FILL bytes the first left -- valid work on stale pixels,
        # so image 2's final bytes are not checked; its mid bytes must be FILL
        mo = int(r.layout.mid_off[2])
        assert (mid[mo:mo + 16 * 24 * 3] == FILL).all(), what
        do = int(r.layout.dst_off[2])
        dst[do:do + 16 * 24 * 3] = FILL
        r.dst.copy_(torch.from_numpy(dst))
    r.check(skipped=victims)


# ---------------------------------------------------------------------------------------------------------------- the models
MODEL_HW = [(20, 31), (16, 24), (37, 18)]
MODEL_SIZE = (24, 16)


def check_pix2pix_list(lib, device, size=MODEL_SIZE):
    """forward_u8([three sizes], resize=(w, h)) == forward_u8(stack of the three lanczos_resize_u8 results), bit for bit; the list forms
    without a common size raise."""
    import pytest
    import randn_cases as rc
    from img2img_turbo_amd import image_ops
    model = rc.make_model(lib, device, False)
    try:
        srcs = images(MODEL_HW, 3)
        devs = [to_dev(a, device) for a in srcs]
        _, cap = rc.pipeline_inputs(1, device, size[1], size[0])
        eps = torch.randn(len(srcs), 4, size[1] // 8, size[0] // 8, generator=torch.Generator().manual_seed(3)).to(device)
        out = model.forward_u8(devs, caption_enc=cap, eps=eps, resize=size)
        stack = torch.cat([image_ops.lanczos_resize_u8(t[None], size, lib=lib) for t in devs])
        want = model.forward_u8(stack, caption_enc=cap, eps=eps)
        assert out.shape == (len(srcs), size[1], size[0], 3) and out.dtype == torch.uint8 and torch.equal(out, want)
        assert len(set(out.cpu().numpy().reshape(-1).tolist())) > 2                 # (not a constant image)
        with pytest.raises(ValueError):
            model.forward_u8(devs, caption_enc=cap, eps=eps, resize="multiple_of_8")
        with pytest.raises(ValueError):
            model.forward_u8(devs, caption_enc=cap, eps=eps)
    finally:
        model.release_plans()


def check_cyclegan_list(lib, device, size=MODEL_SIZE):
    """CycleGAN forward_u8(list, resize=..., resize_back=True) returns a list, element b == lanczos_resize_u8(out[b:b+1], size_b); the
    image_prep spelling of the same size gives the same; resized_crop_512 / no size raise."""
    import pytest
    from oracle import TINY_UNET, TINY_VAE
    from oracle.synth import make_cyclegan_weights
    from img2img_turbo_amd import image_ops
    from img2img_turbo_amd.cyclegan_turbo import CycleGAN_Turbo
    from img2img_turbo_amd.weights import GeneratorWeights
    mw = make_cyclegan_weights(TINY_UNET, TINY_VAE, rank_unet=16)
    gw = GeneratorWeights(mw.unet, mw.vae, mw.unet_arch, mw.vae_arch, mw.unet_scaling, mw.vae_scaling, mw.vae_b2a)
    model = CycleGAN_Turbo(weights=gw, device=device, dtype=torch.float32, lib=lib)
    try:
        srcs = images(MODEL_HW, 3)
        devs = [to_dev(a, device) for a in srcs]
        g = torch.Generator().manual_seed(4)
        cap = torch.randn(1, 77, TINY_UNET.cross_attention_dim, generator=g).to(device)
        eps = torch.randn(len(srcs), 4, size[1] // 8, size[0] // 8, generator=g).to(device)
        kw = dict(direction="a2b", caption_emb=cap, eps=eps)
        outs = model.forward_u8(devs, resize=size, resize_back=True, **kw)
        assert isinstance(outs, list) and len(outs) == len(srcs)
        stack = torch.cat([image_ops.lanczos_resize_u8(t[None], size, lib=lib) for t in devs])
        mid = model.forward_u8(stack, **kw)
        assert torch.equal(model.forward_u8(devs, resize=size, **kw), mid)          # without resize_back: the stacked batch
        for b, (h, w) in enumerate(MODEL_HW):
            want = image_ops.lanczos_resize_u8(mid[b:b + 1].clone(), (w, h), lib=lib)[0]
            assert outs[b].shape == (h, w, 3) and torch.equal(outs[b], want), b
        with pytest.raises(ValueError):
            model.forward_u8(devs, image_prep="resized_crop_512", resize_back=True, **kw)
        with pytest.raises(ValueError):
            model.forward_u8(devs, resize_back=True, **kw)
        with pytest.raises(ValueError):
            model.forward_u8(devs, image_prep="no_resize", **kw)
    finally:
        model.release_plans()

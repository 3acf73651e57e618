"""Cases and backend-independent checks shared by tests/test_tile_emu.py (CPU emulator) and tests/test_tile_gpu.py (MI355X): the tiled
forward's two ends -- i2i_tile_positions, i2i_tile_cut and i2i_tile_blend_u8 (csrc/resize.hip, the contract is the comment of
i2i_tile_request in include/i2i_turbo.h), image_ops.tile_layout / tile_cut_u8 / tile_cut_planes / tile_blend_u8 and ``tile=`` of the two
models' forward_u8.  The oracle is tests/tile_ref.py (numpy slicing and the integer feather in int64); every comparison is
np.array_equal / torch.equal: byte movement and integer arithmetic have no tolerance.  The one exception is the noise field against
tests/randn_ref.py (fp64), under the bound of the noise contract (randn_cases.TOL)."""
import ctypes as C

import numpy as np
import torch

import tile_ref

FILL = 0xA5
GUARD = 64               # bytes in front of and behind the tile batch (and behind the last request of the blend's arena)
PARENT_SIZEOF_OP = 368

# (L, t, ov) of the layout rule: for every (t, ov) the lengths t, t + 1, t + 7, t + 8, 2t - ov, 2t - ov + 1, 3t + 5, and the two worked examples
POSITION_CASES = [(L, t, ov) for t, ov in ((16, 8), (16, 0), (24, 8), (512, 64), (512, 256))
                  for L in (t, t + 1, t + 7, t + 8, 2 * t - ov, 2 * t - ov + 1, 3 * t + 5)] + [(1280, 512, 64), (720, 512, 64)]

# name -> ((tw, th), overlap, [(h, w)]): 16 x 24 is exactly one tile of (24, 16); 17 x 25 one pixel more both ways (row bytes 75); 34 x 34 with
# t = 16, ov = 8 has the triple cover (pixels 18 .. 23); widths 25 and 37 give rows of 3-byte pixels that are no multiple of 4 bytes
SIZES = [(16, 24), (17, 25), (34, 34), (20, 37)]
LAYOUTS = {"one_tile_24x16_ov8": ((24, 16), 8, SIZES),
           "triple_16_ov8": ((16, 16), 8, SIZES),          # ov = t / 2
           "paste_16_ov0": ((16, 16), 0, SIZES)}
SECOND_SIZES = [(40, 16), (16, 16), (19, 50)]             # the second request set of the graph test (fewer requests: the rest become empty slots)


def to_dev(a, device):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(device)


def sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def stream_of(device):
    return torch.cuda.current_stream().cuda_stream if device != "cpu" else 0


def u8_requests(sizes, c, seed=0):
    rng = np.random.RandomState(100 + seed)
    return [None if hw is None else rng.randint(0, 256, (hw[0], hw[1], c)).astype(np.uint8) for hw in sizes]


def f32_requests(sizes, planes, seed=0):
    rng = np.random.RandomState(200 + seed)
    return [rng.standard_normal((planes, h, w)).astype(np.float32) for h, w in sizes]


# ---------------------------------------------------------------------------------------------------------------- the ABI
def check_struct_size(lib):
    from img2img_turbo_amd import _capi as K, image_ops
    assert lib.lib.i2i_sizeof_op() == C.sizeof(K.Op) == PARENT_SIZEOF_OP
    assert lib.lib.i2i_abi_version() == K.ABI_VERSION == 14 and (K.OP_TILE_CUT, K.OP_TILE_BLEND_U8) == (27, 28)
    assert C.sizeof(K.TileRequest) == 48 == image_ops.TILE_REQUEST_DTYPE.itemsize
    assert C.sizeof(K.TileCutParams) <= C.sizeof(K.IgemmParams) and C.sizeof(K.TileBlendU8Params) <= C.sizeof(K.IgemmParams)
    assert ([image_ops.TILE_REQUEST_DTYPE.fields[n][1] for n, _ in K.TileRequest._fields_]
            == [getattr(K.TileRequest, n).offset for n, _ in K.TileRequest._fields_])


# ---------------------------------------------------------------------------------------------------------------- positions
def check_positions(lib, L, t, ov):
    """i2i_tile_positions == image_ops.tile_positions == tile_ref.positions, and every property the layout rule promises."""
    from img2img_turbo_amd import image_ops
    want = tile_ref.positions(L, t, ov)
    assert image_ops.tile_positions(L, t, ov) == want and lib.tile_positions(L, t, ov) == want, (L, t, ov)
    assert lib.lib.i2i_tile_positions(L, t, ov, None, 0) == len(want)
    x = np.array(want, dtype=np.int64)
    assert x[0] == 0 and x[-1] + t == L
    assert (np.diff(x) > 0).all()                                            # strictly increasing
    assert (x[:-1] + t - x[1:] >= ov).all()                                  # neighbours overlap by at least ov
    assert (x[:-1] % 8 == 0).all()                                           # every position but the last is a multiple of 8
    cover = np.zeros(L, dtype=np.int64)
    for v in want:
        cover[v:v + t] += 1
    assert cover.min() >= 1 and cover.max() <= 3
    assert (x // 8 + t // 8 <= -(-L // 8)).all()                             # the latent crop stays inside the latent field
    assert len(want) < 4 or (x[3:] >= x[:-3] + t).all()                      # what i2i_tile_blend_u8's check asks for


def check_positions_examples(lib):
    assert lib.tile_positions(1280, 512, 64) == [0, 448, 768]
    assert lib.tile_positions(720, 512, 64) == [0, 208]
    assert lib.tile_positions(34, 16, 8) == [0, 8, 16, 18]
    cover = np.zeros(34, dtype=int)
    for v in (0, 8, 16, 18):
        cover[v:v + 16] += 1
    assert np.flatnonzero(cover == 3).tolist() == list(range(18, 24))


def check_positions_errors(lib):
    """Arguments outside the rule return I2I_ERR_BAD_ARG and write nothing; Python raises ValueError for the same ones."""
    import pytest
    from img2img_turbo_amd import image_ops
    out = np.full(8, 77, dtype=np.int32)
    f = lib.lib.i2i_tile_positions
    for L, t, ov in ((15, 16, 8), (64, 12, 0), (64, 0, 0), (64, -8, 0), (64, 16, 4), (64, 16, 16), (64, 16, -8), (0, 16, 0)):
        assert f(L, t, ov, out.ctypes.data, 8) == -1, (L, t, ov)
        assert lib.lib.i2i_last_error().decode().startswith("tile_positions:")
        with pytest.raises(ValueError):
            image_ops.tile_positions(L, t, ov)
    assert f(34, 16, 8, out.ctypes.data, 3) == -1 and (out == 77).all()      # capacity 3 < 4 tiles
    assert f(34, 16, 8, out.ctypes.data, 8) == 4 and out.tolist() == [0, 8, 16, 18, 77, 77, 77, 77]


# ---------------------------------------------------------------------------------------------------------------- the raw entries
class Batch:
    """One set of requests laid out in caller-owned, FILL-ed buffers of a fixed capacity (what a host with static buffers does): the
    request arena, the tile batch between two guards, descriptors, positions, the flag word.  ``reqs``: numpy arrays, uint8 [h, w, c] or
    fp32 [planes, h, w]; None is an empty slot.  The descriptors are packed here from tile_ref's positions, not by image_ops."""

    def __init__(self, lib, device, reqs, tile, ov, *, capacity=None):
        self.lib, self.device, self.tile, self.ov = lib, device, tile, ov
        first = next(a for a in reqs if a is not None)
        self.f32 = first.dtype == np.float32
        self.planes, self.px = (first.shape[0], 4) if self.f32 else (1, first.shape[-1])
        self.pack(reqs)
        cap = capacity or dict(arena=self.arena_bytes + GUARD, tiles=self.T, pos=self.pos.size, n=len(reqs))
        assert self.arena_bytes <= cap["arena"] and self.T <= cap["tiles"] and self.pos.size <= cap["pos"] and len(reqs) <= cap["n"]
        self.cap = cap
        self.tile_bytes = self.planes * tile[1] * tile[0] * self.px
        self.arena = torch.full((cap["arena"],), FILL, dtype=torch.uint8, device=device)
        self.tbuf = torch.full((2 * GUARD + cap["tiles"] * self.tile_bytes,), FILL, dtype=torch.uint8, device=device)
        self.tiles = self.tbuf[GUARD:GUARD + cap["tiles"] * self.tile_bytes]
        self.desc_dev = torch.zeros(cap["n"] * 6, dtype=torch.int64, device=device)
        self.pos_dev = torch.zeros(cap["pos"], dtype=torch.int32, device=device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=device)
        self.upload()

    def pack(self, reqs, positions=None):
        """Descriptors, positions and offsets of ``reqs`` on the host.  ``positions``: {request: (xs, ys)} overriding the rule."""
        from img2img_turbo_amd import image_ops
        self.reqs = reqs
        tw, th = self.tile
        self.desc = np.zeros(len(reqs), dtype=image_ops.TILE_REQUEST_DTYPE)
        self.org, self.offs, self.tile0 = [], [], []
        pool, off, t0 = [], 0, 0
        for b, a in enumerate(reqs):
            self.offs.append(off)
            self.tile0.append(t0)
            if a is None:
                self.org.append([])
                continue
            h, w = a.shape[1:] if self.f32 else a.shape[:2]
            xs, ys = (positions or {}).get(b) or (tile_ref.positions(w, tw, self.ov), tile_ref.positions(h, th, self.ov))
            self.org.append(tile_ref.origins(h, w, tw, th, self.ov, xs, ys))
            xs_off = sum(len(p) for p in pool)
            pool += [list(xs), list(ys)]
            self.desc[b] = (off, h, w, t0, len(xs), len(ys), xs_off, xs_off + len(xs), (0, 0, 0))
            off += (a.nbytes + 3) & ~3
            t0 += len(xs) * len(ys)
        self.arena_bytes, self.T = off, t0
        self.pos = np.array([v for p in pool for v in p], dtype=np.int32)

    def upload(self, pixels=True):
        """Descriptors (padded with empty slots up to the capacity) and positions in place; with ``pixels`` the requests into the arena."""
        from img2img_turbo_amd import image_ops
        d = np.zeros(self.cap["n"], dtype=image_ops.TILE_REQUEST_DTYPE)
        d[:len(self.reqs)] = self.desc
        self.desc_dev.copy_(torch.from_numpy(d.view(np.int64).reshape(-1).copy()))
        p = np.zeros(self.cap["pos"], dtype=np.int32)
        p[:self.pos.size] = self.pos
        self.pos_dev.copy_(torch.from_numpy(p))
        if pixels:
            host = np.full(self.cap["arena"], FILL, dtype=np.uint8)
            for a, off in zip(self.reqs, self.offs):
                if a is not None:
                    host[off:off + a.nbytes] = np.frombuffer(a.tobytes(), dtype=np.uint8)
            self.arena.copy_(torch.from_numpy(host))

    def cut_op(self, units=None):
        from img2img_turbo_amd import ops as O
        units = units or max(1, self.T * self.tile_bytes // 4)
        return O.tile_cut(self.arena, self.tiles, self.desc_dev, self.pos_dev, n=self.cap["n"], planes=self.planes, px_bytes=self.px, tw=self.tile[0],
                          th=self.tile[1], tiles_capacity=self.cap["tiles"], grid_units=units, bad_mask=self.bad)

    def blend_op(self, ramp, units=None):
        from img2img_turbo_amd import ops as O
        assert not self.f32
        units = units or max(1, self.arena_bytes)
        return O.tile_blend_u8(self.tiles, self.arena, self.desc_dev, self.pos_dev, n=self.cap["n"], c=self.px, ramp=ramp, tw=self.tile[0],
                               th=self.tile[1], tiles_capacity=self.cap["tiles"], grid_units=units, bad_mask=self.bad)

    def cut(self, units=None):
        _, p = self.cut_op(units)
        self.lib.check(self.lib.lib.i2i_tile_cut(C.addressof(p), 0, C.c_void_p(stream_of(self.device))))
        sync(self.device)
        return self

    def blend(self, ramp, units=None):
        _, p = self.blend_op(ramp, units)
        self.lib.check(self.lib.lib.i2i_tile_blend_u8(C.addressof(p), 0, C.c_void_p(stream_of(self.device))))
        sync(self.device)
        return self

    def mask(self):
        return int(self.bad.cpu().numpy().view(np.uint32)[0])

    def set_tiles(self, tiles):
        """Tile contents for the blend: uint8 [T, th, tw, c] into the first T slots."""
        self.tiles[:tiles.size].copy_(torch.from_numpy(np.ascontiguousarray(tiles).reshape(-1)))

    def want_tiles(self, skipped=()):
        """{slot: the tile by numpy slicing} of every request not in ``skipped``."""
        tw, th = self.tile
        out = {}
        for b, a in enumerate(self.reqs):
            if a is None or b in skipped:
                continue
            for k, t in enumerate(tile_ref.cut(a, self.org[b], tw, th, axes=(1, 2) if self.f32 else (0, 1))):
                out[self.tile0[b] + k] = t
        return out

    def check_cut(self, skipped=()):
        """Every tile of every request not in ``skipped`` is bit-equal to slicing; every other byte of the tile buffer -- both guards, the
        slots of skipped requests, the slots behind the last tile -- still holds FILL."""
        buf = self.tbuf.cpu().numpy()
        untouched = np.ones(buf.size, dtype=bool)
        for slot, t in self.want_tiles(skipped).items():
            lo = GUARD + slot * self.tile_bytes
            got = buf[lo:lo + self.tile_bytes]
            assert np.array_equal(got, np.frombuffer(np.ascontiguousarray(t).tobytes(), dtype=np.uint8)), ("tile", slot)
            untouched[lo:lo + self.tile_bytes] = False
        assert (buf[untouched] == FILL).all(), ("tile buffer", np.flatnonzero(untouched & (buf != FILL))[:8])

    def check_blend(self, tiles, ramp, skipped=(), holes=()):
        """Every request not in ``skipped`` equals tile_ref.blend of its tiles; padding, skipped requests and the tail hold FILL."""
        got = self.arena.cpu().numpy()
        untouched = np.ones(got.size, dtype=bool)
        for b, a in enumerate(self.reqs):
            if a is None or b in skipped:
                continue
            h, w = a.shape[:2]
            n = len(self.org[b])
            want, hole = tile_ref.blend(tiles[self.tile0[b]:self.tile0[b] + n], h, w, self.org[b], ramp)
            assert hole == (b in holes), b
            assert np.array_equal(got[self.offs[b]:self.offs[b] + a.nbytes].reshape(a.shape), want), ("blend", b, a.shape)
            untouched[self.offs[b]:self.offs[b] + a.nbytes] = False
        assert (got[untouched] == FILL).all(), ("arena", np.flatnonzero(untouched & (got != FILL))[:8])


def layout_batch(lib, device, name, c=3, *, f32=False, empty=False, **kw):
    tile, ov, sizes = LAYOUTS[name]
    reqs = f32_requests(sizes, 4) if f32 else u8_requests(sizes, c)
    if empty:
        reqs = reqs[:2] + [None] + reqs[2:]
    return Batch(lib, device, reqs, tile, ov, **kw)


def check_cut(lib, device, name, c=3, f32=False):
    """i2i_tile_cut == numpy slicing, guards untouched, nobody flagged; with an empty slot in the middle."""
    for empty in (False, True):
        b = layout_batch(lib, device, name, c, f32=f32, empty=empty).cut()
        b.check_cut()
        assert b.mask() == 0


def random_tiles(b, seed=5):
    rng = np.random.RandomState(seed)
    t = rng.randint(0, 256, (b.T, b.tile[1], b.tile[0], b.px)).astype(np.uint8)
    t[::3] = np.where(rng.rand(*t[::3].shape) < 0.5, 0, 255)                 # hard 0 / 255 tiles: both ends of the rounding
    return t


def check_blend(lib, device, name, c=3):
    """i2i_tile_blend_u8 on random tiles == tile_ref.blend at ramp = max(ov, 1) and at ramp = 1 (the plain average); the two differ where
    the overlap is wider than a pixel; with an empty slot too."""
    outs = {}
    for ramp in (max(LAYOUTS[name][1], 1), 1):
        for empty in (False, True):
            b = layout_batch(lib, device, name, c, empty=empty)
            tiles = random_tiles(b)
            b.set_tiles(tiles)
            b.arena.fill_(FILL)
            b.blend(ramp).check_blend(tiles, ramp)
            assert b.mask() == 0
            if not empty:
                outs[ramp] = b.arena.cpu().numpy()
    if LAYOUTS[name][1] > 1:
        assert not np.array_equal(outs[LAYOUTS[name][1]], outs[1])
    if LAYOUTS[name][1] == 0:                                               # overlap 0 on a multiple of the tile: a plain paste
        b = Batch(lib, device, u8_requests([(32, 48)], c), LAYOUTS[name][0], 0)
        tiles = random_tiles(b)
        b.set_tiles(tiles)
        b.blend(1)
        got = b.arena.cpu().numpy()[:32 * 48 * c].reshape(32, 48, c)
        for t, (y0, x0) in enumerate(b.org[0]):
            assert np.array_equal(got[y0:y0 + 16, x0:x0 + 16], tiles[t]), t


def check_round_trip(lib, device, name, c=3):
    """blend(cut(img)) == img: the weighted average of equal values is exact under the rounding rule."""
    b = layout_batch(lib, device, name, c).cut()
    want = b.arena.cpu().numpy().copy()
    b.arena.fill_(FILL)
    b.blend(max(b.ov, 1))
    assert np.array_equal(b.arena.cpu().numpy(), want) and b.mask() == 0
    # the eager forms: a list of requests of different sizes, and a stacked tensor
    from img2img_turbo_amd import image_ops
    tile, ov, sizes = LAYOUTS[name]
    reqs = u8_requests(sizes, c, seed=1)
    tiles, layout = image_ops.tile_cut_u8([to_dev(a, device) for a in reqs], tile, ov, lib)
    assert tiles.shape == (layout.T, tile[1], tile[0], c) and layout.T == b.T and layout.counts == [(len(set(x for _, x in o)), len(set(y for y, _ in o))) for o in b.org]
    for t, (r, y0, x0) in enumerate(layout.origins):
        assert np.array_equal(tiles[t].cpu().numpy(), reqs[r][y0:y0 + tile[1], x0:x0 + tile[0]]), t
    back = image_ops.tile_blend_u8(tiles, layout, lib)
    assert isinstance(back, list) and all(np.array_equal(g.cpu().numpy(), a) for g, a in zip(back, reqs))
    stack = np.stack(u8_requests([sizes[2]] * 2, c, seed=2))
    tiles, layout = image_ops.tile_cut_u8(to_dev(stack, device), tile, ov, lib)
    back = image_ops.tile_blend_u8(tiles, layout, lib, stack=True)
    assert torch.is_tensor(back) and np.array_equal(back.cpu().numpy(), stack)


def check_planes_eager(lib, device):
    """image_ops.tile_cut_planes: the latent-resolution crop of fp32 fields (the noise rule) == slicing at (y0 // 8, x0 // 8)."""
    from img2img_turbo_amd import image_ops
    sizes = [(56, 72), (32, 40), (37, 51)]
    layout = image_ops.tile_layout(sizes, (40, 32), 8)
    fields = f32_requests([(-(-h // 8), -(-w // 8)) for h, w in sizes], 4)
    got = image_ops.tile_cut_planes([to_dev(f, device) for f in fields], layout, lib).cpu().numpy()
    assert got.shape == (layout.T, 4, 4, 5)
    for t, (b, y0, x0) in enumerate(layout.origins):
        assert np.array_equal(got[t], fields[b][:, y0 // 8:y0 // 8 + 4, x0 // 8:x0 // 8 + 5]), t


def check_grid_independence(lib, device):
    """Capacity hint 1 (one workgroup per request striding over everything) and a huge one (the grid is capped): the same bits, both ops."""
    name = "triple_16_ov8"
    tiles = None
    res = []
    for units in (1, 1 << 40):
        b = layout_batch(lib, device, name).cut(units)
        b.check_cut()
        tiles = random_tiles(b)
        b.set_tiles(tiles)
        b.arena.fill_(FILL)
        b.blend(8, units).check_blend(tiles, 8)
        res.append(b.arena.cpu().numpy())
    assert np.array_equal(res[0], res[1])


def check_graph(lib, device):
    """One captured graph of cut and blend over fixed-capacity buffers serves two sets of request sizes: launch, rewrite descriptors,
    positions and pixels in place (other sizes, fewer requests: the rest become empty slots), launch again.  The blend writes the round
    trip back into the arena the cut read (the ops run in order on one stream)."""
    from img2img_turbo_amd import _capi as K
    tile, ov = (16, 16), 8
    cap = dict(arena=32 << 10, tiles=64, pos=64, n=6)
    b = Batch(lib, device, u8_requests(SIZES, 3), tile, ov, capacity=cap)
    prog = K.Program()
    for label, (opcode, params) in (("tile.cut", b.cut_op(units=1 << 14)), ("tile.blend", b.blend_op(8, units=1 << 14))):
        prog.add(opcode, K.F32, params, label)
    prog.freeze()
    g = lib.graph_create(prog)
    try:
        for reqs in (b.reqs, u8_requests(SECOND_SIZES, 3, seed=3)):
            b.pack(reqs)
            b.tbuf.fill_(FILL)
            b.upload()
            want = b.arena.cpu().numpy().copy()
            lib.graph_launch(g, stream_of(device))
            sync(device)
            b.check_cut()
            assert np.array_equal(b.arena.cpu().numpy(), want) and b.mask() == 0
    finally:
        sync(device)
        lib.graph_destroy(g)
    b.tbuf.fill_(FILL)                                                      # the same program through i2i_run (capi.hip's dispatch)
    lib.run(prog, stream_of(device))
    sync(device)
    b.check_cut()


# ---------------------------------------------------------------------------------------------------------------- errors
def check_bad_args(lib, device):
    """Every host-side error of the contract returns I2I_ERR_BAD_ARG with a message and launches nothing; n == 0 is a successful no-op."""
    b = layout_batch(lib, device, "triple_16_ov8")
    for entry, make, prefix in ((lib.lib.i2i_tile_cut, b.cut_op, "tile_cut:"), (lib.lib.i2i_tile_blend_u8, lambda: b.blend_op(8), "tile_blend_u8:")):
        p = make()[1]
        first, px = ("src", "px_bytes") if prefix == "tile_cut:" else ("tiles", "c")
        bad = [{first: 0}, dict(dst=0), dict(reqs=0), dict(pos=0), {first: getattr(p, first) + 2}, dict(dst=p.dst + 1), dict(pos=p.pos + 2), dict(reqs=p.reqs + 4),
               dict(bad_mask=p.bad_mask + 2), {px: 0}, {px: 5}, dict(n=-1), dict(tw=0), dict(th=-16), dict(tiles_capacity=-1), dict(grid_units=0),
               dict(arena_bytes=-1), dict(pos_len=-1)] + ([dict(planes=0)] if prefix == "tile_cut:" else [dict(ramp=0), dict(ramp=257)])
        for kw in bad:
            q = make()[1]
            for k, v in kw.items():
                setattr(q, k, v)
            assert entry(C.addressof(q), 0, C.c_void_p(stream_of(device))) == -1, (prefix, kw)
            msg = lib.lib.i2i_last_error().decode()
            assert msg.startswith(prefix) and len(msg) > len(prefix) + 1, (kw, msg)
        assert entry(None, 0, C.c_void_p(stream_of(device))) == -1
        q = make()[1]
        q.n = 0
        assert entry(C.addressof(q), 0, C.c_void_p(stream_of(device))) == 0
    sync(device)
    assert (b.tbuf.cpu().numpy() == FILL).all() and b.mask() == 0


REJECTS = ["a position outside the image", "a negative position", "a tile slot beyond capacity", "a misaligned offset", "an offset past the arena",
           "positions past the pool", "an uncovered pixel", "four tiles over a pixel"]


def check_rejection(lib, device, what):
    """EMULATOR ONLY (the GPU tests use valid descriptors): request 2 (34 x 34, sixteen tiles) has a wrong descriptor.  It is skipped whole
    by the op that objects -- its tile slots / its bytes of the arena stay FILL -- its bit is set in bad_mask, its neighbours are
    bit-exact.  "an uncovered pixel" is accepted by the check: the request is written with 0 there, and flagged."""
    name = "triple_16_ov8"
    b = layout_batch(lib, device, name)
    d = b.desc
    cut_rejects = blend_rejects = True
    positions = None
    if what == "a position outside the image":
        b.pos[int(d["xs_off"][2]) + 3] = 34 - 16 + 1
    elif what == "a negative position":
        b.pos[int(d["ys_off"][2])] = -8
    elif what == "a tile slot beyond capacity":
        d["tile0"][2] = b.cap["tiles"] - 15                                   # sixteen tiles do not fit behind it
    elif what == "a misaligned offset":
        d["off"][2] += 2
    elif what == "an offset past the arena":
        d["off"][2] = (b.cap["arena"] & ~3) - 64
    elif what == "positions past the pool":
        d["ys_off"][2] = b.cap["pos"] - 3
    elif what == "an uncovered pixel":
        positions = {2: ([0, 18], [0, 8, 16, 18])}                            # columns 16 and 17 have no tile
        cut_rejects = blend_rejects = False
    elif what == "four tiles over a pixel":
        positions = {2: ([0, 2, 4, 6, 18], [0, 8, 16, 18])}                   # valid for the cut; the blend's cover bound refuses it
        cut_rejects = False
    else:
        raise AssertionError(what)
    if positions:
        b = Batch(lib, device, b.reqs, b.tile, b.ov, capacity=dict(arena=b.cap["arena"], tiles=b.cap["tiles"] + 8, pos=b.cap["pos"] + 8, n=b.cap["n"]))
        b.pack(b.reqs, positions)
    b.upload()
    b.cut()
    assert b.mask() == ((1 << 2) if cut_rejects else 0), (what, hex(b.mask()))
    b.check_cut(skipped=(2,) if cut_rejects else ())
    tiles = random_tiles(b)
    b.set_tiles(tiles)
    b.bad.zero_()
    b.arena.fill_(FILL)
    b.blend(8)
    assert b.mask() == ((1 << 2) if (blend_rejects or what == "an uncovered pixel") else 0), (what, hex(b.mask()))
    b.check_blend(tiles, 8, skipped=(2,) if blend_rejects else (), holes=(2,) if what == "an uncovered pixel" else ())


# ---------------------------------------------------------------------------------------------------------------- the models
MODEL_TILE = (40, 32)


def make_pix2pix(lib, device, dtype=torch.float32, **kw):
    from img2img_turbo_amd import arch
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.synth import make_pix2pix_weights
    return Pix2Pix_Turbo(weights=make_pix2pix_weights(arch.TINY_UNET, arch.TINY_VAE, seed=1234), device=device, dtype=dtype, lib=lib, **kw)


def make_cyclegan(lib, device, dtype=torch.float32):
    """As ragged_cases.check_cyclegan_list builds it."""
    from oracle import TINY_UNET, TINY_VAE
    from oracle.synth import make_cyclegan_weights
    from img2img_turbo_amd.cyclegan_turbo import CycleGAN_Turbo
    from img2img_turbo_amd.weights import GeneratorWeights
    mw = make_cyclegan_weights(TINY_UNET, TINY_VAE, rank_unet=16)
    gw = GeneratorWeights(mw.unet, mw.vae, mw.unet_arch, mw.vae_arch, mw.unet_scaling, mw.vae_scaling, mw.vae_b2a)
    return CycleGAN_Turbo(weights=gw, device=device, dtype=dtype, lib=lib)


def caption(device, n=1, seed=4):
    from oracle import TINY_UNET
    return torch.randn(n, 77, TINY_UNET.cross_attention_dim, generator=torch.Generator().manual_seed(seed)).to(device)


def photo(h, w, seed):
    """uint8 [h, w, 3]: smooth blobs with hard edges (something for Canny to find), not noise."""
    rng = np.random.RandomState(300 + seed)
    yy, xx = np.mgrid[:h, :w]
    img = np.zeros((h, w, 3), dtype=np.float64)
    for _ in range(4):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, 14)
        img += ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r)[:, :, None] * rng.uniform(60, 250, 3)
    return np.clip(img + rng.uniform(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)


def noise_crops(lib, device, layout, seeds, stream=0, lat=4):
    """The test's own statement of the noise rule: request b's field is rng.randn([lat, ceil(h / 8), ceil(w / 8)]) at (seeds[b], step 0,
    stream); tile t gets its slice at (y0 // 8, x0 // 8) -- torch slicing, not the cut kernel."""
    from img2img_turbo_amd import rng
    tw, th = layout.tile
    fields = [rng.randn((lat, -(-h // 8), -(-w // 8)), s, 0, stream, device=device, lib=lib) for (h, w), s in zip(layout.sizes, seeds)]
    return torch.stack([fields[b][:, y0 // 8:y0 // 8 + th // 8, x0 // 8:x0 // 8 + tw // 8] for b, y0, x0 in layout.origins]), fields


def check_noise(lib, device):
    """With seed=, the eps handed to the forward for tile k is the crop of tests/randn_ref.py's field of that request (within the noise
    contract's bound); two overlapping tiles agree bit for bit on the latent cells they share; the same request in another slot and under
    another chunking gets the same crops.  The forward itself is replaced by a recorder: the rule lives in front of it."""
    import randn_cases as rc
    import randn_ref
    model = make_pix2pix(lib, device)
    sizes = [(56, 72), (32, 40)]
    items = [to_dev(photo(h, w, i), device) for i, (h, w) in enumerate(sizes)]
    seen = []

    def record(tiles, cap, eps, noise):
        seen.append(eps.clone())
        return tiles

    def run(reqs, seeds, tile_batch):
        del seen[:]
        out, layout = model._forward_tiles(reqs, False, record, tile=MODEL_TILE, tile_overlap=8, tile_batch=tile_batch, seed=seeds, stochastic=False,
                                           caption_enc=caption(device))
        assert all(torch.equal(o, r) for o, r in zip(out, reqs))               # (identity forward: the round trip)
        return torch.cat(seen).cpu().numpy(), layout

    eps, layout = run(items, [11, 12], 8)
    assert layout.T == 5 and eps.shape == (5, 4, 4, 5)
    for t, (b, y0, x0) in enumerate(layout.origins):
        h8, w8 = -(-sizes[b][0] // 8), -(-sizes[b][1] // 8)
        val, rad = randn_ref.normal(4 * h8 * w8, 11 + b, 0, 0)
        sl = (slice(None), slice(y0 // 8, y0 // 8 + 4), slice(x0 // 8, x0 // 8 + 5))
        want, bound = val.reshape(4, h8, w8)[sl], rad.reshape(4, h8, w8)[sl] * rc.TOL
        assert (np.abs(eps[t] - want) <= bound).all(), t
    # tiles 0 and 1 of request 0 sit at x0 = 0 and 32: latent columns 4 of the first and 0 of the second are the same cells; tiles 0 and 2
    # at y0 = 0 and 24: latent row 3 of the first is row 0 of the second
    assert layout.origins[:4] == [(0, 0, 0), (0, 0, 32), (0, 24, 0), (0, 24, 32)]
    assert np.array_equal(eps[0][:, :, 4:], eps[1][:, :, :1]) and np.array_equal(eps[0][:, 3:, :], eps[2][:, :1, :])
    swapped, layout2 = run(items[::-1], [12, 11], 2)                           # the other slot order, chunks of 2 + 2 + 1
    assert layout2.origins[0] == (0, 0, 0) and np.array_equal(swapped[0], eps[4]) and np.array_equal(swapped[1:], eps[:4])
    model.release_plans()


def check_pix2pix_tiled(lib, device, sizes, *, dtype=torch.float32, canny=None, overlap=8, tile_batch=2, stacked=True):
    """forward_u8(list, tile=, seed=) == tile_blend_u8(forward_u8(the cut tiles in the same chunks, eps = the crops), layout), bit for bit;
    with canny= the edges over the WHOLE request equal image_ops.canny_u8 of it and are what gets cut."""
    from img2img_turbo_amd import image_ops
    model = make_pix2pix(lib, device, dtype)
    try:
        reqs = [to_dev(photo(h, w, i), device) for i, (h, w) in enumerate(sizes)]
        cap, seeds = caption(device), [21 + i for i in range(len(sizes))]
        if canny is None:
            outs = model.forward_u8(reqs, caption_enc=cap, tile=MODEL_TILE, tile_overlap=overlap, tile_batch=tile_batch, seed=seeds)
            inputs = reqs
        else:
            outs, edges = model.forward_u8(reqs, caption_enc=cap, tile=MODEL_TILE, tile_overlap=overlap, tile_batch=tile_batch, seed=seeds, canny=canny,
                                           return_edges=True)
            inputs = [image_ops.canny_u8(r[None], canny[0], canny[1], 3, lib)[0] for r in reqs]
            assert isinstance(edges, list) and all(torch.equal(e, w) for e, w in zip(edges, inputs))
            assert any(int(e.max()) == 255 for e in inputs)                      # (there are edges to find)
        assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(h, w, 3) for h, w in sizes]
        tiles, layout = image_ops.tile_cut_u8(inputs, MODEL_TILE, overlap, lib)
        eps, _ = noise_crops(lib, device, layout, seeds)
        parts = [model.forward_u8(tiles[k:k + tile_batch], caption_enc=cap, eps=eps[k:k + tile_batch]) for k in range(0, layout.T, tile_batch)]
        want = image_ops.tile_blend_u8(torch.cat(parts), layout, lib)
        for b in range(len(sizes)):
            assert torch.equal(outs[b], want[b]), (b, int((outs[b] != want[b]).sum()))
        assert len(set(outs[0].cpu().numpy().reshape(-1).tolist())) > 2             # (not a constant image)
        # a request that is exactly one tile is the ordinary forward of it
        one = [b for b, hw in enumerate(sizes) if hw == (MODEL_TILE[1], MODEL_TILE[0])]
        for b in one:
            k = layout.tile0[b]
            assert torch.equal(outs[b], torch.cat(parts)[k])
        if stacked:                              # a stacked tensor in, a stacked tensor out; one seed for the batch, no seed at all
            both = torch.stack([reqs[0], reqs[0]])
            for seed in (seeds[0], None):
                st = model.forward_u8(both, caption_enc=cap, tile=MODEL_TILE, tile_overlap=overlap, tile_batch=8, seed=seed)
                assert torch.is_tensor(st) and st.shape == both.shape and st.dtype == torch.uint8
    finally:
        model.release_plans()


def check_cyclegan_tiled(lib, device, sizes, *, dtype=torch.float32, overlap=8, tile_batch=2):
    """The same identity for CycleGAN_Turbo.forward_u8, with one caption per request expanded per tile."""
    from img2img_turbo_amd import image_ops
    model = make_cyclegan(lib, device, dtype)
    try:
        reqs = [to_dev(photo(h, w, 10 + i), device) for i, (h, w) in enumerate(sizes)]
        caps, seeds = caption(device, len(sizes)), [31 + i for i in range(len(sizes))]
        outs = model.forward_u8(reqs, direction="a2b", caption_emb=caps, tile=MODEL_TILE, tile_overlap=overlap, tile_batch=tile_batch, seed=seeds)
        assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(h, w, 3) for h, w in sizes]
        tiles, layout = image_ops.tile_cut_u8(reqs, MODEL_TILE, overlap, lib)
        eps, _ = noise_crops(lib, device, layout, seeds)
        per_tile = caps[torch.tensor(layout.request_of_tile, device=caps.device)]
        parts = [model.forward_u8(tiles[k:k + tile_batch], direction="a2b", caption_emb=per_tile[k:k + tile_batch], eps=eps[k:k + tile_batch])
                 for k in range(0, layout.T, tile_batch)]
        want = image_ops.tile_blend_u8(torch.cat(parts), layout, lib)
        for b in range(len(sizes)):
            assert torch.equal(outs[b], want[b]), (b, int((outs[b] != want[b]).sum()))
    finally:
        model.release_plans()


def check_value_errors(lib, device):
    """Every refusal of section "Errors" is a ValueError with a reason, raised before any forward runs."""
    import pytest
    cap = caption(device)
    big, small = to_dev(photo(56, 72, 0), device), to_dev(photo(24, 40, 1), device)
    p2p = make_pix2pix(lib, device)
    cyc = make_cyclegan(lib, device)
    kw = dict(caption_enc=cap, tile=MODEL_TILE, tile_overlap=8, seed=1)
    for bad in (dict(images=[small]),                                        # a request smaller than the tile along an axis
                dict(tile=(36, 32)), dict(tile=(40, 0)), dict(tile=40),      # not a (positive) multiple of 8, not a pair
                dict(tile_overlap=4), dict(tile_overlap=24), dict(tile_overlap=-8),
                dict(variations=2), dict(eps=torch.zeros(1, 4, 4, 5)), dict(tile_batch=0)):
        args = dict(kw)
        images = bad.pop("images", [big])
        args.update(bad)
        if "eps" in bad:
            args.pop("seed")
        with pytest.raises(ValueError) as e:
            p2p.forward_u8(images, **args)
        assert len(str(e.value)) > 10, bad
    with pytest.raises(ValueError):
        cyc.forward_u8([big], direction="a2b", caption_emb=cap, tile=MODEL_TILE, tile_overlap=8, resize_back=True)
    with pytest.raises(ValueError):
        cyc.forward_u8([big], direction="a2b", caption_emb=cap, tile=MODEL_TILE, eps=torch.zeros(1, 4, 4, 5))
    for extra in (dict(health="stages", health_per_image=True), dict(fingerprint="io")):
        with pytest.raises(ValueError):
            make_pix2pix(lib, device, **extra).forward_u8([big], **kw)
    assert not p2p._plans and not cyc._plans                                    # nothing was planned, nothing ran

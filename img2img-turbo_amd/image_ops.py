"""Device-side image pre/post-processing of the callers (row f1): LANCZOS resize of uint8 HWC image batches, bit-identical to
Pillow, and Canny edge detection, both of which the reference applies on the host around the generator:

  src/inference_paired.py:38-41    input_image.resize((w - w % 8, h - h % 8), Image.LANCZOS)
  src/inference_unpaired.py:40,53  transforms.Resize((512, 512), LANCZOS) ... output_pil.resize(input size, Image.LANCZOS)
  src/inference_paired.py:47-50    canny_from_pil(input_image, low, high) = cv2.Canny replicated to 3 channels (src/image_prep.py:6-12)

The tap windows and 22-bit fixed-point weights are computed here in double precision exactly as Pillow's
``precompute_coeffs`` / ``normalize_coeffs_8bpc`` do (src/libImaging/Resample.c); the two integer passes run in
csrc/resize.hip through ``i2i_resize_u8``, or, for a batch of images of different sizes, through ``i2i_resize_u8_ragged`` (two launches
for the whole batch, ``lanczos_resize_u8_ragged``).  Pure plumbing otherwise: no pixel arithmetic happens in Python.
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _capi

PRECISION_BITS = 32 - 8 - 2


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bicubic(x):
    """Pillow's bicubic_filter (Keys' cubic, a = -0.5), evaluated in its order of operations."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}      # name -> (weight function, support), as Pillow's `struct filter`


@functools.lru_cache(maxsize=128)
def resample_coeffs(in_size, out_size, filter="lanczos"):
    """Pillow's per-output-coordinate tap window and weights for one axis under ``filter`` ("lanczos": Image.LANCZOS; "bicubic":
    Image.BICUBIC, the default of ``Image.resize`` -- what gradio_canny2image.py:16 gets by passing no filter):
    (ksize, bounds int32 [out, 2], weights int32 [out, ksize])."""
    if filter not in FILTERS:
        raise ValueError("resample filter %r (supported: %s)" % (filter, ", ".join(sorted(FILTERS))))
    weight, filter_support = FILTERS[filter]
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ww = 0.0
        for x in range(xmax):
            w = weight((x + xmin - center + 0.5) * ss)
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            for x in range(xmax):
                kk[xx, x] /= ww
        bounds[xx] = (xmin, xmax)
    ik = np.where(kk < 0, (-0.5 + kk * (1 << PRECISION_BITS)).astype(np.int64),
                  (0.5 + kk * (1 << PRECISION_BITS)).astype(np.int64)).astype(np.int32)
    return ksize, bounds, ik


def lanczos_coeffs(in_size, out_size):
    """``resample_coeffs(in_size, out_size, "lanczos")``: Pillow's LANCZOS tap windows and weights for one axis."""
    return resample_coeffs(in_size, out_size, "lanczos")


import collections
import contextlib

_DEV_TABLES = collections.OrderedDict()      # (in, out, device[, filter]) -> coefficient tables on the device; small LRU: a server fed
_DEV_TABLES_MAX = 64                         # arbitrary input sizes must not grow device memory without bound


def _tables(in_size, out_size, device, resample="lanczos"):
    key = (in_size, out_size, str(device)) + (() if resample == "lanczos" else (resample,))
    if key in _DEV_TABLES:
        _DEV_TABLES.move_to_end(key)
    else:
        ksize, b, k = resample_coeffs(in_size, out_size, resample)
        _DEV_TABLES[key] = (ksize, torch.from_numpy(b.copy()).to(device), torch.from_numpy(k.copy()).to(device))
        while len(_DEV_TABLES) > _DEV_TABLES_MAX:
            _DEV_TABLES.popitem(last=False)
    return _DEV_TABLES[key]


def lanczos_resize_u8(images, size, lib=None, *, resample="lanczos"):
    """images: uint8 [N, H, W, C] (C <= 4) on the device -> uint8 [N, size[1], size[0], C]; ``size`` = (width, height) as PIL takes it.
    Bit-identical to ``Image.resize(size, Image.LANCZOS)`` per image.  Asynchronous on the current stream.
    ``resample="bicubic"``: the same passes on Pillow's BICUBIC tables, bit-identical to ``Image.resize(size)`` (Pillow's default filter:
    gradio_canny2image.py:16)."""
    assert images.dtype == torch.uint8 and images.dim() == 4 and images.shape[-1] <= 4
    lib = lib or _capi.default_library()
    n, h, w, c = images.shape
    ow, oh = int(size[0]), int(size[1])
    cur = images.contiguous()
    dev = cur.device
    # the GPU library takes device tensors only, the CPU emulator host tensors only: no silent mismatch
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    # the launches go to the GPU that owns the images even when another one is current
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        for axis, n_in, n_out in ((1, w, ow), (0, h, oh)):          # Pillow's order: horizontal pass, then vertical pass
            if n_in == n_out:
                continue
            ksize, bounds, coeffs = _tables(n_in, n_out, dev, resample)
            hin, win = cur.shape[1], cur.shape[2]
            out = torch.empty((n, hin, n_out, c) if axis == 1 else (n, n_out, win, c), dtype=torch.uint8, device=dev)
            p = _capi.ResizeU8Params()
            p.src, p.dst, p.n, p.hin, p.win, p.c = cur.data_ptr(), out.data_ptr(), n, hin, win, c
            p.axis, p.nout, p.ksize, p.bounds, p.coeffs = axis, n_out, ksize, bounds.data_ptr(), coeffs.data_ptr()
            lib.check(lib.lib.i2i_resize_u8(C.addressof(p), 0, stream))
            cur = out
    return cur


# ---- mixed-size batches: i2i_resize_u8_ragged (include/i2i_turbo.h), two launches for any number of images of any sizes ----
# one image of one pass as the kernels read it from device memory (i2i_resize_image, 48 bytes)
RAGGED_IMAGE_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("hin", "<i4"), ("win", "<i4"), ("nout", "<i4"), ("ksize", "<i4"),
                               ("bounds_off", "<i4"), ("coeffs_off", "<i4"), ("reserved", "<i4", (2,))])
assert RAGGED_IMAGE_DTYPE.itemsize == 48

RaggedLayout = collections.namedtuple("RaggedLayout", "n c desc tables src_off mid_off dst_off src_bytes mid_bytes dst_bytes units_h units_v")


def _align4(n):
    return (n + 3) & ~3


def ragged_layout(in_hw, out_wh, c, tables_of=lanczos_coeffs):
    """Host-side packing of one ragged resize (no device work): image b goes from ``in_hw[b]`` = (h, w) to ``out_wh[b]`` = (width, height).
    Three byte arenas -- sources, the horizontal pass's results [h, width, c], the final images [height, width, c] -- hold the images
    densely at 4-byte aligned offsets in batch order; one int32 pool holds bounds | coeffs of every distinct (in, out) pair once.
    ``desc`` is RAGGED_IMAGE_DTYPE [2, n]: row 0 the horizontal pass (sources -> mid), row 1 the vertical pass (mid -> final).  An image
    with h == 0 or w == 0 is an empty slot (hin = 0 in both passes, no bytes in any arena).  ``units_h`` / ``units_v``: the largest output
    pixel / output dword (or byte) count of an image, the grid_units of the two launches.  ``tables_of(in, out)`` -> (ksize, bounds,
    coeffs): lanczos_coeffs, or a library's own i2i_lanczos_tables (Library.lanczos_tables)."""
    n = len(in_hw)
    assert len(out_wh) == n and 1 <= c <= 4
    pool, where, pos = [], {}, 0
    desc = np.zeros((2, n), dtype=RAGGED_IMAGE_DTYPE)
    offs = np.zeros((3, n + 1), dtype=np.int64)
    units_h = units_v = 1
    for b, ((h, w), (ow, oh)) in enumerate(zip(in_hw, out_wh)):
        h, w, ow, oh = int(h), int(w), int(ow), int(oh)
        offs[:, b + 1] = offs[:, b]
        if h == 0 or w == 0:
            continue
        assert h > 0 and w > 0 and ow > 0 and oh > 0
        tab = []
        for key in ((w, ow), (h, oh)):
            if key not in where:
                ksize, bounds, coeffs = tables_of(*key)
                where[key] = (ksize, pos, pos + bounds.size)
                pool += [np.ascontiguousarray(bounds, dtype=np.int32).reshape(-1), np.ascontiguousarray(coeffs, dtype=np.int32).reshape(-1)]
                pos += bounds.size + coeffs.size
            tab.append(where[key])
        desc[0, b] = (offs[0, b], offs[1, b], h, w, ow, tab[0][0], tab[0][1], tab[0][2], (0, 0))
        desc[1, b] = (offs[1, b], offs[2, b], h, ow, oh, tab[1][0], tab[1][1], tab[1][2], (0, 0))
        offs[:, b + 1] += (_align4(h * w * c), _align4(h * ow * c), _align4(oh * ow * c))
        units_h = max(units_h, h * ow)
        units_v = max(units_v, oh * (ow * c // 4 if (ow * c) % 4 == 0 else ow * c))
    assert pos < 2 ** 31, "the table pool is indexed with int32"
    tables = np.concatenate(pool) if pool else np.zeros(1, dtype=np.int32)
    return RaggedLayout(n, c, desc, tables, offs[0, :n].copy(), offs[1, :n].copy(), offs[2, :n].copy(),
                        int(offs[0, n]), int(offs[1, n]), int(offs[2, n]), units_h, units_v)


def ragged_upload(layout, device):
    """(descriptors as an int64 device tensor [2 * n * 6], the table pool as an int32 device tensor) of a RaggedLayout."""
    desc = torch.from_numpy(np.ascontiguousarray(layout.desc).view(np.int64).reshape(-1).copy()) if layout.n else torch.zeros(6, dtype=torch.int64)
    return desc.to(device), torch.from_numpy(layout.tables.copy()).to(device)


def ragged_ops(layout, src, mid, dst, desc_dev, tables_dev, bad_mask=None, units=None):
    """The two ops of a ragged resize, horizontal then vertical, for _capi.Program.add / direct calls: [(opcode, params)] * 2.  ``units``:
    (units_h, units_v) to size the grids for a capacity other than this layout's own."""
    from . import ops as O
    uh, uv = units or (layout.units_h, layout.units_v)
    return [O.resize_u8_ragged(src, mid, desc_dev, tables_dev, n=layout.n, c=layout.c, axis=1, grid_units=uh, bad_mask=bad_mask),
            O.resize_u8_ragged(mid, dst, desc_dev, tables_dev, n=layout.n, c=layout.c, axis=0, grid_units=uv, bad_mask=bad_mask, first_image=layout.n)]


_RAGGED_POOLS = collections.OrderedDict()    # (sizes in, sizes out, c, library, device) -> (layout, descriptors, tables) on the device
_RAGGED_POOLS_MAX = 16


def _ragged_pool(lib, in_hw, out_wh, c, device, resample="lanczos"):
    key = (tuple(in_hw), tuple(out_wh), c, lib.path, str(device)) + (() if resample == "lanczos" else (resample,))
    if key in _RAGGED_POOLS:
        _RAGGED_POOLS.move_to_end(key)
    else:
        layout = ragged_layout(in_hw, out_wh, c, tables_of=lib.lanczos_tables if resample == "lanczos" else functools.partial(lib.resample_tables, resample))
        _RAGGED_POOLS[key] = (layout,) + ragged_upload(layout, device)
        while len(_RAGGED_POOLS) > _RAGGED_POOLS_MAX:
            _RAGGED_POOLS.popitem(last=False)
    return _RAGGED_POOLS[key]


def lanczos_resize_u8_ragged(images, size, lib=None, *, resample="lanczos"):
    """LANCZOS resize of a batch whose images differ in size, in TWO launches whatever the batch holds (i2i_resize_u8_ragged; the eager
    lanczos_resize_u8 is two launches and two allocations per distinct size).
    ``images``: a list of uint8 HWC tensors [H_b, W_b, C] on one device (same C <= 4), or one stacked uint8 [N, H, W, C].
    ``size``: one (width, height) for every image -> a stacked uint8 [N, height, width, C]; or a list of N (width, height) -> a list of
    uint8 [height_b, width_b, C] tensors (views of one arena).  Image b is bit-identical to ``lanczos_resize_u8(images[b][None], size_b)``,
    hence (C = 1, 3) to ``Image.resize(size_b, Image.LANCZOS)``.  Asynchronous on the current stream; the tap tables come from the
    library's i2i_lanczos_tables and are cached per set of sizes.  ``resample="bicubic"``: Pillow's BICUBIC tables (i2i_resample_tables)."""
    if resample not in FILTERS:
        raise ValueError("resample filter %r (supported: %s)" % (resample, ", ".join(sorted(FILTERS))))
    lib = lib or _capi.default_library()
    stacked_in = torch.is_tensor(images)
    if stacked_in:
        assert images.dtype == torch.uint8 and images.dim() == 4 and 1 <= images.shape[-1] <= 4
        items = list(images.unbind(0))
    else:
        items = list(images)
        assert all(torch.is_tensor(t) and t.dtype == torch.uint8 and t.dim() == 3 for t in items), "a list of uint8 [H, W, C] tensors"
    n = len(items)
    one_size = len(size) == 2 and all(isinstance(v, (int, np.integer)) for v in size)
    out_wh = [(int(size[0]), int(size[1]))] * n if one_size else [(int(s[0]), int(s[1])) for s in size]
    if len(out_wh) != n:
        raise ValueError("lanczos_resize_u8_ragged: %d sizes for %d images" % (len(out_wh), n))
    if n == 0:
        raise ValueError("lanczos_resize_u8_ragged: no images")
    c, dev = items[0].shape[-1], items[0].device
    if not (1 <= c <= 4) or any(t.shape[-1] != c or t.device != dev for t in items):
        raise ValueError("lanczos_resize_u8_ragged: the images must share the channel count (1..4) and the device")
    if any(min(t.shape[0], t.shape[1]) < 1 for t in items) or any(min(s) < 1 for s in out_wh):
        raise ValueError("lanczos_resize_u8_ragged: empty image or target size")
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    in_hw = [(int(t.shape[0]), int(t.shape[1])) for t in items]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        layout, desc_dev, tables_dev = _ragged_pool(lib, in_hw, out_wh, c, dev, resample)
        nb = in_hw[0][0] * in_hw[0][1] * c
        if stacked_in and nb % 4 == 0 and images.is_contiguous() and images.data_ptr() % 4 == 0:
            src = images.view(-1)                                                # already an arena: dense images at 4-byte aligned offsets
        else:                                                                    # one concatenation, each image padded to a multiple of 4 bytes
            pad = torch.zeros(3, dtype=torch.uint8, device=dev)
            parts = []
            for t, (h, w) in zip(items, in_hw):
                parts.append(t.reshape(-1))
                if (h * w * c) % 4:
                    parts.append(pad[:4 - (h * w * c) % 4])
            src = torch.cat(parts)
        mid = torch.empty(max(layout.mid_bytes, 4), dtype=torch.uint8, device=dev)
        dst = torch.empty(max(layout.dst_bytes, 4), dtype=torch.uint8, device=dev)
        for _, p in ragged_ops(layout, src, mid, dst, desc_dev, tables_dev):
            lib.check(lib.lib.i2i_resize_u8_ragged(C.addressof(p), 0, stream))
    views = [dst[o:o + oh * ow * c].view(oh, ow, c) for o, (ow, oh) in zip(layout.dst_off.tolist(), out_wh)]
    if not one_size:
        return views
    ow, oh = out_wh[0]
    return dst[:n * oh * ow * c].view(n, oh, ow, c) if (oh * ow * c) % 4 == 0 else torch.stack(views)


# ---- tiled forward at native resolution: i2i_tile_cut / i2i_tile_blend_u8 (include/i2i_turbo.h, the note above i2i_tile_request) ----
# one request as the kernels read it from device memory (i2i_tile_request, 48 bytes)
TILE_REQUEST_DTYPE = np.dtype([("off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("tile0", "<i4"), ("nx", "<i4"), ("ny", "<i4"), ("xs_off", "<i4"),
                               ("ys_off", "<i4"), ("reserved", "<i4", (3,))])
assert TILE_REQUEST_DTYPE.itemsize == 48


def tile_positions(length, tile, overlap):
    """THE layout rule of one axis (stated at i2i_tile_request; i2i_tile_positions is its C twin): stride s = tile - overlap, n = 1 +
    ceil((length - tile) / s) tiles at min(k * s, length - tile).  ValueError outside tile % 8 == 0, overlap % 8 == 0, 0 <= overlap <=
    tile / 2, length >= tile."""
    L, t, ov = int(length), int(tile), int(overlap)
    if t < 8 or t % 8:
        raise ValueError("tile extent %d is not a positive multiple of 8" % t)
    if ov < 0 or ov % 8 or ov > t // 2:
        raise ValueError("tile overlap %d (a multiple of 8 in 0 .. %d, half the tile extent %d)" % (ov, t // 2, t))
    if L < t:
        raise ValueError("a request of length %d is smaller than the tile extent %d" % (L, t))
    s = t - ov
    return [min(k * s, L - t) for k in range(1 + -(-(L - t) // s))]


TileTable = collections.namedtuple("TileTable", "desc pos offs arena_bytes planes px_bytes tw th units_cut units_blend desc_dev pos_dev")


class TileLayout:
    """The tiles of a batch of requests (host-side geometry, no device work): ``sizes[b]`` = (h, w), ``tile`` = (tw, th), ``overlap``.
    ``xs[b]`` / ``ys[b]``: the positions of request b, ``counts[b]`` = (nx, ny), ``tile0[b]`` its first tile slot, ``T`` the number of
    tiles, ``origins[t]`` = (request, y0, x0) of tile t (row-major per request, request after request).  ``table()`` packs the device
    descriptors for one tensor kind."""

    def __init__(self, sizes, tile, overlap):
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.tile = (int(tile[0]), int(tile[1]))
        self.overlap = int(overlap)
        tw, th = self.tile
        self.xs = [tile_positions(w, tw, self.overlap) for _, w in self.sizes]
        self.ys = [tile_positions(h, th, self.overlap) for h, _ in self.sizes]
        self.counts = [(len(x), len(y)) for x, y in zip(self.xs, self.ys)]
        self.tile0, self.origins = [], []
        for b, (x, y) in enumerate(zip(self.xs, self.ys)):
            self.tile0.append(len(self.origins))
            self.origins += [(b, y0, x0) for y0 in y for x0 in x]
        self.T = len(self.origins)
        self.request_of_tile = [o[0] for o in self.origins]
        self._tables = {}

    def table(self, planes, px_bytes, div=1, device=None):
        """The descriptors of the requests as [planes][h][w] pixels of ``px_bytes`` bytes packed densely, request after request at 4-byte
        aligned offsets: TileTable(desc TILE_REQUEST_DTYPE [n], pos int32 pool, offs, arena_bytes, .., tw, th, grid hints, and -- with
        ``device`` -- both as device tensors, cached).  ``div=8``: the latent-resolution twin (the noise rule): extents ceil(. / 8),
        positions // 8, tile extent // 8."""
        key = (int(planes), int(px_bytes), int(div), str(device))
        if key not in self._tables:
            planes, px_bytes, div = key[:3]
            n = len(self.sizes)
            tw, th = self.tile[0] // div, self.tile[1] // div
            desc = np.zeros(n, dtype=TILE_REQUEST_DTYPE)
            pool, offs, off, units_cut, units_blend = [], [], 0, 1, 1
            for b, (h, w) in enumerate(self.sizes):
                h, w = -(-h // div), -(-w // div)
                nx, ny = self.counts[b]
                xs_off = sum(len(p) for p in pool)
                pool += [[x // div for x in self.xs[b]], [y // div for y in self.ys[b]]]
                desc[b] = (off, h, w, self.tile0[b], nx, ny, xs_off, xs_off + nx, (0, 0, 0))
                offs.append(off)
                off += _align4(planes * h * w * px_bytes)
                units_cut = max(units_cut, nx * ny * planes * th * -(-tw * px_bytes // 4))
                units_blend = max(units_blend, h * w * px_bytes)
            pos = np.array([v for p in pool for v in p] or [0], dtype=np.int32)
            dd = pd = None
            if device is not None:
                dd = torch.from_numpy(desc.view(np.int64).reshape(-1).copy() if n else np.zeros(6, dtype=np.int64)).to(device)
                pd = torch.from_numpy(pos.copy()).to(device)
            self._tables[key] = TileTable(desc, pos, offs, off, planes, px_bytes, tw, th, units_cut, units_blend, dd, pd)
        return self._tables[key]


_TILE_LAYOUTS = collections.OrderedDict()    # (sizes, tile, overlap) -> TileLayout with its device tables; small LRU like _RAGGED_POOLS
_TILE_LAYOUTS_MAX = 16


def tile_layout(sizes, tile, overlap):
    """The cached TileLayout of a set of request sizes [(h, w)], ``tile`` = (tw, th) and ``overlap``: positions, tile counts and (through
    ``.table(planes, px_bytes, div, device)``) the descriptors as device tensors, cached like the tap tables.  ValueError if the layout
    rule refuses an argument (tile_positions)."""
    key = (tuple((int(h), int(w)) for h, w in sizes), (int(tile[0]), int(tile[1])), int(overlap))
    if key in _TILE_LAYOUTS:
        _TILE_LAYOUTS.move_to_end(key)
    else:
        _TILE_LAYOUTS[key] = TileLayout(*key)
        while len(_TILE_LAYOUTS) > _TILE_LAYOUTS_MAX:
            _TILE_LAYOUTS.popitem(last=False)
    return _TILE_LAYOUTS[key]


def _pack_arena(items):
    """The flattened tensors as ONE uint8 arena, each padded to a multiple of 4 bytes (what TileLayout.table's offsets assume)."""
    dev = items[0].device
    pad = torch.zeros(3, dtype=torch.uint8, device=dev)
    parts = []
    for t in items:
        flat = t.contiguous().view(torch.uint8).reshape(-1)
        parts.append(flat)
        if flat.numel() % 4:
            parts.append(pad[:4 - flat.numel() % 4])
    return torch.cat(parts) if len(parts) > 1 else parts[0]


def _tile_cut(items, layout, table, out, lib):
    dev = items[0].device
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    from . import ops as O
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        src = _pack_arena(items)
        if src.data_ptr() % 4:                               # (a single request that is a view starting off a dword)
            src = src.clone()
        assert src.numel() == table.arena_bytes
        _, p = O.tile_cut(src, out, table.desc_dev, table.pos_dev, n=len(items), planes=table.planes, px_bytes=table.px_bytes, tw=table.tw, th=table.th,
                          tiles_capacity=layout.T, grid_units=table.units_cut)
        lib.check(lib.lib.i2i_tile_cut(C.addressof(p), 0, stream))
    return out


def _request_list(images, what):
    if torch.is_tensor(images):
        assert images.dim() == 4, "%s: a stacked batch is [B, ...] with three more dimensions" % what
        return list(images.unbind(0))
    items = list(images)
    if not items:
        raise ValueError("%s: no requests" % what)
    return items


def tile_cut_u8(images, tile, overlap, lib=None):
    """Every tile of every request in ONE launch (i2i_tile_cut): ``images`` a uint8 [B, H, W, C] tensor or a list of uint8 [H_b, W_b, C]
    tensors of different sizes on one device (same C <= 4) -> (tiles uint8 [T, th, tw, C], the TileLayout).  ``tile`` = (tw, th); bit-equal to
    slicing.  Asynchronous on the current stream."""
    lib = lib or _capi.default_library()
    items = _request_list(images, "tile_cut_u8")
    c, dev = int(items[0].shape[-1]), items[0].device
    if not (1 <= c <= 4) or any(t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != c or t.device != dev for t in items):
        raise ValueError("tile_cut_u8: uint8 [H, W, C] requests that share the channel count (1..4) and the device")
    layout = tile_layout([t.shape[:2] for t in items], tile, overlap)
    out = torch.empty((layout.T, layout.tile[1], layout.tile[0], c), dtype=torch.uint8, device=dev)
    return _tile_cut(items, layout, layout.table(1, c, 1, dev), out, lib), layout


def tile_cut_planes(fields, layout, lib=None, div=8):
    """The noise rule: ``fields`` a list of fp32 [P, ceil(H_b / div), ceil(W_b / div)] tensors (or one stacked [B, P, ., .]), one per request
    of ``layout`` -> fp32 [T, P, th / div, tw / div], tile t the crop of its request's field at (y0 // div, x0 // div).  One launch."""
    lib = lib or _capi.default_library()
    items = _request_list(fields, "tile_cut_planes")
    planes, dev = int(items[0].shape[0]), items[0].device
    want = [(planes, -(-h // div), -(-w // div)) for h, w in layout.sizes]
    if len(items) != len(want) or any(t.dtype != torch.float32 or tuple(t.shape) != s or t.device != dev for t, s in zip(items, want)):
        raise ValueError("tile_cut_planes: fp32 fields of shapes %s expected, got %s" % (want, [tuple(t.shape) for t in items]))
    if layout.tile[0] % div or layout.tile[1] % div:
        raise ValueError("tile_cut_planes: the tile %s is not a multiple of %d" % (layout.tile, div))
    out = torch.empty((layout.T, planes, layout.tile[1] // div, layout.tile[0] // div), dtype=torch.float32, device=dev)
    return _tile_cut(items, layout, layout.table(planes, 4, div, dev), out, lib)


def tile_blend_u8(tiles, layout, lib=None, *, ramp=None, stack=False):
    """The inverse of tile_cut_u8 (i2i_tile_blend_u8, one launch): ``tiles`` uint8 [T, th, tw, C] tile outputs -> a list of uint8
    [H_b, W_b, C] images (views of one arena), or with ``stack=True`` one [B, H, W, C] tensor.  Overlaps are blended with the integer
    feather of i2i_tile_blend_u8_params; ``ramp`` defaults to max(overlap, 1).  Asynchronous on the current stream."""
    lib = lib or _capi.default_library()
    tw, th = layout.tile
    assert tiles.dtype == torch.uint8 and tiles.dim() == 4 and tuple(tiles.shape[:3]) == (layout.T, th, tw) and 1 <= tiles.shape[-1] <= 4
    c, dev = int(tiles.shape[-1]), tiles.device
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    from . import ops as O
    table = layout.table(1, c, 1, dev)
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        dst = torch.empty(max(table.arena_bytes, 4), dtype=torch.uint8, device=dev)
        _, p = O.tile_blend_u8(tiles.contiguous(), dst, table.desc_dev, table.pos_dev, n=len(layout.sizes), c=c,
                               ramp=max(layout.overlap, 1) if ramp is None else int(ramp), tw=tw, th=th, tiles_capacity=layout.T,
                               grid_units=table.units_blend)
        lib.check(lib.lib.i2i_tile_blend_u8(C.addressof(p), 0, stream))
    views = [dst[o:o + h * w * c].view(h, w, c) for o, (h, w) in zip(table.offs, layout.sizes)]
    if not stack:
        return views
    h, w = layout.sizes[0]
    return dst[:len(views) * h * w * c].view(len(views), h, w, c) if (h * w * c) % 4 == 0 and len(set(layout.sizes)) == 1 else torch.stack(views)


# ---- JPEG files on the device: i2i_jpeg_encode_u8 (include/i2i_turbo.h), five launches for any number of images of any sizes ----
JPEG_IMAGE_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("c", "<i4"), ("quality", "<i4"), ("subsampling", "<i4"),
                             ("capacity", "<i4"), ("reserved", "<i4", (2,))])
assert JPEG_IMAGE_DTYPE.itemsize == 48
JPEG_SUBSAMPLINGS = {"4:4:4": 0, "4:2:0": 2, 0: 0, 2: 2}     # the names and Pillow's numbers


def jpeg_blocks(h, w, subsampling):
    """8 x 8 blocks of an image in scan order, dummy blocks included (the unit of i2i_jpeg_encode_u8's capacity hint)."""
    if JPEG_SUBSAMPLINGS[subsampling] == 2:
        return 6 * (-(-h // 16)) * (-(-w // 16))
    return 3 * (-(-h // 8)) * (-(-w // 8))


def jpeg_capacity(h, w, subsampling):
    """Default bytes reserved for one file: header, EOI and 128 bytes per block, i.e. two bytes per sample.  Uniform noise and random 0 / 255
    pixels at quality 100 need up to 102 bytes per block (tests/jpeg_ref.py), twice what 3 bytes per pixel holds for 4:4:4; the hard bound
    of the format is 416 (1660 bits per block, every byte stuffed), which a caller who needs it passes as ``capacity=``."""
    return _capi.JPEG_HEADER_BYTES + 2 + 128 * jpeg_blocks(h, w, subsampling)


def _per_image(value, n, what):
    vals = list(value) if isinstance(value, (list, tuple)) else [value] * n
    if len(vals) != n:
        raise ValueError("jpeg_encode_u8: %d %s for %d images" % (len(vals), what, n))
    return vals


def jpeg_encode_u8(images, quality=75, subsampling="4:2:0", *, capacity=None, lib=None, return_tensors=False, max_blocks=None):
    """Baseline JPEG files of a batch, byte-identical to ``Image.fromarray(x).save(f, "JPEG", quality=, subsampling=)`` of Pillow with
    libjpeg-turbo (i2i_jpeg_encode_u8: five launches whatever the batch holds).  ``images``: a uint8 [B, H, W, C] tensor or a list of uint8
    [H_b, W_b, C] tensors of different sizes on one device, C = 3 or 1 (grey, replicated); ``quality`` (1 .. 100) and ``subsampling``
    ("4:4:4" / "4:2:0", or Pillow's 0 / 2): one value or one per image; the defaults are Pillow's.  ``capacity``: bytes reserved per file
    (one value or one per image; default jpeg_capacity).  ``max_blocks``: the capacity hint that sizes grids and workspace (default: the
    largest image's blocks; results do not depend on it).  Returns a list of ``bytes`` after ONE synchronisation and ONE copy of the used
    bytes; an image that was flagged (its file does not fit its capacity) raises I2IError naming its index.  ``return_tensors=True``:
    (pool uint8, offsets list, lengths int32 [B] on the device, bad_mask int32 [1]) without any synchronisation."""
    lib = lib or _capi.default_library()
    items = _request_list(images, "jpeg_encode_u8")
    n, dev = len(items), items[0].device
    c = int(items[0].shape[-1]) if items[0].dim() == 3 else 0
    if c not in (1, 3) or any(t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != c or t.device != dev for t in items):
        raise ValueError("jpeg_encode_u8: uint8 [H, W, C] images that share the channel count (3 or 1) and the device")
    if any(not (1 <= t.shape[0] <= 65535 and 1 <= t.shape[1] <= 65535) for t in items):
        raise ValueError("jpeg_encode_u8: image extents must be 1 .. 65535")
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    quals = [int(q) for q in _per_image(quality, n, "qualities")]
    try:
        subs = [JPEG_SUBSAMPLINGS[s] for s in _per_image(subsampling, n, "subsamplings")]
    except (KeyError, TypeError):
        raise ValueError("jpeg_encode_u8: subsampling must be \"4:4:4\" or \"4:2:0\" (0 or 2), got %r" % (subsampling,))
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in items]
    caps = [jpeg_capacity(h, w, s) for (h, w), s in zip(sizes, subs)] if capacity is None else [int(v) for v in _per_image(capacity, n, "capacities")]
    blocks = max(jpeg_blocks(h, w, s) for (h, w), s in zip(sizes, subs))
    max_blocks = blocks if max_blocks is None else int(max_blocks)
    desc = np.zeros(n, dtype=JPEG_IMAGE_DTYPE)
    src_off = dst_off = 0
    offsets = []
    for b, ((h, w), q, s, cap) in enumerate(zip(sizes, quals, subs, caps)):
        desc[b] = (src_off, dst_off, h, w, c, q, s, cap, (0, 0))
        offsets.append(dst_off)
        src_off += _align4(h * w * c)
        dst_off += cap
    from . import ops as O
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        src = _pack_arena(items)
        if src.data_ptr() % 4:
            src = src.clone()
        desc_dev = torch.from_numpy(desc.view(np.int64).reshape(-1).copy()).to(dev)
        pool = torch.empty(max(dst_off, 4), dtype=torch.uint8, device=dev)
        state = torch.zeros(n + 1, dtype=torch.int32, device=dev)               # lengths [n], then the flag word
        ws = torch.empty(max(lib.jpeg_workspace_bytes(n, max_blocks), 16), dtype=torch.uint8, device=dev)
        p = O.jpeg_encode_u8(src, pool, desc_dev, state, ws, n=n, max_blocks=max_blocks, bad_mask=state[n:], dst_bytes=dst_off)
        lib.check(lib.lib.i2i_jpeg_encode_u8(C.addressof(p), 0, stream))
    if return_tensors:
        return pool, offsets, state[:n], state[n:]
    host = state.cpu().numpy()                                                   # the one synchronisation
    lengths = host[:n].astype(np.int64)
    bad = [b for b in range(n) if lengths[b] == 0]
    if bad or host[n]:
        raise _capi.I2IError("jpeg_encode_u8: image %d does not fit its capacity of %d bytes (or its descriptor was refused); flagged: %s"
                             % (bad[0] if bad else -1, caps[bad[0]] if bad else 0, bad))
    if n == 1 or int(lengths.sum()) * 2 >= dst_off:
        used = pool[:offsets[-1] + int(lengths[-1])].cpu().numpy()
        return [used[o:o + int(l)].tobytes() for o, l in zip(offsets, lengths)]
    idx = torch.cat([torch.arange(o, o + int(l), device=dev) for o, l in zip(offsets, lengths)])   # the used bytes only, one copy
    used = pool[idx].cpu().numpy()
    ends = np.cumsum(lengths)
    return [used[e - l:e].tobytes() for e, l in zip(ends, lengths)]


def jpeg_argument(jpeg, n, variations=1):
    """``jpeg=`` of the models' forward_u8 -> (qualities, subsamplings), one per output file (n inputs x V variations, image-major).
    ``True``: Pillow's defaults (75, "4:2:0"); an int: the quality; ``(quality, subsampling)``; a LIST of n such entries, one per input."""
    def one(e):
        if e is True:
            return 75, 2
        if isinstance(e, tuple) and len(e) == 2:
            q, s = e
        else:
            q, s = e, "4:2:0"
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or isinstance(s, bool) or s not in JPEG_SUBSAMPLINGS:
            raise ValueError("jpeg=%r: True, a quality (int), (quality, \"4:4:4\" | \"4:2:0\"), or a list of one such entry per image" % (jpeg,))
        return int(q), JPEG_SUBSAMPLINGS[s]
    if isinstance(jpeg, list):
        if len(jpeg) != n:
            raise ValueError("jpeg= holds %d entries for %d images" % (len(jpeg), n))
        entries = [one(e) for e in jpeg for _ in range(variations)]
    else:
        entries = [one(jpeg)] * (n * variations)
    return [q for q, _ in entries], [s for _, s in entries]


def jpeg_files(result, spec, lib):
    """What forward_u8 returned (the uint8 images, or a tuple that starts with them) with the images replaced by their JPEG files."""
    rest = ()
    if isinstance(result, tuple):
        result, rest = result[0], result[1:]
    files = jpeg_encode_u8(result, spec[0], spec[1], lib=lib)
    return (files,) + rest if rest else files


# ---- PNG files on the device: i2i_png_encode_u8 (include/i2i_turbo.h), six launches for any number of images of any sizes ----
PNG_IMAGE_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("c", "<i4"), ("flags", "<i4"), ("capacity", "<i4"),
                            ("reserved", "<i4", (3,))])
assert PNG_IMAGE_DTYPE.itemsize == 48


def png_stream_bytes(h, w, c):
    """Bytes of the filtered scanline stream, h * (1 + w * c): the unit of i2i_png_encode_u8's capacity hint."""
    return h * (1 + w * c)


def png_encode_u8(images, *, invert=False, lib=None, capacity=None, return_tensors=False, max_bytes=None):
    """PNG files of a batch (i2i_png_encode_u8: six launches whatever the batch holds): the container and the filtered scanline stream of
    ``Image.fromarray(x).save(f, "PNG")``, the deflate stream this project's own (lossless either way: the files decode to the input).
    ``images``: a uint8 [B, H, W, C] tensor or a list of uint8 [H_b, W_b, C] / [H_b, W_b] tensors of different sizes on one
    device, C = 3 (RGB) or 1 (grey); ``invert`` (one value or one per image): 255 - x is encoded, the script's canny_viz_inv.  ``capacity``:
    bytes reserved per file (one value or one per image; default Library.png_bound, which no file exceeds).  ``max_bytes``: the capacity
    hint that sizes grids and workspace (default: the largest image's filtered stream; results do not depend on it).  Returns a list of
    ``bytes`` after ONE synchronisation and ONE copy of the used bytes; an image that was flagged (its file does not fit its capacity) raises
    I2IError naming its index.  ``return_tensors=True``: (pool uint8, offsets list, lengths int32 [B] on the device, bad_mask int32 [1])
    without any synchronisation."""
    lib = lib or _capi.default_library()
    items = _request_list(images, "png_encode_u8")
    items = [t.unsqueeze(-1) if t.dim() == 2 else t for t in items]
    n, dev = len(items), items[0].device
    c = int(items[0].shape[-1]) if items[0].dim() == 3 else 0
    if c not in (1, 3) or any(t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != c or t.device != dev for t in items):
        raise ValueError("png_encode_u8: uint8 [H, W, C] or [H, W] images that share the channel count (3 or 1) and the device")
    if any(not (1 <= t.shape[0] <= 65535 and 1 <= t.shape[1] <= 65535) for t in items):
        raise ValueError("png_encode_u8: image extents must be 1 .. 65535")
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in items]
    flags = [1 if v else 0 for v in (list(invert) if isinstance(invert, (list, tuple)) else [invert] * n)]
    if len(flags) != n:
        raise ValueError("png_encode_u8: %d invert flags for %d images" % (len(flags), n))
    caps = [lib.png_bound(w, h, c) for h, w in sizes] if capacity is None else [int(v) for v in (list(capacity) if isinstance(capacity, (list, tuple)) else [capacity] * n)]
    if len(caps) != n:
        raise ValueError("png_encode_u8: %d capacities for %d images" % (len(caps), n))
    largest = max(png_stream_bytes(h, w, c) for h, w in sizes)
    max_bytes = largest if max_bytes is None else int(max_bytes)
    if largest > _capi.PNG_MAX_BYTES:
        raise ValueError("png_encode_u8: an image of %d filtered bytes exceeds the entry's 2^27" % largest)
    desc = np.zeros(n, dtype=PNG_IMAGE_DTYPE)
    src_off = dst_off = 0
    offsets = []
    for b, ((h, w), f, cap) in enumerate(zip(sizes, flags, caps)):
        desc[b] = (src_off, dst_off, h, w, c, f, cap, (0, 0, 0))
        offsets.append(dst_off)
        src_off += _align4(h * w * c)
        dst_off += cap
    from . import ops as O
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        src = _pack_arena(items)
        desc_dev = torch.from_numpy(desc.view(np.int64).reshape(-1).copy()).to(dev)
        pool = torch.empty(max(dst_off, 4), dtype=torch.uint8, device=dev)
        state = torch.zeros(n + 1, dtype=torch.int32, device=dev)               # lengths [n], then the flag word
        ws = torch.empty(max(lib.png_workspace_bytes(n, max_bytes), 16), dtype=torch.uint8, device=dev)
        p = O.png_encode_u8(src, pool, desc_dev, state, ws, n=n, max_bytes=max_bytes, bad_mask=state[n:], dst_bytes=dst_off)
        lib.check(lib.lib.i2i_png_encode_u8(C.addressof(p), 0, stream))
    if return_tensors:
        return pool, offsets, state[:n], state[n:]
    host = state.cpu().numpy()                                                   # the one synchronisation
    lengths = host[:n].astype(np.int64)
    bad = [b for b in range(n) if lengths[b] == 0]
    if bad or host[n]:
        raise _capi.I2IError("png_encode_u8: image %d does not fit its capacity of %d bytes (or its descriptor was refused); flagged: %s"
                             % (bad[0] if bad else -1, caps[bad[0]] if bad else 0, bad))
    if n == 1 or int(lengths.sum()) * 2 >= dst_off:
        used = pool[:offsets[-1] + int(lengths[-1])].cpu().numpy()
        return [used[o:o + int(l)].tobytes() for o, l in zip(offsets, lengths)]
    idx = torch.cat([torch.arange(o, o + int(l), device=dev) for o, l in zip(offsets, lengths)])   # the used bytes only, one copy
    used = pool[idx].cpu().numpy()
    ends = np.cumsum(lengths)
    return [used[e - l:e].tobytes() for e, l in zip(ends, lengths)]


def png_argument(png, jpeg=None):
    """``png=`` of the models' forward_u8: None / False (off) or True; anything else, or ``png=`` beside ``jpeg=``, is refused."""
    if png is None or png is False:
        return False
    if png is not True:
        raise ValueError("png=%r: True or None (PNG has no settings here)" % (png,))
    if jpeg is not None:
        raise ValueError("png= and jpeg= together: one call returns one kind of file")
    return True


def png_files(result, lib, images=True, edges=False):
    """What forward_u8 returned (the uint8 images, or a tuple that starts with them): with ``images`` the images are replaced by their PNG
    files, with ``edges`` the second entry (the uint8 edge maps the generator saw) by the PNG files of the INVERTED maps, the script's
    ``canny_viz_inv.save(..._canny.png)`` (src/inference_paired.py:48-49)."""
    rest = ()
    if isinstance(result, tuple):
        result, rest = result[0], result[1:]
    if edges:
        rest = (png_encode_u8(rest[0], invert=True, lib=lib),) + rest[1:]
    if images:
        result = png_encode_u8(result, lib=lib)
    return (result,) + rest if rest else result


def canny_thresholds(low, high):
    """The two ints the kernels compare against: float thresholds floored (the magnitudes are integers, so ``mag > floor(t)`` is
    ``mag > t``); the kernels swap them if low > high."""
    return int(math.floor(low)), int(math.floor(high))


def sigma_to_q16(sigma):
    """sigma of the median rule as the kernels take it (i2i_canny_auto_thr_params.sigma_q16): the one place this conversion lives."""
    return int(round(sigma * 65536))


def sigma_q16_list(sigma, n):
    """``sigma`` (a scalar, or a sequence of n values whose None entries mean "leave that image's pair untouched") -> n int32 values;
    None becomes -1, anything outside 0 .. 1 is refused."""
    vals = list(sigma) if isinstance(sigma, (list, tuple)) else [sigma] * n
    if len(vals) != n:
        raise ValueError("%d sigma values for %d images" % (len(vals), n))
    out = []
    for v in vals:
        if v is None:
            out.append(-1)
            continue
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError("sigma = %r outside 0 .. 1" % (v,))
        out.append(sigma_to_q16(float(v)))
    return out


def canny_auto_thresholds(images, sigma=0.33, lib=None, *, thr=None):
    """The median rule ("auto-Canny") on the device: images uint8 [N, H, W, C] (C <= 4) -> (thr int32 [N, 2] = {low, high} per image,
    median2 uint32 bits [N] (an int32 tensor) = twice the median of ALL bytes of the image), both on the device, with
    low = max(0, (1 - sigma) * median), high = min(255, (1 + sigma) * median) in the integer form of i2i_canny_auto_thr_params
    (include/i2i_turbo.h; tests/canny_auto_ref.py is its CPU oracle).  The rule is not part of the reference, and sigma = 0.33 is its
    customary default, not a tuned value.  ``sigma``: a scalar or a sequence of N; a None entry leaves that image's row of ``thr`` (zeros
    unless the caller passes its own table) and of median2 untouched.  Asynchronous on the current stream: three launches, no read-back."""
    assert images.dtype == torch.uint8 and images.dim() == 4 and 1 <= images.shape[-1] <= 4
    lib = lib or _capi.default_library()
    n, h, w, c = images.shape
    src = images.contiguous()
    dev = src.device
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    sq = sigma_q16_list(sigma, n)
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        sig = torch.tensor(sq, dtype=torch.int32).to(dev)
        if thr is None:
            thr = torch.zeros(n, 2, dtype=torch.int32, device=dev)
        assert thr.dtype == torch.int32 and thr.shape == (n, 2) and thr.is_contiguous() and thr.device == dev
        med = torch.zeros(n, dtype=torch.int32, device=dev)
        ws = torch.empty(max(lib.canny_auto_ws_bytes(n), 16), dtype=torch.uint8, device=dev)
        p = _capi.CannyAutoThrParams()
        p.src, p.sigma_q16, p.thr, p.median2, p.ws = src.data_ptr(), sig.data_ptr(), thr.data_ptr(), med.data_ptr(), ws.data_ptr()
        p.n, p.h, p.w, p.c = n, h, w, c
        lib.check(lib.lib.i2i_canny_auto_thr(C.addressof(p), 0, stream))
    return thr, med


def canny_u8(images, low=100, high=200, out_channels=3, lib=None, *, sigma=0.33):
    """images: uint8 [N, H, W, C] (C <= 4) on the device -> uint8 [N, H, W, out_channels] (1 or 3), 255 on edges: ``cv2.Canny(img, low,
    high)`` (aperture 3, L1 gradient) per image, replicated over the channels as ``canny_from_pil`` does (src/image_prep.py:6-12).  The
    contract is spelled out at i2i_canny_u8_params (include/i2i_turbo.h), tests/canny_ref.py is its CPU oracle; parity with OpenCV itself is
    unpinned where cv2 is not installed.  Asynchronous on the current stream (five launches in csrc/resize.hip, no read-back).
    ``low`` / ``high`` may also be sequences of N values, one pair per image (i2i_canny_u8_batch_params: image b of the result is what a
    call on image b alone with its pair gives, bit for bit); a scalar beside a sequence holds for every image.
    ``low="auto"``: the thresholds come from the images themselves (canny_auto_thresholds with ``sigma``, a scalar or one per image) and feed
    the per-image entry without leaving the device; ``high`` is ignored."""
    assert images.dtype == torch.uint8 and images.dim() == 4 and 1 <= images.shape[-1] <= 4
    lib = lib or _capi.default_library()
    n, h, w, c = images.shape
    src = images.contiguous()
    dev = src.device
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    auto = isinstance(low, str)
    if auto:
        if low != "auto":
            raise ValueError("canny_u8: low = %r (a number, a sequence, or \"auto\")" % (low,))
        if any(v is None for v in (sigma if isinstance(sigma, (list, tuple)) else [sigma])):
            raise ValueError("canny_u8(low=\"auto\"): every image needs a sigma (None has no pair to fall back to here)")
        thr_auto, _ = canny_auto_thresholds(src, sigma, lib)
    per_image = auto or not all(isinstance(v, (int, float)) for v in (low, high))
    if per_image and not auto:
        lows, highs = [(list(v) if not isinstance(v, (int, float)) else [v] * n) for v in (low, high)]
        if len(lows) != n or len(highs) != n:
            raise ValueError("canny_u8: %d low / %d high thresholds for %d images" % (len(lows), len(highs), n))
        pairs = [canny_thresholds(a, b) for a, b in zip(lows, highs)]
    elif not auto:
        lo, hi = canny_thresholds(low, high)
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        out = torch.empty((n, h, w, int(out_channels)), dtype=torch.uint8, device=dev)
        ws = torch.empty(max(lib.canny_ws_bytes(n, h, w), 16), dtype=torch.uint8, device=dev)
        if per_image:
            thr = thr_auto if auto else torch.tensor(pairs, dtype=torch.int32).reshape(n, 2).to(dev)
            q = _capi.CannyU8BatchParams()
            q.src, q.dst, q.ws, q.thr = src.data_ptr(), out.data_ptr(), ws.data_ptr(), thr.data_ptr()
            q.n, q.h, q.w, q.c, q.out_c = n, h, w, c, int(out_channels)
            lib.check(lib.lib.i2i_canny_u8_batch(C.addressof(q), 0, stream))
            return out
        p = _capi.CannyU8Params()
        p.src, p.dst, p.ws, p.thr_dev = src.data_ptr(), out.data_ptr(), ws.data_ptr(), 0
        p.n, p.h, p.w, p.c, p.out_c, p.low, p.high = n, h, w, c, int(out_channels), lo, hi
        lib.check(lib.lib.i2i_canny_u8(C.addressof(p), 0, stream))
    return out


def resize_to_multiple_of_8(images, lib=None, *, resample="lanczos"):
    """src/inference_paired.py:38-41 on the device: LANCZOS resize to (w - w % 8, h - h % 8)."""
    h, w = images.shape[1], images.shape[2]
    return lanczos_resize_u8(images, (w - w % 8, h - h % 8), lib, resample=resample)


def apply_image_prep(images, image_prep, lib=None):
    """The inference-time options of the reference's ``build_transform`` (src/my_utils/training_utils.py:184-215, used at
    src/inference_unpaired.py:40) on a uint8 HWC batch on the device:
      "resize_512x512" / "resize_512", "resize_256x256" / "resize_256"  -> Resize((S, S), LANCZOS)
      "resized_crop_512"  -> Resize(512, LANCZOS) (shorter side to 512, torchvision's size rule) then CenterCrop(512)
      "no_resize"         -> identity
    The random training augmentation ("resize_286_randomcrop_256x256_hflip") is out of scope (training)."""
    h, w = images.shape[1], images.shape[2]
    if image_prep == "no_resize":
        return images
    if image_prep in ("resize_256", "resize_256x256"):
        return lanczos_resize_u8(images, (256, 256), lib)
    if image_prep in ("resize_512", "resize_512x512"):
        return lanczos_resize_u8(images, (512, 512), lib)
    if image_prep == "resized_crop_512":
        size = 512
        short, long = (w, h) if w <= h else (h, w)
        new_long = int(size * long / short)                      # torchvision _compute_resized_output_size
        ow, oh = (size, new_long) if w <= h else (new_long, size)
        r = lanczos_resize_u8(images, (ow, oh), lib)
        top, left = int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))      # torchvision center_crop
        return r[:, top:top + size, left:left + size].contiguous()
    raise ValueError("image_prep %r is a training-time augmentation or unknown (supported: resize_256[x256], resize_512[x512], "
                     "resized_crop_512, no_resize)" % (image_prep,))

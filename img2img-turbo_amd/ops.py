"""Op-descriptor builders: torch tensors (as raw pointers + shapes) -> i2i_op parameter structs.

Pure plumbing.  Every function returns ``(opcode, params)`` for ``_capi.Program.add``; nothing here
computes.  Activations are NHWC / token-major tensors whose last-dim stride is 1.
"""
import torch

from . import _capi as K

DT = {torch.float32: K.F32, torch.bfloat16: K.BF16, torch.float16: K.F16}
TORCH_DT = {K.F32: torch.float32, K.BF16: torch.bfloat16, K.F16: torch.float16}


def ptr(t):
    return 0 if t is None else t.data_ptr()


def _keep(p, *tensors):
    """The descriptors carry raw pointers only; pin the tensors to the descriptor so a temporary passed by a caller
    cannot be freed while a program still references it."""
    p._keep = tuple(t for t in tensors if t is not None)
    return p


def conv(x0, w, out, *, nimg, hin, win, ho, wo, ks, stride=1, pad=0, ups=0, x1=None, c0=None, c1=0,
         lda0=None, lda1=None, N=None, ldb=None, gn_ss=None, act=0, bias=None, bias_mode=None, alpha=1.0,
         res=None, ldr=None, ldc=None, geglu=0, out_f32=0, tile=0, splitk=0, ws=None, subpix=0, up_size=None, act_out=0, k2=None):
    """Implicit-GEMM conv / linear over NHWC sources.  ``w`` is packed [N][ks*ks*(c0+c1)]."""
    p = K.IgemmParams()
    c0 = x0.shape[-1] if c0 is None else c0
    p.a0, p.a1 = ptr(x0), ptr(x1)
    p.c0, p.c1 = c0, c1
    p.lda0 = lda0 if lda0 is not None else x0.shape[-1]
    p.lda1 = (lda1 if lda1 is not None else x1.shape[-1]) if x1 is not None else 0
    p.nimg, p.hin, p.win, p.ho, p.wo = nimg, hin, win, ho, wo
    p.ks, p.stride, p.pad, p.ups = ks, stride, pad, ups
    p.b = ptr(w)
    p.K = ks * ks * (c0 + c1)
    p.ldb = ldb if ldb is not None else w.shape[-1]
    p.M = nimg * ho * wo
    p.N = N if N is not None else w.shape[0]
    p.gn_ss, p.act = ptr(gn_ss), act
    p.bias = ptr(bias)
    p.bias_mode = (1 if bias is not None else 0) if bias_mode is None else bias_mode
    p.alpha = alpha
    p.res = ptr(res)
    p.ldr = (ldr if ldr is not None else res.shape[-1]) if res is not None else 0
    p.c = ptr(out)
    p.ldc = ldc if ldc is not None else out.shape[-1]
    p.zcount, p.zh_count = 1, 1
    p.geglu, p.out_f32, p.tile = geglu, out_f32, tile
    p.splitk, p.ws, p.subpix = splitk, ptr(ws), subpix
    p.up_h, p.up_w = up_size if up_size else (0, 0)
    p.act_out = act_out
    if k2 is not None:      # (tensor [nimg][ho][wo][ld], weights [N][ldb], channels): second contraction, see i2i_igemm_params.k2_a
        k2a, k2b, k2c = k2
        p.k2_a, p.k2_b, p.k2_c, p.k2_lda, p.k2_ldb = ptr(k2a), ptr(k2b), k2c, k2a.shape[-1], k2b.shape[-1]
    return K.OP_IGEMM, _keep(p, x0, x1, w, out, gn_ss, bias, res, ws, *(k2[:2] if k2 is not None else ()))


def bgemm(a, b, out, *, M, N, Kdim, lda, ldb, ldc, batch, heads, a_bs, b_bs, c_bs, alpha=1.0, out_f32=0,
          bias=None, bias_mode=0, tile=0):
    """Batched C[z] = alpha * A[z] . B[z]^T with z = (batch, head); strides are (per-batch, per-head) pairs."""
    p = K.IgemmParams()
    p.a0, p.a1, p.c0, p.c1, p.lda0, p.lda1 = ptr(a), 0, Kdim, 0, lda, 0
    p.a_bs_b, p.a_bs_h = a_bs
    p.nimg, p.hin, p.win, p.ho, p.wo = 1, 1, M, 1, M
    p.ks, p.stride, p.pad, p.ups = 1, 1, 0, 0
    p.b, p.ldb = ptr(b), ldb
    p.b_bs_b, p.b_bs_h = b_bs
    p.M, p.N, p.K = M, N, Kdim
    p.bias, p.bias_mode = ptr(bias), bias_mode
    p.alpha = alpha
    p.c, p.ldc = ptr(out), ldc
    p.c_bs_b, p.c_bs_h = c_bs
    p.zcount, p.zh_count = batch * heads, heads
    p.out_f32, p.tile = out_f32, tile
    return K.OP_IGEMM, _keep(p, a, b, out, bias)


def gn_stats(x0, gamma, beta, partial, ss, *, nimg, hw, groups, eps, nparts, x1=None, c0=None, c1=0,
             ld0=None, ld1=None, finalize_only=0, counters=None):
    p = K.GnStatsParams()
    p.counters = ptr(counters)
    p.x0, p.x1 = ptr(x0), ptr(x1)
    p.finalize_only = finalize_only
    p.c0 = x0.shape[-1] if c0 is None else c0
    p.c1 = c1
    p.ld0 = ld0 if ld0 is not None else x0.shape[-1]
    p.ld1 = (ld1 if ld1 is not None else x1.shape[-1]) if x1 is not None else 0
    p.nimg, p.hw, p.groups, p.eps = nimg, hw, groups, eps
    p.gamma, p.beta, p.partial, p.nparts, p.ss = ptr(gamma), ptr(beta), ptr(partial), nparts, ptr(ss)
    return K.OP_GN_STATS, _keep(p, x0, x1, gamma, beta, partial, ss, counters)


def gn_apply(x, y, ss, *, nimg, hw, c, act, ldx=0, ldy=0, ss_ld=0, ss_off=0, y_off=0, x1=None, c1=0, ldx1=0):
    """y[..., y_off:y_off+c] = act(x * scale + shift); ``y_off``/``ldy`` write a channel slice of a wider buffer.  ``x1`` / ``c1``: a second
    source whose channels follow x's (the concatenated input of an up-block resnet in one launch)."""
    p = K.GnApplyParams()
    p.x, p.ss, p.nimg, p.hw, p.c, p.act = ptr(x), ptr(ss), nimg, hw, c, act
    p.y = ptr(y) + y_off * y.element_size()
    p.ldx, p.ldy, p.ss_ld, p.ss_off = ldx, ldy, ss_ld, ss_off
    p.x1, p.c1, p.ldx1 = ptr(x1), (c1 if x1 is not None else 0), ldx1
    return K.OP_GN_APPLY, _keep(p, x, y, ss, x1)


def layernorm(x, y, gamma, beta, *, rows, c, eps=1e-5, ldx=None, ldy=None):
    p = K.LayerNormParams()
    p.x, p.y, p.gamma, p.beta = ptr(x), ptr(y), ptr(gamma), ptr(beta)
    p.rows, p.c, p.ldx, p.ldy, p.eps = rows, c, ldx or c, ldy or c, eps
    return K.OP_LAYERNORM, p


def softmax(s, pout, *, rows, cols, lds, ldp, scale):
    p = K.SoftmaxParams()
    p.s, p.p, p.rows, p.cols, p.lds, p.ldp, p.scale = ptr(s), ptr(pout), rows, cols, lds, ldp, scale
    return K.OP_SOFTMAX, p


def attention(q, k, vt, o, *, batch, heads, d, tq, tk, ldq, ldk, ldvt, ldo, q_bs, k_bs, vt_bs, o_bs, scale, causal=0, ksplit=0, ws=None):
    p = K.AttentionParams()
    p.ksplit, p.ws = ksplit, ptr(ws)
    p.q, p.k, p.vt, p.o = ptr(q), ptr(k), ptr(vt), ptr(o)
    p.batch, p.heads, p.d, p.tq, p.tk = batch, heads, d, tq, tk
    p.ldq, p.ldk, p.ldvt, p.ldo = ldq, ldk, ldvt, ldo
    p.q_bs, p.k_bs, p.vt_bs, p.o_bs, p.scale = q_bs, k_bs, vt_bs, o_bs, scale
    p.causal = causal
    return K.OP_ATTENTION, _keep(p, q, k, vt, o, ws)


def embed(ids, tok, pos, y, *, rows, T, c):
    """y[row] = tok[ids[row]] + pos[row % T]  (CLIP text embeddings; ids int64 on the device)."""
    p = K.EmbedParams()
    p.ids, p.tok, p.pos, p.y, p.rows, p.T, p.c, p.vocab = ptr(ids), ptr(tok), ptr(pos), ptr(y), rows, T, c, tok.shape[0]
    return K.OP_EMBED, _keep(p, ids, tok, pos, y)


def nchw_to_nhwc(x, y, *, n, c, h, w, cpad, mul=1.0, add=0.0, binarize_below=0):
    """x: NCHW float tensor, or a uint8 HWC image batch [n, h, w, c] (then y = x/255*mul + add, or with binarize_below = k:
    y = (x < k)*mul + add -- the sketch script's ``F.to_tensor(img) < 0.5`` is k = 128)."""
    p = K.NchwToNhwcParams()
    p.x, p.y, p.n, p.c, p.h, p.w, p.cpad = ptr(x), ptr(y), n, c, h, w, cpad
    p.src_dtype, p.mul, p.add = (K.U8 if x.dtype == torch.uint8 else DT[x.dtype]), mul, add
    p.binarize_below = int(binarize_below)
    return K.OP_NCHW_TO_NHWC, p


def canny_u8(src, dst, ws, *, n, h, w, c, out_c=3, low=100, high=200, thr_dev=None):
    """dst[n, h, w, out_c] = Canny edge map (255 / 0) of the uint8 HWC batch src[n, h, w, c]: cv2.Canny(img, low, high) replicated to out_c
    channels (src/image_prep.py:6-12).  ``ws``: a uint8 tensor of at least Library.canny_ws_bytes(n, h, w) bytes; ``thr_dev``: optional int32
    device tensor {low, high} read at run time instead of the two ints."""
    p = K.CannyU8Params()
    p.src, p.dst, p.ws, p.thr_dev = ptr(src), ptr(dst), ptr(ws), ptr(thr_dev)
    p.n, p.h, p.w, p.c, p.out_c, p.low, p.high = n, h, w, c, out_c, int(low), int(high)
    return K.OP_CANNY_U8, _keep(p, src, dst, ws, thr_dev)


def randn(dst, *, n=None, state=None, seed=0, step=0, stream_id=0, kind=K.RANDN_NORMAL):
    """dst[0 .. n-1] = seeded noise (the contract: i2i_randn_params, include/i2i_turbo.h): fp32 normal deviates (RANDN_NORMAL) or the raw
    Philox words (RANDN_RAW, dst of a 4-byte integer type); RANDN_ADVANCE (dst = None) bumps the step word of ``state``.  ``state``:
    optional 4-word device tensor {seed_lo, seed_hi, step, reserved} read at run time instead of the immediate seed / step."""
    p = K.RandnParams()
    p.dst, p.state = ptr(dst), ptr(state)
    p.n = (dst.numel() if dst is not None else 0) if n is None else int(n)
    p.seed, p.step, p.stream_id, p.kind = int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, int(stream_id) & 0xFFFFFFFF, int(kind)
    return K.OP_RANDN, _keep(p, dst, state)


def randn_batch(dst, states, *, batch, per_image=None, stream_id=0, kind=K.RANDN_NORMAL):
    """dst[b][0 .. per_image-1] = seeded noise of image b's state row (the contract: i2i_randn_batch_params): ``states`` is the device
    int32 / uint32 [batch, 4] table read at run time; RANDN_ADVANCE (dst = None) bumps the step word of every row."""
    p = K.RandnBatchParams()
    p.dst, p.states, p.batch = ptr(dst), ptr(states), int(batch)
    p.per_image = ((dst.numel() // max(int(batch), 1)) if dst is not None else 0) if per_image is None else int(per_image)
    p.stream_id, p.kind = int(stream_id) & 0xFFFFFFFF, int(kind)
    return K.OP_RANDN_BATCH, _keep(p, dst, states)


def canny_u8_batch(src, dst, ws, thr, *, n, h, w, c, out_c=3):
    """canny_u8 with one {low, high} pair per image: ``thr`` is a device int32 [n, 2] read at run time (i2i_canny_u8_batch_params)."""
    p = K.CannyU8BatchParams()
    p.src, p.dst, p.ws, p.thr = ptr(src), ptr(dst), ptr(ws), ptr(thr)
    p.n, p.h, p.w, p.c, p.out_c = n, h, w, c, out_c
    return K.OP_CANNY_U8_BATCH, _keep(p, src, dst, ws, thr)


def canny_auto_thr(src, sigma_q16, thr, ws, *, n, h, w, c, median2=None):
    """thr[b] = {low, high} of the median rule on image b of the uint8 HWC batch src[n, h, w, c] (i2i_canny_auto_thr_params): ``sigma_q16``
    device int32 [n] (sigma * 65536, negative = leave thr[b] as it is), ``thr`` device int32 [n, 2] -- the table canny_u8_batch reads --,
    ``median2`` optional device int32 / uint32 [n], ``ws``: a uint8 tensor of at least Library.canny_auto_ws_bytes(n) bytes."""
    p = K.CannyAutoThrParams()
    p.src, p.sigma_q16, p.thr, p.median2, p.ws = ptr(src), ptr(sigma_q16), ptr(thr), ptr(median2), ptr(ws)
    p.n, p.h, p.w, p.c = int(n), int(h), int(w), int(c)
    return K.OP_CANNY_AUTO_THR, _keep(p, src, sigma_q16, thr, median2, ws)


def resize_u8_ragged(src, dst, images, tables, *, n, c, axis, grid_units, bad_mask=None, src_bytes=None, dst_bytes=None, tables_len=None,
                     first_image=0):
    """One separable LANCZOS pass over a ragged batch (i2i_resize_u8_ragged_params): ``src`` / ``dst`` are uint8 arenas, ``images`` a device
    tensor holding n 48-byte descriptors from ``first_image`` on (image_ops.ragged_descriptors), ``tables`` the int32 pool of tap tables.  All
    three are read at run time; ``grid_units`` sizes the grid only."""
    p = K.ResizeU8RaggedParams()
    p.src, p.dst, p.tables, p.bad_mask = ptr(src), ptr(dst), ptr(tables), ptr(bad_mask)
    p.images = ptr(images) + 48 * int(first_image)
    p.src_bytes = src.numel() * src.element_size() if src_bytes is None else int(src_bytes)
    p.dst_bytes = dst.numel() * dst.element_size() if dst_bytes is None else int(dst_bytes)
    p.tables_len = tables.numel() if tables_len is None else int(tables_len)
    p.n, p.c, p.axis, p.grid_units = int(n), int(c), int(axis), int(grid_units)
    return K.OP_RESIZE_U8_RAGGED, _keep(p, src, dst, images, tables, bad_mask)


def tile_cut(src, dst, reqs, pos, *, n, planes, px_bytes, tw, th, tiles_capacity, grid_units, bad_mask=None, arena_bytes=None, pos_len=None):
    """Every tile of every request of a ragged batch in one launch (i2i_tile_cut_params): ``src`` the request arena, ``dst`` the tile batch
    [tiles_capacity][planes][th][tw] pixels of ``px_bytes`` bytes, ``reqs`` a device tensor of n 48-byte i2i_tile_request descriptors,
    ``pos`` the int32 pool of positions.  All are read at run time; ``grid_units`` sizes the grid only."""
    p = K.TileCutParams()
    p.src, p.dst, p.reqs, p.pos, p.bad_mask = ptr(src), ptr(dst), ptr(reqs), ptr(pos), ptr(bad_mask)
    p.arena_bytes = src.numel() * src.element_size() if arena_bytes is None else int(arena_bytes)
    p.pos_len = pos.numel() if pos_len is None else int(pos_len)
    p.n, p.planes, p.px_bytes, p.tw, p.th = int(n), int(planes), int(px_bytes), int(tw), int(th)
    p.tiles_capacity, p.grid_units = int(tiles_capacity), int(grid_units)
    return K.OP_TILE_CUT, _keep(p, src, dst, reqs, pos, bad_mask)


def tile_blend_u8(tiles, dst, reqs, pos, *, n, c, ramp, tw, th, tiles_capacity, grid_units, bad_mask=None, arena_bytes=None, pos_len=None):
    """The inverse of tile_cut for uint8 tile outputs [tiles_capacity][th][tw][c] with the integer feather of i2i_tile_blend_u8_params;
    ``dst`` is the request arena the descriptors' offsets refer to."""
    p = K.TileBlendU8Params()
    p.tiles, p.dst, p.reqs, p.pos, p.bad_mask = ptr(tiles), ptr(dst), ptr(reqs), ptr(pos), ptr(bad_mask)
    p.arena_bytes = dst.numel() * dst.element_size() if arena_bytes is None else int(arena_bytes)
    p.pos_len = pos.numel() if pos_len is None else int(pos_len)
    p.n, p.c, p.ramp, p.tw, p.th = int(n), int(c), int(ramp), int(tw), int(th)
    p.tiles_capacity, p.grid_units = int(tiles_capacity), int(grid_units)
    return K.OP_TILE_BLEND_U8, _keep(p, tiles, dst, reqs, pos, bad_mask)


def jpeg_encode_u8(src, dst, images, length, ws, *, n, max_blocks, bad_mask=None, src_bytes=None, dst_bytes=None):
    """The params of one i2i_jpeg_encode_u8 call (no opcode: an eager entry, ``lib.lib.i2i_jpeg_encode_u8(addressof(p), 0, stream)``): ``src``
    the uint8 pixel arena, ``dst`` the uint8 output pool, ``images`` a device tensor of n 48-byte i2i_jpeg_image descriptors, ``length`` device
    int32 / uint32 [n], ``ws`` a uint8 tensor of at least Library.jpeg_workspace_bytes(n, max_blocks) bytes.  Everything is read at run time;
    ``max_blocks`` sizes the grids and the workspace slots."""
    p = K.JpegEncodeU8Params()
    p.src, p.dst, p.images, p.length, p.bad_mask, p.ws = ptr(src), ptr(dst), ptr(images), ptr(length), ptr(bad_mask), ptr(ws)
    p.src_bytes = src.numel() * src.element_size() if src_bytes is None else int(src_bytes)
    p.dst_bytes = dst.numel() * dst.element_size() if dst_bytes is None else int(dst_bytes)
    p.ws_bytes = ws.numel() * ws.element_size()
    p.n, p.max_blocks = int(n), int(max_blocks)
    return _keep(p, src, dst, images, length, ws, bad_mask)


def png_encode_u8(src, dst, images, length, ws, *, n, max_bytes, bad_mask=None, src_bytes=None, dst_bytes=None):
    """The params of one i2i_png_encode_u8 call (no opcode: an eager entry, ``lib.lib.i2i_png_encode_u8(addressof(p), 0, stream)``): ``src``
    the uint8 pixel arena, ``dst`` the uint8 output pool, ``images`` a device tensor of n 48-byte i2i_png_image descriptors, ``length`` device
    int32 / uint32 [n], ``ws`` a uint8 tensor of at least Library.png_workspace_bytes(n, max_bytes) bytes.  Everything is read at run time;
    ``max_bytes`` sizes the grids and the workspace slots."""
    p = K.PngEncodeU8Params()
    p.src, p.dst, p.images, p.length, p.bad_mask, p.ws = ptr(src), ptr(dst), ptr(images), ptr(length), ptr(bad_mask), ptr(ws)
    p.src_bytes = src.numel() * src.element_size() if src_bytes is None else int(src_bytes)
    p.dst_bytes = dst.numel() * dst.element_size() if dst_bytes is None else int(dst_bytes)
    p.ws_bytes = ws.numel() * ws.element_size()
    p.n, p.max_bytes = int(n), int(max_bytes)
    return _keep(p, src, dst, images, length, ws, bad_mask)


def twin_fold(dst, bias, pre, cur, rg, *, bias_pre=None, bias_cur=None):
    """dst[N][K] (+ bias[N]) = the TwinConv fold of two packed layers at the device scale rg[0] (i2i_twin_fold_params).  ``pre`` / ``cur``:
    (w0 fp32 [N][K], A fp32 [rank][K] or None, B fp32 [N][rank] or None)."""
    p = K.TwinFoldParams()
    (w0, a0, b0), (w1, a1, b1) = pre, cur
    p.dst, p.bias, p.rg = ptr(dst), ptr(bias), ptr(rg)
    p.w_pre, p.a_pre, p.b_pre, p.bias_pre = ptr(w0), ptr(a0), ptr(b0), ptr(bias_pre)
    p.w_cur, p.a_cur, p.b_cur, p.bias_cur = ptr(w1), ptr(a1), ptr(b1), ptr(bias_cur)
    p.N, p.K = w0.shape
    p.rank_pre, p.rank_cur = (0 if a0 is None else a0.shape[0]), (0 if a1 is None else a1.shape[0])
    return K.OP_TWIN_FOLD, _keep(p, dst, bias, w0, a0, b0, bias_pre, w1, a1, b1, bias_cur, rg)


def scan(x, rec, *, rows, cols, ld=None, limit):
    """rec[0..7] (a 64-byte aligned slice of an int64 tensor holding uint64 bits) += the health record of the rows x cols view of ``x`` (the
    contract: i2i_scan_params, include/i2i_turbo.h).  The op's dtype must be the element type of ``x``."""
    p = K.ScanParams()
    p.x, p.rec = ptr(x), ptr(rec)
    p.rows, p.cols, p.ld, p.limit = int(rows), int(cols), int(cols if ld is None else ld), float(limit)
    return K.OP_SCAN, _keep(p, x, rec)


def scan_batch(x, rec, *, images, rows, cols, ld=None, img_stride=None, limit, rec_stride=64):
    """``scan`` with one record per image (i2i_scan_batch_params): image b is the rows x cols view ``img_stride`` elements behind image
    b - 1 (default: the images follow each other, rows * ld), its record lies ``rec_stride`` bytes behind the previous image's."""
    p = K.ScanBatchParams()
    p.x, p.rec = ptr(x), ptr(rec)
    ld = int(cols if ld is None else ld)
    p.images, p.rows, p.cols, p.ld, p.limit = int(images), int(rows), int(cols), ld, float(limit)
    p.img_stride, p.rec_stride = int(int(rows) * ld if img_stride is None else img_stride), int(rec_stride)
    return K.OP_SCAN_BATCH, _keep(p, x, rec)


def scan_verdict(rec, verdict, *, taps, images, mode):
    """K.VERDICT_CLEAR: zero the [taps][images][8] records; K.VERDICT_JUDGE: fold them into ``verdict`` (int32 tensor holding uint32 bits,
    [images][4] = first_bad, first_over, runs, bad_runs) -- i2i_scan_verdict_params."""
    p = K.ScanVerdictParams()
    p.rec, p.verdict = ptr(rec), ptr(verdict)
    p.taps, p.images, p.mode = int(taps), int(images), int(mode)
    return K.OP_SCAN_VERDICT, _keep(p, rec, verdict)


def digest(x, rec, *, images, rows, cols, ld=None, img_stride=None, index0=0):
    """rec[b][0..3] (an int64 tensor holding uint64 bits, 32 bytes per image) += the fingerprint {s0, s1, elements, 0} of image b's rows x cols
    view of ``x`` (the contract: i2i_digest_params, include/i2i_turbo.h).  The op's dtype must be the element type of ``x`` (K.U8 for bytes)."""
    p = K.DigestParams()
    p.x, p.rec = ptr(x), ptr(rec)
    ld = int(cols if ld is None else ld)
    p.images, p.rows, p.cols, p.ld = int(images), int(rows), int(cols), ld
    p.img_stride = int(int(rows) * ld if img_stride is None else img_stride)
    p.index0, p.kind = int(index0) & (2 ** 64 - 1), K.DIGEST_ADD
    return K.OP_DIGEST, _keep(p, x, rec)


def digest_clear(rec, *, n_records):
    """Zero ``n_records`` 32-byte fingerprint records from ``rec`` on (I2I_DIGEST_CLEAR)."""
    p = K.DigestParams()
    p.rec, p.kind, p.n_records = ptr(rec), K.DIGEST_CLEAR, int(n_records)
    return K.OP_DIGEST, _keep(p, rec)


def repeat(pairs, *, batch, variations, bytes_per_image=None):
    """dst_s = src_s.repeat_interleave(variations, 0) for up to 8 (src, dst) tensor pairs in one launch (the contract: i2i_repeat_params):
    src_s holds ``batch`` contiguous images, dst_s ``batch * variations``, image-major.  ``bytes_per_image``: one value per pair (default:
    the source's bytes / batch)."""
    p = K.RepeatParams()
    pairs = list(pairs)
    p.batch, p.variations, p.n_segments = int(batch), int(variations), len(pairs)
    for s, (src, dst) in enumerate(pairs[:K.REPEAT_MAX_SEGMENTS]):      # (more than 8: n_segments says so and the library refuses the op)
        n = (src.numel() * src.element_size() // max(int(batch), 1)) if bytes_per_image is None else int(bytes_per_image[s])
        setattr(p, "src%d" % s, ptr(src))
        setattr(p, "dst%d" % s, ptr(dst))
        setattr(p, "bytes%d" % s, n)
    return K.OP_REPEAT, _keep(p, *[t for pair in pairs for t in pair])


def nhwc_to_nchw(x, y, *, n, c, h, w, ldx, clamp=0, mul=0.0, add=0.0):
    """y: NCHW float tensor, or a uint8 HWC image batch [n, h, w, c] (then y = trunc(clamp01(x*mul+add)*255))."""
    p = K.NhwcToNchwParams()
    p.x, p.y, p.n, p.c, p.h, p.w, p.ldx = ptr(x), ptr(y), n, c, h, w, ldx
    p.dst_dtype, p.clamp = (K.U8 if y.dtype == torch.uint8 else DT[y.dtype]), clamp
    p.mul, p.add = mul, add
    return K.OP_NHWC_TO_NCHW, p


def posterior(moments, eps, u, *, n, hw, lat, ldm, ldu, sf, r=1.0, noise=None, noise_n=0, u_f32=None, moments_f32=0, r_dev=None):
    p = K.PosteriorParams()
    p.r_dev = ptr(r_dev)
    p.moments, p.eps, p.noise, p.u = ptr(moments), ptr(eps), ptr(noise), ptr(u)
    p.n, p.hw, p.lat, p.ldm, p.ldu, p.noise_n, p.sf, p.r = n, hw, lat, ldm, ldu, noise_n, sf, r
    p.u_f32, p.moments_f32 = ptr(u_f32), moments_f32
    return K.OP_POSTERIOR, p


def ddpm_postquant(u, e, y, wpq, bpq, *, n, hw, lat, ldu, lde, ldy, sqrt_abar, sqrt_1m_abar, sf, u_f32=0, e_f32=0):
    p = K.DdpmParams()
    p.u, p.e, p.y, p.wpq, p.bpq = ptr(u), ptr(e), ptr(y), ptr(wpq), ptr(bpq)
    p.n, p.hw, p.lat, p.ldu, p.lde, p.ldy = n, hw, lat, ldu, lde, ldy
    p.sqrt_abar, p.sqrt_1m_abar, p.sf, p.u_f32, p.e_f32 = sqrt_abar, sqrt_1m_abar, sf, u_f32, e_f32
    return K.OP_DDPM_POSTQUANT, p

"""ctypes binding of include/i2i_turbo.h (the C ABI of the gfx950 kernels).

The product loads exactly one library: the hipcc-built ``csrc/libi2i_turbo.so`` that sits in-tree.
There is NO fallback: if the library is missing or does not export the ABI, import-time use raises.
(Tests may pass an explicit path to a differently built twin, e.g. the CPU emulator under
tests/emu/; the product never does.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libi2i_turbo.so")

F32, BF16, F16, U8 = 0, 1, 2, 3
OP_IGEMM, OP_GN_STATS, OP_LAYERNORM, OP_SOFTMAX = 1, 2, 3, 4
OP_NCHW_TO_NHWC, OP_NHWC_TO_NCHW, OP_POSTERIOR, OP_DDPM_POSTQUANT, OP_ATTENTION, OP_GN_APPLY, OP_EMBED = 5, 6, 7, 8, 9, 10, 11
OP_LORA_MERGE = 12
OP_RESIZE_U8 = 13
OP_NOP = 14
OP_CANNY_U8 = 15
OP_RANDN = 16
OP_TWIN_FOLD = 17
OP_SCAN = 18
OP_RANDN_BATCH = 19      # ABI 14 additions: new opcodes / structs / exports only, so the version number did not move (include/i2i_turbo.h)
OP_CANNY_U8_BATCH = 20
OP_RESIZE_U8_RAGGED = 21
OP_SCAN_BATCH, OP_SCAN_VERDICT = 22, 23      # per-image health (i2i_scan_batch_params / i2i_scan_verdict_params)
OP_CANNY_AUTO_THR = 24                      # automatic per-image Canny thresholds (i2i_canny_auto_thr_params)
OP_DIGEST = 25                              # device fingerprints (i2i_digest_params)
OP_REPEAT = 26                              # variations: image-major replication of up to 8 tensors (i2i_repeat_params)
OP_TILE_CUT, OP_TILE_BLEND_U8 = 27, 28          # tiled forward: cut requests into tiles, feather-blend the tile outputs (i2i_tile_request)
REPEAT_MAX_SEGMENTS = 8
DIGEST_ADD, DIGEST_CLEAR = 0, 1             # i2i_digest_kind
ERR_UNSUPPORTED, ERR_MISMATCH = -3, -5      # i2i_status values callers tell apart (i2i_plan_verify)
FILTER_LANCZOS, FILTER_BICUBIC = 0, 1       # i2i_resample_filter
VERDICT_CLEAR, VERDICT_JUDGE = 0, 1         # i2i_verdict_mode
RANDN_NORMAL, RANDN_RAW, RANDN_ADVANCE = 0, 1, 2      # i2i_randn_kind

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
ABI_VERSION = 14         # include/i2i_turbo.h I2I_ABI_VERSION this binding was written for


class IgemmParams(C.Structure):
    _fields_ = [("a0", vp), ("a1", vp), ("c0", i32), ("c1", i32), ("lda0", i32), ("lda1", i32),
                ("a_bs_b", i64), ("a_bs_h", i64), ("nimg", i32), ("hin", i32), ("win", i32),
                ("ho", i32), ("wo", i32), ("ks", i32), ("stride", i32), ("pad", i32), ("ups", i32),
                ("b", vp), ("ldb", i32), ("b_bs_b", i64), ("b_bs_h", i64),
                ("M", i32), ("N", i32), ("K", i32), ("gn_ss", vp), ("act", i32),
                ("bias", vp), ("bias_mode", i32), ("alpha", f32),
                ("res", vp), ("ldr", i32), ("r_bs_b", i64), ("r_bs_h", i64),
                ("c", vp), ("ldc", i32), ("c_bs_b", i64), ("c_bs_h", i64),
                ("zcount", i32), ("zh_count", i32), ("geglu", i32), ("out_f32", i32), ("tile", i32),
                ("splitk", i32), ("ws", vp), ("gn_part", vp), ("gn_part_groups", i32), ("subpix", i32), ("act_out", i32), ("up_h", i32), ("up_w", i32),
                ("k2_a", vp), ("k2_b", vp), ("k2_c", i32), ("k2_lda", i32), ("k2_ldb", i32),
                ("ln_cs", vp), ("ln_eps", f32), ("n_trans", i32), ("c2", vp), ("ldc2", i32)]


class GnStatsParams(C.Structure):
    _fields_ = [("x0", vp), ("x1", vp), ("c0", i32), ("c1", i32), ("ld0", i32), ("ld1", i32),
                ("nimg", i32), ("hw", i32), ("groups", i32), ("eps", f32),
                ("gamma", vp), ("beta", vp), ("partial", vp), ("nparts", i32), ("ss", vp), ("finalize_only", i32), ("counters", vp)]


class GnApplyParams(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("ss", vp), ("nimg", i32), ("hw", i32), ("c", i32), ("act", i32),
                ("ldx", i32), ("ldy", i32), ("ss_ld", i32), ("ss_off", i32), ("x1", vp), ("c1", i32), ("ldx1", i32)]


class LayerNormParams(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("gamma", vp), ("beta", vp), ("rows", i32), ("c", i32),
                ("ldx", i32), ("ldy", i32), ("eps", f32)]


class SoftmaxParams(C.Structure):
    _fields_ = [("s", vp), ("p", vp), ("rows", i64), ("cols", i32), ("lds", i32), ("ldp", i32), ("scale", f32)]


class AttentionParams(C.Structure):
    _fields_ = [("q", vp), ("k", vp), ("vt", vp), ("o", vp),
                ("batch", i32), ("heads", i32), ("d", i32), ("tq", i32), ("tk", i32),
                ("ldq", i32), ("ldk", i32), ("ldvt", i32), ("ldo", i32),
                ("q_bs", i64), ("k_bs", i64), ("vt_bs", i64), ("o_bs", i64), ("scale", f32), ("causal", i32),
                ("ksplit", i32), ("ws", vp)]


class EmbedParams(C.Structure):
    _fields_ = [("ids", vp), ("tok", vp), ("pos", vp), ("y", vp), ("rows", i32), ("T", i32), ("c", i32), ("vocab", i32)]


class NchwToNhwcParams(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("n", i32), ("c", i32), ("h", i32), ("w", i32), ("cpad", i32),
                ("src_dtype", i32), ("mul", f32), ("add", f32), ("binarize_below", i32)]


class NhwcToNchwParams(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("n", i32), ("c", i32), ("h", i32), ("w", i32), ("ldx", i32),
                ("dst_dtype", i32), ("clamp", i32), ("mul", f32), ("add", f32)]


class PosteriorParams(C.Structure):
    _fields_ = [("moments", vp), ("eps", vp), ("noise", vp), ("u", vp),
                ("n", i32), ("hw", i32), ("lat", i32), ("ldm", i32), ("ldu", i32), ("noise_n", i32),
                ("sf", f32), ("r", f32), ("r_dev", vp), ("u_f32", vp), ("moments_f32", i32)]


class DdpmParams(C.Structure):
    _fields_ = [("u", vp), ("e", vp), ("y", vp), ("wpq", vp), ("bpq", vp),
                ("n", i32), ("hw", i32), ("lat", i32), ("ldu", i32), ("lde", i32), ("ldy", i32),
                ("sqrt_abar", f32), ("sqrt_1m_abar", f32), ("sf", f32), ("u_f32", i32), ("e_f32", i32)]


class LoraMergeParams(C.Structure):
    _fields_ = [("dst", vp), ("w0", vp), ("a", vp), ("b", vp), ("N", i32), ("K", i32), ("rank", i32), ("use_gamma", i32), ("rg", vp),
                ("kscale", vp), ("kshift", vp), ("bias0", vp), ("colsum", vp), ("bias_out", vp)]


class ResizeU8Params(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("n", i32), ("hin", i32), ("win", i32), ("c", i32), ("axis", i32), ("nout", i32), ("ksize", i32),
                ("bounds", vp), ("coeffs", vp)]


class CannyU8Params(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("n", i32), ("h", i32), ("w", i32), ("c", i32), ("out_c", i32), ("low", i32), ("high", i32),
                ("thr_dev", vp), ("ws", vp)]


class RandnParams(C.Structure):
    _fields_ = [("dst", vp), ("n", i64), ("state", vp), ("seed", C.c_uint64), ("step", C.c_uint32), ("stream_id", C.c_uint32), ("kind", i32)]


class RandnBatchParams(C.Structure):
    _fields_ = [("dst", vp), ("per_image", i64), ("batch", i32), ("states", vp), ("stream_id", C.c_uint32), ("kind", i32)]


class CannyU8BatchParams(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("n", i32), ("h", i32), ("w", i32), ("c", i32), ("out_c", i32), ("thr", vp), ("ws", vp)]


class ResizeImage(C.Structure):
    """One image of a ragged resize pass (i2i_resize_image, 48 bytes, lives in DEVICE memory: image_ops.ragged_descriptors packs it)."""
    _fields_ = [("src_off", i64), ("dst_off", i64), ("hin", i32), ("win", i32), ("nout", i32), ("ksize", i32),
                ("bounds_off", i32), ("coeffs_off", i32), ("reserved", i32 * 2)]


class ResizeU8RaggedParams(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("src_bytes", i64), ("dst_bytes", i64), ("images", vp), ("tables", vp), ("tables_len", i64),
                ("n", i32), ("c", i32), ("axis", i32), ("grid_units", i64), ("bad_mask", vp)]


class TwinFoldParams(C.Structure):
    _fields_ = [("dst", vp), ("bias", vp), ("w_pre", vp), ("a_pre", vp), ("b_pre", vp), ("bias_pre", vp),
                ("w_cur", vp), ("a_cur", vp), ("b_cur", vp), ("bias_cur", vp),
                ("N", i32), ("K", i32), ("rank_pre", i32), ("rank_cur", i32), ("rg", vp)]


class ScanParams(C.Structure):
    _fields_ = [("x", vp), ("rows", i64), ("cols", i32), ("ld", i64), ("limit", f32), ("rec", vp)]


class ScanBatchParams(C.Structure):
    _fields_ = [("x", vp), ("images", i32), ("cols", i32), ("rows", i64), ("ld", i64), ("img_stride", i64), ("limit", f32), ("rec", vp),
                ("rec_stride", i64)]


class ScanVerdictParams(C.Structure):
    _fields_ = [("rec", vp), ("taps", i32), ("images", i32), ("verdict", vp), ("mode", i32)]


class CannyAutoThrParams(C.Structure):
    _fields_ = [("src", vp), ("n", i32), ("h", i32), ("w", i32), ("c", i32), ("sigma_q16", vp), ("thr", vp), ("median2", vp), ("ws", vp)]


class DigestParams(C.Structure):
    _fields_ = [("x", vp), ("images", i32), ("cols", i32), ("rows", i64), ("ld", i64), ("img_stride", i64), ("index0", C.c_uint64), ("rec", vp),
                ("kind", i32), ("reserved", i32), ("n_records", i64)]


class RepeatParams(C.Structure):
    """i2i_repeat_params with its by-value table seg[8] = {src, dst, bytes_per_image} written out flat (src0, dst0, bytes0, src1, ..): the same
    memory, and every pointer is a plain member, which is what the plan exporter's relocation scan walks."""
    _fields_ = ([("batch", i32), ("variations", i32), ("n_segments", i32), ("reserved", i32)]
                + [f for s in range(REPEAT_MAX_SEGMENTS) for f in (("src%d" % s, vp), ("dst%d" % s, vp), ("bytes%d" % s, i64))])


class TileRequest(C.Structure):
    """One request of a tiled forward (i2i_tile_request, 48 bytes, lives in DEVICE memory: image_ops.TILE_REQUEST_DTYPE packs it)."""
    _fields_ = [("off", i64), ("h", i32), ("w", i32), ("tile0", i32), ("nx", i32), ("ny", i32), ("xs_off", i32), ("ys_off", i32), ("reserved", i32 * 3)]


class TileCutParams(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("arena_bytes", i64), ("reqs", vp), ("pos", vp), ("pos_len", i64), ("n", i32), ("planes", i32),
                ("px_bytes", i32), ("tw", i32), ("th", i32), ("tiles_capacity", i32), ("grid_units", i64), ("bad_mask", vp)]


class TileBlendU8Params(C.Structure):
    _fields_ = [("tiles", vp), ("dst", vp), ("arena_bytes", i64), ("reqs", vp), ("pos", vp), ("pos_len", i64), ("n", i32), ("c", i32),
                ("ramp", i32), ("tw", i32), ("th", i32), ("tiles_capacity", i32), ("grid_units", i64), ("bad_mask", vp)]


class JpegImage(C.Structure):
    """One image of a JPEG encode (i2i_jpeg_image, 48 bytes, lives in DEVICE memory: image_ops.JPEG_IMAGE_DTYPE packs it)."""
    _fields_ = [("src_off", i64), ("dst_off", i64), ("h", i32), ("w", i32), ("c", i32), ("quality", i32), ("subsampling", i32), ("capacity", i32),
                ("reserved", i32 * 2)]


class JpegEncodeU8Params(C.Structure):
    """i2i_jpeg_encode_u8_params: an eager entry, not a member of i2i_op (no opcode)."""
    _fields_ = [("src", vp), ("src_bytes", i64), ("dst", vp), ("dst_bytes", i64), ("images", vp), ("length", vp), ("bad_mask", vp), ("ws", vp),
                ("ws_bytes", i64), ("n", i32), ("reserved", i32), ("max_blocks", i64)]


JPEG_HEADER_BYTES = 623


class PngImage(C.Structure):
    """One image of a PNG encode (i2i_png_image, 48 bytes, lives in DEVICE memory: image_ops.PNG_IMAGE_DTYPE packs it)."""
    _fields_ = [("src_off", i64), ("dst_off", i64), ("h", i32), ("w", i32), ("c", i32), ("flags", i32), ("capacity", i32), ("reserved", i32 * 3)]


class PngEncodeU8Params(C.Structure):
    """i2i_png_encode_u8_params: an eager entry, not a member of i2i_op (no opcode)."""
    _fields_ = [("src", vp), ("src_bytes", i64), ("dst", vp), ("dst_bytes", i64), ("images", vp), ("length", vp), ("bad_mask", vp), ("ws", vp),
                ("ws_bytes", i64), ("n", i32), ("reserved", i32), ("max_bytes", i64)]


PNG_BLOCK_BYTES = 16384
PNG_MAX_BYTES = 1 << 27


class NopParams(C.Structure):
    _fields_ = [("unused", i32)]


class _OpUnion(C.Union):
    _fields_ = [("igemm", IgemmParams), ("gn_stats", GnStatsParams), ("gn_apply", GnApplyParams),
                ("layernorm", LayerNormParams), ("softmax", SoftmaxParams), ("attention", AttentionParams),
                ("to_nhwc", NchwToNhwcParams), ("to_nchw", NhwcToNchwParams), ("embed", EmbedParams),
                ("posterior", PosteriorParams), ("ddpm", DdpmParams), ("lora_merge", LoraMergeParams), ("resize_u8", ResizeU8Params),
                ("nop", NopParams), ("canny_u8", CannyU8Params), ("randn", RandnParams), ("twin_fold", TwinFoldParams), ("scan", ScanParams),
                ("randn_batch", RandnBatchParams), ("canny_u8_batch", CannyU8BatchParams), ("resize_u8_ragged", ResizeU8RaggedParams),
                ("scan_batch", ScanBatchParams), ("scan_verdict", ScanVerdictParams), ("canny_auto_thr", CannyAutoThrParams),
                ("digest", DigestParams), ("repeat", RepeatParams), ("tile_cut", TileCutParams), ("tile_blend_u8", TileBlendU8Params)]


class Op(C.Structure):
    _fields_ = [("opcode", i32), ("dtype", i32), ("u", _OpUnion)]


_FIELD_OF = {OP_IGEMM: "igemm", OP_GN_STATS: "gn_stats", OP_GN_APPLY: "gn_apply", OP_LAYERNORM: "layernorm",
             OP_SOFTMAX: "softmax", OP_ATTENTION: "attention", OP_NCHW_TO_NHWC: "to_nhwc",
             OP_NHWC_TO_NCHW: "to_nchw", OP_POSTERIOR: "posterior", OP_DDPM_POSTQUANT: "ddpm", OP_EMBED: "embed",
             OP_LORA_MERGE: "lora_merge", OP_RESIZE_U8: "resize_u8", OP_NOP: "nop", OP_CANNY_U8: "canny_u8", OP_RANDN: "randn", OP_TWIN_FOLD: "twin_fold", OP_SCAN: "scan",
             OP_RANDN_BATCH: "randn_batch", OP_CANNY_U8_BATCH: "canny_u8_batch", OP_RESIZE_U8_RAGGED: "resize_u8_ragged",
             OP_SCAN_BATCH: "scan_batch", OP_SCAN_VERDICT: "scan_verdict", OP_CANNY_AUTO_THR: "canny_auto_thr",
             OP_DIGEST: "digest", OP_REPEAT: "repeat", OP_TILE_CUT: "tile_cut", OP_TILE_BLEND_U8: "tile_blend_u8"}

EXPORTS = ["i2i_abi_version", "i2i_backend", "i2i_last_error", "i2i_sizeof_op", "i2i_igemm", "i2i_igemm_gn_parts", "i2i_igemm_route", "i2i_gn_stats",
           "i2i_gn_apply", "i2i_nop", "i2i_calib_mfma", "i2i_calib_stream", "i2i_layernorm", "i2i_softmax", "i2i_attention", "i2i_nchw_to_nhwc",
           "i2i_nhwc_to_nchw", "i2i_posterior", "i2i_ddpm_postquant", "i2i_embed", "i2i_lora_merge", "i2i_resize_u8", "i2i_canny_u8", "i2i_canny_ws_bytes", "i2i_randn", "i2i_twin_fold", "i2i_scan",
           "i2i_randn_batch", "i2i_canny_u8_batch", "i2i_resize_u8_ragged", "i2i_scan_batch", "i2i_scan_verdict", "i2i_lanczos_ksize", "i2i_lanczos_tables",
           "i2i_canny_auto_thr", "i2i_canny_auto_ws_bytes", "i2i_resample_ksize", "i2i_resample_tables",
           "i2i_merge_group_create", "i2i_merge_group_run", "i2i_merge_group_destroy", "i2i_run", "i2i_run_timed",
           "i2i_graph_create", "i2i_graph_launch", "i2i_graph_destroy",
           "i2i_plan_load", "i2i_plan_io", "i2i_plan_write", "i2i_plan_read", "i2i_plan_ops", "i2i_plan_run", "i2i_plan_destroy",
           "i2i_plan_has_scale", "i2i_plan_set_scale", "i2i_digest", "i2i_plan_verify", "i2i_repeat",
           "i2i_tile_cut", "i2i_tile_blend_u8", "i2i_tile_positions", "i2i_jpeg_encode_u8", "i2i_jpeg_workspace_bytes", "i2i_jpeg_header",
           "i2i_png_encode_u8", "i2i_png_workspace_bytes", "i2i_png_bound"]


class I2IError(RuntimeError):
    pass


def _preload_torch_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64 (same SONAME as /opt/rocm's).  Streams, events and graphs are only
    meaningful inside ONE HIP runtime instance, so make sure torch's copy is the one already mapped when the
    kernel library's DT_NEEDED entry is resolved (the loader then binds to it by SONAME)."""
    import torch
    hip = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)


def _assert_single_hip_runtime():
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    paths.add(os.path.realpath(line.split()[-1]))
    except OSError:
        return
    if len(paths) > 1:
        raise I2IError("two HIP runtimes are mapped in this process (%s): import torch before loading the kernel "
                       "library so both share one runtime" % sorted(paths))


class Library:
    """One loaded libi2i_turbo.so.  ``path`` defaults to the in-tree product build."""

    def __init__(self, path=None):
        path = path or os.environ.get("I2I_LIB") or DEFAULT_LIB      # I2I_LIB: an experiment build (csrc/build.py --tag)
        if not os.path.exists(path):
            raise I2IError(
                "HIP kernel library not found at %s -- build it with `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % path)
        self.path = path
        _preload_torch_hip_runtime()
        self.lib = C.CDLL(path)
        _assert_single_hip_runtime()
        missing = [s for s in EXPORTS if not hasattr(self.lib, s)]
        if missing:
            raise I2IError("library %s lacks ABI symbols: %s" % (path, missing))
        L = self.lib
        L.i2i_backend.restype = C.c_char_p
        L.i2i_last_error.restype = C.c_char_p
        L.i2i_sizeof_op.restype = C.c_size_t
        for name in ("i2i_igemm", "i2i_gn_stats", "i2i_gn_apply", "i2i_layernorm", "i2i_softmax", "i2i_attention",
                     "i2i_nchw_to_nhwc", "i2i_nhwc_to_nchw", "i2i_posterior", "i2i_ddpm_postquant", "i2i_embed", "i2i_lora_merge", "i2i_resize_u8", "i2i_canny_u8", "i2i_randn", "i2i_twin_fold", "i2i_scan",
                     "i2i_randn_batch", "i2i_canny_u8_batch", "i2i_resize_u8_ragged", "i2i_scan_batch", "i2i_scan_verdict", "i2i_canny_auto_thr", "i2i_digest", "i2i_repeat",
                     "i2i_tile_cut", "i2i_tile_blend_u8", "i2i_jpeg_encode_u8", "i2i_png_encode_u8"):
            getattr(L, name).argtypes = [vp, C.c_int, vp]
            getattr(L, name).restype = C.c_int
        L.i2i_canny_ws_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.i2i_canny_ws_bytes.restype = C.c_size_t
        L.i2i_canny_auto_ws_bytes.argtypes = [C.c_int]
        L.i2i_canny_auto_ws_bytes.restype = C.c_size_t
        L.i2i_resample_ksize.argtypes = [C.c_int, C.c_int, C.c_int]
        L.i2i_resample_ksize.restype = C.c_int
        L.i2i_resample_tables.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, C.c_int]
        L.i2i_resample_tables.restype = C.c_int
        L.i2i_tile_positions.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int]
        L.i2i_tile_positions.restype = C.c_int
        L.i2i_jpeg_workspace_bytes.argtypes = [C.c_int, C.c_int64]
        L.i2i_jpeg_workspace_bytes.restype = C.c_size_t
        L.i2i_jpeg_header.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.i2i_jpeg_header.restype = C.c_int
        L.i2i_png_workspace_bytes.argtypes = [C.c_int, C.c_int64]
        L.i2i_png_workspace_bytes.restype = C.c_size_t
        L.i2i_png_bound.argtypes = [C.c_int, C.c_int, C.c_int]
        L.i2i_png_bound.restype = C.c_int64
        L.i2i_lanczos_ksize.argtypes = [C.c_int, C.c_int]
        L.i2i_lanczos_ksize.restype = C.c_int
        L.i2i_lanczos_tables.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int]
        L.i2i_lanczos_tables.restype = C.c_int
        L.i2i_nop.argtypes = [vp]
        L.i2i_calib_mfma.argtypes = [C.c_int, C.c_int, vp, vp, vp]
        L.i2i_calib_stream.argtypes = [vp, vp, C.c_size_t, vp]
        L.i2i_igemm_gn_parts.argtypes = [vp, C.c_int, C.c_int]
        L.i2i_igemm_gn_parts.restype = C.c_int
        L.i2i_igemm_route.argtypes = [vp, C.c_int]
        L.i2i_igemm_route.restype = C.c_char_p
        L.i2i_run.argtypes = [vp, C.c_int, vp]
        L.i2i_run_timed.argtypes = [vp, C.c_int, vp, vp]
        L.i2i_graph_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.i2i_graph_launch.argtypes = [vp, vp]
        L.i2i_graph_destroy.argtypes = [vp]
        L.i2i_plan_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.i2i_plan_io.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.i2i_plan_write.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
        L.i2i_plan_read.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
        L.i2i_plan_ops.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int)]
        L.i2i_plan_run.argtypes = [vp, vp]
        L.i2i_plan_destroy.argtypes = [vp]
        L.i2i_plan_has_scale.argtypes = [vp]
        L.i2i_plan_set_scale.argtypes = [vp, C.c_float, C.c_float, vp]
        L.i2i_plan_verify.argtypes = [vp, vp, C.POINTER(C.c_int)]
        L.i2i_merge_group_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.i2i_merge_group_run.argtypes = [vp, vp]
        L.i2i_merge_group_destroy.argtypes = [vp]
        if L.i2i_abi_version() != ABI_VERSION:
            raise I2IError("ABI version mismatch")
        if L.i2i_sizeof_op() != C.sizeof(Op):
            raise I2IError("i2i_op layout mismatch: C %d vs ctypes %d" % (L.i2i_sizeof_op(), C.sizeof(Op)))
        self.backend = L.i2i_backend().decode()

    def check(self, rc):
        if rc != 0:
            raise I2IError("i2i error %d: %s" % (rc, self.lib.i2i_last_error().decode()))

    def canny_ws_bytes(self, n, h, w):
        """Bytes of the workspace i2i_canny_u8 needs for an [n, h, w, c] batch."""
        return int(self.lib.i2i_canny_ws_bytes(int(n), int(h), int(w)))

    def canny_auto_ws_bytes(self, n):
        """Bytes of the workspace i2i_canny_auto_thr needs for n images (one 256-bin histogram each)."""
        return int(self.lib.i2i_canny_auto_ws_bytes(int(n)))

    def resample_tables(self, filter, in_size, out_size, ksize_capacity=None):
        """lanczos_tables for any of the library's filters: ``filter`` = "lanczos" / "bicubic" or an i2i_resample_filter code
        (i2i_resample_tables, host code); bit-equal to image_ops.resample_coeffs."""
        import numpy as np
        code = {"lanczos": FILTER_LANCZOS, "bicubic": FILTER_BICUBIC}.get(filter, filter)
        ksize = int(self.lib.i2i_resample_ksize(int(code), int(in_size), int(out_size)))
        self.check(min(ksize, 0))
        cap = ksize if ksize_capacity is None else int(ksize_capacity)
        bounds = np.zeros((int(out_size), 2), dtype=np.int32)
        coeffs = np.zeros((int(out_size), max(cap, 1)), dtype=np.int32)
        got = int(self.lib.i2i_resample_tables(int(code), int(in_size), int(out_size), bounds.ctypes.data, coeffs.ctypes.data, cap))
        self.check(min(got, 0))
        return got, bounds, coeffs

    def tile_positions(self, length, tile, overlap):
        """The library's own tile positions of one axis (i2i_tile_positions, host code) as a list of ints -- what a host that is not Python
        computes; equal to image_ops.tile_positions.  Raises I2IError for arguments outside the layout rule."""
        n = int(self.lib.i2i_tile_positions(int(length), int(tile), int(overlap), None, 0))
        self.check(min(n, 0))
        out = (C.c_int32 * n)()
        self.check(min(int(self.lib.i2i_tile_positions(int(length), int(tile), int(overlap), C.addressof(out), n)), 0))
        return list(out)

    def jpeg_workspace_bytes(self, n, max_blocks):
        """Bytes of the workspace i2i_jpeg_encode_u8 needs for n images of at most ``max_blocks`` 8 x 8 blocks each."""
        return int(self.lib.i2i_jpeg_workspace_bytes(int(n), int(max_blocks)))

    def jpeg_header(self, quality, subsampling, w, h):
        """The 623 bytes i2i_jpeg_encode_u8 writes in front of the scan (i2i_jpeg_header, host code); ``subsampling``: 0 or 2."""
        out = (C.c_uint8 * JPEG_HEADER_BYTES)()
        self.check(min(int(self.lib.i2i_jpeg_header(int(quality), int(subsampling), int(w), int(h), C.addressof(out))), 0))
        return bytes(out)

    def png_workspace_bytes(self, n, max_bytes):
        """Bytes of the workspace i2i_png_encode_u8 needs for n images of at most ``max_bytes`` filtered bytes, h * (1 + w * c), each."""
        return int(self.lib.i2i_png_workspace_bytes(int(n), int(max_bytes)))

    def png_bound(self, w, h, c):
        """A file size i2i_png_encode_u8 never exceeds for a w x h x c image (i2i_png_bound, host code)."""
        n = int(self.lib.i2i_png_bound(int(w), int(h), int(c)))
        self.check(min(n, 0))
        return n

    def lanczos_tables(self, in_size, out_size, ksize_capacity=None):
        """The library's own tap tables (i2i_lanczos_tables, host code): (ksize, bounds int32 [out, 2], coeffs int32 [out, capacity]) as numpy
        arrays -- what a host that is not Python computes; bit-equal to image_ops.lanczos_coeffs."""
        import numpy as np
        ksize = int(self.lib.i2i_lanczos_ksize(int(in_size), int(out_size)))
        self.check(min(ksize, 0))
        cap = ksize if ksize_capacity is None else int(ksize_capacity)
        bounds = np.zeros((int(out_size), 2), dtype=np.int32)
        coeffs = np.zeros((int(out_size), max(cap, 1)), dtype=np.int32)
        got = int(self.lib.i2i_lanczos_tables(int(in_size), int(out_size), bounds.ctypes.data, coeffs.ctypes.data, cap))
        self.check(min(got, 0))
        return got, bounds, coeffs

    # ---- programs -------------------------------------------------------------------------------
    def igemm_gn_parts(self, params, dtype_code, groups):
        """Partial-sum slots per image the igemm op would write through gn_part (0 = its kernel cannot)."""
        return int(self.lib.i2i_igemm_gn_parts(C.addressof(params), dtype_code, groups))

    def igemm_route(self, params, dtype_code):
        """Kernel family i2i_igemm() will run this op on (reporting only)."""
        return self.lib.i2i_igemm_route(C.addressof(params), dtype_code).decode()

    def run(self, prog, stream=0):
        self.check(self.lib.i2i_run(C.addressof(prog.array), prog.n, vp(stream)))

    def run_timed(self, prog, stream=0):
        ms = (C.c_float * prog.n)()
        self.check(self.lib.i2i_run_timed(C.addressof(prog.array), prog.n, vp(stream), C.addressof(ms)))
        return list(ms)

    def graph_create(self, prog):
        g = vp()
        self.check(self.lib.i2i_graph_create(C.addressof(prog.array), prog.n, C.byref(g)))
        return g

    def graph_launch(self, g, stream=0):
        self.check(self.lib.i2i_graph_launch(g, vp(stream)))

    def graph_destroy(self, g):
        self.lib.i2i_graph_destroy(g)

    # ---- plan files (include/i2i_turbo.h, csrc/plan_file.hip; written by plan_file.export_plan) ----
    def plan_load(self, path):
        h = vp()
        self.check(self.lib.i2i_plan_load(str(path).encode(), C.byref(h)))
        return h

    def plan_io(self, h, name):
        ptr, n = vp(), C.c_size_t()
        self.check(self.lib.i2i_plan_io(h, name.encode(), C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def plan_write(self, h, name, host_tensor):
        t = host_tensor.contiguous()
        assert t.device.type == "cpu"
        self.check(self.lib.i2i_plan_write(h, name.encode(), vp(t.data_ptr()), t.numel() * t.element_size()))

    def plan_read(self, h, name, host_tensor):
        assert host_tensor.device.type == "cpu" and host_tensor.is_contiguous()
        self.check(self.lib.i2i_plan_read(h, name.encode(), vp(host_tensor.data_ptr()), host_tensor.numel() * host_tensor.element_size()))
        return host_tensor

    def plan_run(self, h, stream=0):
        self.check(self.lib.i2i_plan_run(h, vp(stream)))

    def plan_destroy(self, h):
        self.lib.i2i_plan_destroy(h)

    def plan_has_scale(self, h):
        return bool(self.lib.i2i_plan_has_scale(h))

    def plan_set_scale(self, h, r, gamma=None, stream=0):
        """New LoRA scale / skip gamma of a loaded plan exported with live_scale: enqueues its scale program on ``stream``."""
        self.check(self.lib.i2i_plan_set_scale(h, float(r), float(r if gamma is None else gamma), vp(stream)))

    def plan_verify(self, h, stream=0):
        """i2i_plan_verify of a loaded plan: (status, first_bad_buffer, message).  status 0 = every stored digest matches; ERR_MISMATCH with
        the buffer's index; ERR_UNSUPPORTED for a file exported without digests.  Does not raise: the caller tells the three apart."""
        bad = C.c_int(-1)
        rc = int(self.lib.i2i_plan_verify(h, vp(stream), C.byref(bad)))
        return rc, bad.value, ("" if rc == 0 else self.lib.i2i_last_error().decode())

    # ---- grouped LoRA re-merge (include/i2i_turbo.h i2i_merge_group_*) ----
    def merge_group_create(self, layers, dtype_code):
        """``layers``: a list of LoraMergeParams (plain form).  The handle keeps copies of the structs, not of what they point at."""
        arr = (LoraMergeParams * max(len(layers), 1))(*layers)
        g = vp()
        self.check(self.lib.i2i_merge_group_create(C.addressof(arr), len(layers), dtype_code, C.byref(g)))
        return g

    def merge_group_run(self, g, stream=0):
        self.check(self.lib.i2i_merge_group_run(g, vp(stream)))

    def merge_group_destroy(self, g):
        self.lib.i2i_merge_group_destroy(g)


class Program:
    """A flat, immutable-once-frozen array of ops (what i2i_run consumes)."""

    def __init__(self):
        self.ops = []      # (opcode, dtype, params struct, label)
        self.array = None
        self.n = 0
        self.labels = []
        self.keep = []     # python objects (tensors) that own the memory the ops point at

    def add(self, opcode, dtype, params, label=""):
        assert self.array is None, "program is frozen"
        self.ops.append((opcode, dtype, params, label))

    def freeze(self):
        self.n = len(self.ops)
        self.array = (Op * max(self.n, 1))()
        for i, (opcode, dtype, params, label) in enumerate(self.ops):
            self.array[i].opcode = opcode
            self.array[i].dtype = dtype
            setattr(self.array[i].u, _FIELD_OF[opcode], params)
        self.labels = [o[3] for o in self.ops]
        return self


_DEFAULT = None


def default_library():
    """The product library (loaded once).  Raises if the HIP build is missing."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Library()
    return _DEFAULT

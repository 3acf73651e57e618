"""Shared cases of the numerical health scan (i2i_scan, csrc/elementwise.hip) for the CPU emulator (tests/test_health_emu.py) and an MI355X
(tests/test_health_gpu.py): every record is compared bit for bit with tests/health_ref.py.

The sizes come from the kernel's constants (csrc/elementwise.hip):
    SCAN_THREADS  = 256   lanes per workgroup
    SCAN_UNROLL   = 4     16-byte chunks per lane and round  -> WG_CHUNKS = 1024 chunks = the stride of one workgroup
    SCAN_MAX_GRID = 1024  workgroups at most                 -> GRID_CHUNKS = 2^20 chunks = one pass of the whole grid
    EPC = 16 / element size (4 fp32, 8 bf16 / fp16) elements per chunk.
"""
import ctypes as C

import numpy as np
import torch

import health_ref as R

SCAN_THREADS, SCAN_UNROLL, SCAN_MAX_GRID = 256, 4, 1024
WG_CHUNKS = SCAN_THREADS * SCAN_UNROLL
GRID_CHUNKS = WG_CHUNKS * SCAN_MAX_GRID
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
FMT_OF = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
LIMIT = 1.5          # exactly representable in the three formats: "equal to the limit" and "the next value above it" exist in each


def epc(dtype):
    return 16 // torch.empty(0, dtype=dtype).element_size()


def sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def healthy_bits(n, dtype, seed):
    """n finite patterns with |x| < 1 (so nothing is over LIMIT), as the format's raw words."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(n, generator=g) * 1.9 - 0.95).to(dtype)
    return R.bits_of(t)[0].copy()


def specials(fmt):
    """One each of: +Inf, -Inf, quiet NaN, a NaN with only the lowest mantissa bit set, -0, the smallest denormal, +-max finite, a value equal
    to LIMIT, the next value above it.  Expected of them alone: 2 NaN, 1 +Inf, 1 -Inf, 3 over (the two max finite, the next above)."""
    f = R.FMT[fmt]
    inf, sign = f["inf"], f["sign"]
    quiet = inf | ((f["abs"] ^ inf) + 1) >> 1
    lim = {"f32": 0x3FC00000, "bf16": 0x3FC0, "f16": 0x3E00}[fmt]
    return np.array([inf, sign | inf, quiet, inf | 1, sign, 1, inf - 1, sign | (inf - 1), lim, lim + 1], dtype=f["word"])


def make_view(rows, cols, ld, dtype, seed, with_specials=False, pad="nan"):
    """Raw words of a rows x cols view with pitch ld; the padding [cols, ld) of every row holds NaN / Inf patterns that must not be counted."""
    fmt = FMT_OF[dtype]
    f = R.FMT[fmt]
    n = (rows - 1) * ld + cols if rows else 0
    flat = np.empty(n, dtype=f["word"])
    body = healthy_bits(rows * cols, dtype, seed).reshape(rows, cols) if rows * cols else np.zeros((0, cols), dtype=f["word"])
    if with_specials:
        sp = specials(fmt)
        pos = np.random.RandomState(seed).choice(rows * cols, size=len(sp), replace=False) if rows * cols >= len(sp) else []
        for p, v in zip(pos, sp):
            body[p // cols, p % cols] = v
    for r in range(rows):
        flat[r * ld:r * ld + cols] = body[r]
        if r < rows - 1:
            flat[r * ld + cols:(r + 1) * ld] = [(f["inf"] | 1), f["inf"]][r & 1]
    return flat


def call(lib, device, x_ptr, rows, cols, ld, limit, rec_ptr, dtype_code):
    from img2img_turbo_amd import _capi as K
    p = K.ScanParams()
    p.x, p.rows, p.cols, p.ld, p.limit, p.rec = x_ptr, rows, cols, ld, limit, rec_ptr
    hip_stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None
    rc = lib.lib.i2i_scan(C.addressof(p), dtype_code, hip_stream)
    sync(device)
    return rc


def new_rec(device):
    rec = torch.zeros(8, dtype=torch.int64, device=device)
    assert rec.data_ptr() % 64 == 0
    return rec


def read_rec(rec):
    return rec.cpu().numpy().view(np.uint64).copy()


def on_device(flat, dtype, device, offset=0):
    """The words in an allocation of their own, `offset` elements past its (16-byte aligned) start; everything around them is NaN."""
    from img2img_turbo_amd import ops as O
    f = R.FMT[FMT_OF[dtype]]
    host = np.full(offset + flat.size + 16, f["inf"] | 1, dtype=f["word"])
    host[offset:offset + flat.size] = flat
    idt = torch.int32 if f["word"] is np.uint32 else torch.int16
    buf = torch.from_numpy(host.view(np.int32 if idt is torch.int32 else np.int16)).to(device)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + offset * buf.element_size(), O.DT[dtype]


def check_view(lib, device, dtype, rows, cols, ld=None, offset=0, seed=1, with_specials=True, limit=LIMIT, launches=1, flat=None):
    """One (or several accumulated) launches over the view against the oracle, bit for bit.  Returns the record."""
    ld = cols if ld is None else ld
    if flat is None:
        flat = make_view(rows, cols, ld, dtype, seed, with_specials=with_specials)
    buf, x_ptr, code = on_device(flat, dtype, device, offset)
    rec = new_rec(device)
    one = R.scan_ref(flat, cols, ld, limit, FMT_OF[dtype], rows=rows)
    want = np.zeros(8, dtype=np.uint64)
    for _ in range(launches):
        rc = call(lib, device, x_ptr, rows, cols, ld, limit, rec.data_ptr(), code)
        assert rc == 0, (rc, lib.lib.i2i_last_error().decode())
        want = R.accumulate(want, one)
    got = read_rec(rec)
    assert np.array_equal(got, want), (str(dtype), rows, cols, ld, offset, got.tolist(), want.tolist())
    return got


# (rows, cols(epc), ld(epc), offset): what each catches is in the comment
def small_views(e):
    return [
        (1, 1, None, 0), (1, 7, None, 0),          # element loads only (fp32: one chunk + a tail of 3)
        (3, 5, 9, 0),                              # rows that do not start on 16-byte boundaries: element loads; the padding holds NaN / Inf
        (2, 8, None, 0), (5, 64, None, 0),         # chunks only
        (4, 13, 16, 0),                            # aligned rows: chunks + a row tail, padding not read
        (5, 64, None, 1), (1, 3, None, e - 1),     # base one element past a 16-byte boundary: the head peel (and a head that is the whole tensor)
        (3, 3 * e, 4 * e, 1),                      # misaligned base with a pitch: element loads
        (40, 33 * e + 3, 40 * e, 0),               # aligned rows over more than one workgroup: 1320 chunks (the 64-bit row division), tails
        (300, 7, 9, 0),                            # 2100 element loads: three workgroups of the element loop
    ]


def check_small(lib, device, dtype):
    e = epc(dtype)
    for i, (rows, cols, ld, off) in enumerate(small_views(e)):
        check_view(lib, device, dtype, rows, cols, ld, off, seed=10 + i)


def check_strides(lib, device, dtype):
    """1 x (one workgroup's stride + 3): a second workgroup with a partial round.  3 x (the whole grid's stride + 5): the second pass of
    the grid-stride loop, a last partial workgroup, and -- with 1024 workgroups -- the exactly-one-lane update of runs / elements."""
    e = epc(dtype)
    check_view(lib, device, dtype, 1, WG_CHUNKS * e + 3, seed=3)
    got = check_view(lib, device, dtype, 3, GRID_CHUNKS * e + 5, seed=4)
    assert got[0] == 1 and got[6] == 3 * (GRID_CHUNKS * e + 5)


def check_classes(lib, device, dtype):
    """The special values alone, then in a healthy tensor; an all-NaN tensor; accumulation over two launches."""
    fmt = FMT_OF[dtype]
    f = R.FMT[fmt]
    sp = specials(fmt)
    got = check_view(lib, device, dtype, 1, len(sp), flat=sp)
    max_fin = int(R.widen(np.array([f["inf"] - 1]), fmt)[0])
    assert got.tolist() == [1, 2, 1, 1, 3, max_fin, len(sp), 0], got.tolist()
    # without the two max-finite values the largest finite one is the value just above the limit
    got = check_view(lib, device, dtype, 1, 8, flat=np.delete(sp, [6, 7]))
    assert got[4] == 1 and got[5] == int(R.widen(np.array([int(sp[9])]), fmt)[0])
    # -0 and the smallest denormal alone: nothing counted, max_abs = the denormal, widened exactly
    got = check_view(lib, device, dtype, 1, 2, flat=sp[4:6].copy())
    assert got[1:5].tolist() == [0, 0, 0, 0] and got[5] == int(R.widen(np.array([1]), fmt)[0]) and got[5] != 0
    # all NaN: max_abs stays 0
    nan = np.full(5 * 64 + 3, f["inf"] | 0x15, dtype=f["word"])
    got = check_view(lib, device, dtype, 1, nan.size, flat=nan)
    assert got[1] == nan.size and got[5] == 0
    # the same launch twice without a reset: counts double, runs == 2, max idempotent
    got = check_view(lib, device, dtype, 5, 64, seed=7, launches=2)
    assert got[0] == 2 and got[6] == 2 * 5 * 64 and got[1] == 4 and got[7] == 0
    # an infinite limit: nothing finite is over it
    got = check_view(lib, device, dtype, 1, len(sp), flat=sp, limit=float("inf"))
    assert got[4] == 0


def check_refusals(lib, device):
    import pytest
    from img2img_turbo_amd import _capi as K
    flat = make_view(4, 16, 16, torch.float32, 1)
    buf, x, code = on_device(flat, torch.float32, device)
    rec = new_rec(device)
    big = torch.zeros(24, dtype=torch.int64, device=device)
    r = rec.data_ptr()
    bad = [dict(x=0), dict(rec=0),                                                    # null pointers
           dict(limit=0.0), dict(limit=-1.0), dict(limit=float("nan")),               # limit must be > 0
           dict(ld=15), dict(rows=-1), dict(cols=-1),                                 # ld < cols, negative sizes
           dict(rec=big.data_ptr() + 8),                                              # rec not 64-byte aligned
           dict(code=K.U8), dict(code=7),                                             # not a float dtype
           dict(x=x + 2)]                                                             # x not aligned to its element
    for kw in bad:
        a = dict(x=x, rows=4, cols=16, ld=16, limit=1.0, rec=r, code=code)
        a.update(kw)
        if "rec" in kw and kw["rec"]:
            assert a["rec"] % 64 != 0
        rc = call(lib, device, a["x"], a["rows"], a["cols"], a["ld"], a["limit"], a["rec"], a["code"])
        assert rc == -1, (kw, rc)
        assert lib.lib.i2i_last_error().decode().startswith("scan:"), kw
        with pytest.raises(K.I2IError):
            lib.check(rc)
    rc = lib.lib.i2i_scan(None, code, None)
    assert rc == -1
    assert not read_rec(rec).any() and not big.cpu().numpy().any()                     # nothing was written by a refused call
    # an empty view is a launch that counts a run and nothing else
    assert call(lib, device, x, 0, 16, 16, 1.0, r, code) == 0
    assert read_rec(rec).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- the planned forward
POISON_CONV = "decoder.up_blocks.1.resnets.0.conv1"


def stage_names(w):
    """The labels health="stages" must produce for these weights' architectures, in program order."""
    nv, nu = len(w.vae_arch.block_out_channels), len(w.unet_arch.block_out_channels)
    return (["encoder.down_blocks.%d" % i for i in range(nv)] + ["moments", "latents"] + ["unet.down_blocks.%d" % i for i in range(nu)]
            + ["unet.mid_block"] + ["unet.up_blocks.%d" % i for i in range(nu)] + ["eps_prediction", "post_quant"]
            + ["decoder.up_blocks.%d" % i for i in range(nv)] + ["pre_clamp"])


def tiny_weights(poison=False):
    from img2img_turbo_amd import arch
    from img2img_turbo_amd.synth import make_pix2pix_weights
    w = make_pix2pix_weights(arch.TINY_UNET, arch.TINY_VAE, seed=1234)
    if poison:          # one bias element of one decoder convolution: 7e4 is beyond fp16 (65504) and well inside bf16
        key = [k for k in (POISON_CONV + ".base_layer.bias", POISON_CONV + ".bias") if k in w.vae][0]
        w.vae[key] = w.vae[key].clone()
        w.vae[key][1] = 7e4
    return w


def tiny_inputs(device, n=1, h=16, w=24):
    from img2img_turbo_amd import arch
    g = torch.Generator().manual_seed(23)
    x = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    cap = torch.randn(1, 77, arch.TINY_UNET.cross_attention_dim, generator=g)
    eps = torch.randn(n, 4, h // 8, w // 8, generator=g)
    return x.to(device), cap.to(device), eps.to(device)


def make_model(lib, device, dtype, health, weights=None, **plan_options):
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    return Pix2Pix_Turbo(weights=weights or tiny_weights(), device=device, dtype=dtype, lib=lib, health=health, plan_options=plan_options)


def ref_of_tap(plan, i, limit=None):
    """health_ref over the tensor record i of ``plan`` describes (the plan must keep its intermediates: debug=True)."""
    t, rows, cols, ld = plan.health_taps[i]
    bits, fmt = R.bits_of(t)
    lim = limit if limit is not None else plan.HEALTH_LIMIT[t.dtype]
    return R.scan_ref(bits[:(rows - 1) * ld + cols], cols, ld, lim, fmt, rows=rows)


def overwritten_later(plan, i):
    """True when an op behind scan i writes the scanned tensor again (the decoder's in-place `sample + skip_conv(skip)`): what a debug plan
    holds after the run is then not what the scan saw."""
    from img2img_turbo_amd import _capi as K
    t = plan.health_taps[i][0]
    at = [k for k, (o, _, _, l) in enumerate(plan.prog.ops) if o == K.OP_SCAN][i]
    return any(o == K.OP_IGEMM and p.c == t.data_ptr() for o, _, p, _ in plan.prog.ops[at + 1:])


def records(plan):
    sync(str(plan.device))
    return plan._health_i64.cpu().numpy().view(np.uint64)[:len(plan.health_labels)].copy()      # (.cpu() of a CPU tensor is the tensor itself)


def check_poison(lib, device, h=16, w=24):
    """7e4 in one bias element of POISON_CONV: in fp16 that convolution's output is the first non-finite tensor; in bf16 the same weights stay
    finite and the tap sees the value.  Expected counts come from health_ref over the intermediates of the (debug) plan itself."""
    x, cap, eps = tiny_inputs(device, 1, h, w)
    wts = tiny_weights(poison=True)
    for dtype in (torch.float16, torch.bfloat16):
        model = make_model(lib, device, dtype, "all", weights=wts, debug=True)
        model(x, caption_enc=cap.to(dtype), eps=eps)
        plan = model._last_plan
        rec = records(plan)
        checked = 0
        for i in range(len(plan.health_labels)):
            if not overwritten_later(plan, i):
                assert np.array_equal(rec[i], ref_of_tap(plan, i)), (str(dtype), plan.health_labels[i], rec[i].tolist())
                checked += 1
        assert checked >= len(plan.health_labels) - 2 * len(plan.va.block_out_channels)
        rep = model.health_report()
        at = plan.health_labels.index(POISON_CONV)
        bad = model.health_first_bad()
        if dtype == torch.float16:
            assert bad is not None and bad["label"] == POISON_CONV and bad["n_pos_inf"] >= 1, bad
            assert all(d["n_nan"] + d["n_pos_inf"] + d["n_neg_inf"] == 0 for d in rep[:at])
            assert any(d["n_nan"] for d in rep[at + 1:])                    # the Inf does not stay alone: the next GroupNorm makes NaNs of it
        else:
            assert bad is None, bad
            assert rep[at]["max_abs"] >= 6.9e4 and rep[at]["n_over"] == 0
        model.release_plans()

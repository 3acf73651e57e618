"""Cases and backend-independent checks shared by tests/test_scale_emu.py (CPU emulator) and tests/test_scale_gpu.py (MI355X): the LoRA
scale r as device state for every host -- the TwinConv fold kernel (i2i_twin_fold), the grouped merge (i2i_merge_group_*), the scale
program of a packer / a live_scale model, and plan files that carry it (magic "I2IPLAN2", i2i_plan_set_scale).  All of csrc/lora_merge.hip
and csrc/plan_file.hip; the contracts are in include/i2i_turbo.h."""
import ctypes as C
import functools
import os
import struct

import numpy as np
import pytest
import torch

F32, BF16, F16 = 0, 1, 2
TORCH = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
CANARY = {F32: 0x5AC3A55A, BF16: 0x5AC3, F16: 0x5AC3}
PAD = 8                    # canary elements around every destination (16 / 32 bytes: the destinations stay 16-byte aligned)
BAD_ARG, UNSUPPORTED = -1, -3

# (N, K, rank_pre, rank_cur): the real conv_in (320 rows of 3*3*8 padded channels, no adapter); a rank on one side only, one row block
# with a ragged row count / a single row; more than one 1024-element x-tile with a ragged second tile, 33 row blocks, both ranks
TWIN_SHAPES = [(320, 72, 0, 0), (5, 4, 0, 3), (1, 8, 2, 0), (130, 1028, 8, 12)]
TWIN_R = [0.0, 0.4, 1.0]


def sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def hip_stream(device):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None


def dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)


def canaries(n, dt, device):
    """n elements of the canary bit pattern as the integer tensor of dt's width."""
    return torch.full((n,), CANARY[dt], dtype=torch.int64).to(INT[dt]).to(device)


def ordinal(bits16):
    """int16 bit patterns of a 16-bit float type -> integers ordered as the values are (+-0 both 0)."""
    b = bits16.astype(np.int64) & 0xFFFF
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -mag, mag)


def from_ordinal(o, dt):
    """The fp64 values of the 16-bit floats with these ordinals."""
    bits = np.where(o < 0, (-o) | 0x8000, o).astype(np.uint16).view(np.int16)
    return torch.from_numpy(bits.copy()).view(TORCH[dt]).double().numpy()


def nearest_ordinal(ref, dt):
    """Ordinal of ref (fp64) rounded to nearest-even in the 16-bit type, computed exactly: torch's conversion goes through fp32 (a double
    rounding that can be one step off), so the three values around it are compared against ref in fp64, ties to the even pattern."""
    c = ordinal(torch.from_numpy(np.array(ref)).to(TORCH[dt]).view(torch.int16).numpy())
    cand = np.stack([c - 1, c, c + 1])
    dist = np.abs(from_ordinal(cand, dt) - ref[None])
    best, bd = cand[1], dist[1]
    for i in (0, 2):              # (a tie is between neighbours, exactly one of which has an even pattern)
        better = (dist[i] < bd) | ((dist[i] == bd) & (cand[i] % 2 == 0))
        best, bd = np.where(better, cand[i], best), np.where(better, dist[i], bd)
    return best


# ---------------------------------------------------------------------------------------------------------------- twin fold
# Operand sets.  "signed": every operand standard normal -- results cancel freely, down to elements five orders below their M.
# "aligned": what a TwinConv checkpoint holds (conv_in_curr starts as a copy of conv_in_pretrained and is fine-tuned from there) with
# magnitudes chosen so that NO element can cancel: |w_pre| in [0.5, 2] with a random sign, w_cur = w_pre * (0.75 .. 1.25), |a|, |b| <= 0.1,
# so sum |b||a| <= 0.08 / 0.12 (ranks 8 / 12) and, for r in [0, 1], |result| >= (1-r)(0.5 - 0.08 r) + r (0.375 - 0.12 r) >= 0.25, M <= 4.7.
KINDS = ("signed", "aligned")


@functools.lru_cache(maxsize=None)
def twin_operands(shape, kind="signed"):
    """fp32 operands of one shape (numpy, read-only) and the per-element magnitude M of the bound."""
    n, k, rp, rc = shape
    g = np.random.RandomState(1000 + n + 7 * k + 31 * rp + 101 * rc)
    if kind == "signed":
        f = lambda *s: g.standard_normal(s).astype(np.float32)
        ops = dict(w_pre=f(n, k), w_cur=f(n, k), a_pre=f(rp, k), b_pre=f(n, rp), a_cur=f(rc, k), b_cur=f(n, rc), bias_pre=f(n), bias_cur=f(n))
    else:
        u = lambda lo, hi, *s: g.uniform(lo, hi, s).astype(np.float32)
        w_pre = u(0.5, 2.0, n, k) * np.where(g.uniform(size=(n, k)) < 0.5, -1, 1).astype(np.float32)
        ops = dict(w_pre=w_pre, w_cur=(w_pre * u(0.75, 1.25, n, k)).astype(np.float32), a_pre=u(-0.1, 0.1, rp, k), b_pre=u(-0.1, 0.1, n, rp),
                   a_cur=u(-0.1, 0.1, rc, k), b_cur=u(-0.1, 0.1, n, rc), bias_pre=u(-1, 1, n), bias_cur=u(-1, 1, n))
    d = {k_: v.astype(np.float64) for k_, v in ops.items()}
    ops["M"] = np.abs(d["w_pre"]) + np.abs(d["w_cur"]) + np.abs(d["b_pre"]) @ np.abs(d["a_pre"]) + np.abs(d["b_cur"]) @ np.abs(d["a_cur"])
    for v in ops.values():
        v.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=None)
def twin_reference(shape, r, kind="signed"):
    """The formula of i2i_twin_fold_params in fp64, at the r the device holds (the fp32 value of r); 1 - r exact."""
    o = {k: v.astype(np.float64) for k, v in twin_operands(shape, kind).items()}
    r = float(np.float32(r))
    w = (1 - r) * (o["w_pre"] + r * (o["b_pre"] @ o["a_pre"])) + r * (o["w_cur"] + r * (o["b_cur"] @ o["a_cur"]))
    b = (1 - r) * o["bias_pre"] + r * o["bias_cur"]
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


def twin_call(lib, device, dt, p):
    rc = lib.lib.i2i_twin_fold(C.addressof(p), dt, hip_stream(device))
    sync(device)
    return rc


def twin_run(lib, device, shape, dt, r, with_bias=True, kind="signed"):
    """One fold into guarded buffers: returns (dst bits as an integer array [N][K], bias fp32 [N] or None) after the canary check."""
    from img2img_turbo_amd import _capi as K
    n, k, rp, rc = shape
    o = twin_operands(shape, kind)
    t = {name: dev(o[name], device) for name in ("w_pre", "w_cur", "a_pre", "b_pre", "a_cur", "b_cur", "bias_pre", "bias_cur")}
    buf = canaries(PAD + n * k + PAD, dt, device)
    bbuf = canaries(PAD + n + PAD, F32, device)
    rg = torch.tensor([r, 123.0], dtype=torch.float32, device=device)          # (the gamma slot is not the fold's business)
    p = K.TwinFoldParams()
    p.dst = buf.data_ptr() + PAD * buf.element_size()
    p.bias = bbuf.data_ptr() + PAD * 4 if with_bias else 0
    p.w_pre, p.w_cur, p.bias_pre, p.bias_cur = t["w_pre"].data_ptr(), t["w_cur"].data_ptr(), t["bias_pre"].data_ptr(), t["bias_cur"].data_ptr()
    if rp:
        p.a_pre, p.b_pre = t["a_pre"].data_ptr(), t["b_pre"].data_ptr()
    if rc:
        p.a_cur, p.b_cur = t["a_cur"].data_ptr(), t["b_cur"].data_ptr()
    p.N, p.K, p.rank_pre, p.rank_cur, p.rg = n, k, rp, rc, rg.data_ptr()
    assert twin_call(lib, device, dt, p) == 0, lib.lib.i2i_last_error().decode()
    host, bhost = buf.cpu().numpy(), bbuf.cpu().numpy()
    can = np.array(CANARY[dt]).astype(host.dtype)
    assert (host[:PAD] == can).all() and (host[PAD + n * k:] == can).all(), ("dst canary", shape, dt, r)
    assert (bhost[:PAD] == CANARY[F32]).all() and (bhost[PAD + n:] == CANARY[F32]).all(), ("bias canary", shape, dt, r)
    if not with_bias:
        assert (bhost == CANARY[F32]).all(), ("bias written without a bias pointer", shape, dt, r)
    return host[PAD:PAD + n * k].reshape(n, k), (bhost[PAD:PAD + n].view(np.float32) if with_bias else None)


def check_twin(lib, device, shape, dt):
    """Every r of one (shape, dtype) against the fp64 formula, with and without the bias, on both operand sets.

    fp32: each element within (rank_pre + rank_cur + 4) * 2^-24 * M (every step of the documented arithmetic is one rounding of relative
    size 2^-24 on a quantity no larger than M).
    16-bit, "aligned" operands: each element is the fp64 value rounded to T or one of its two neighbours.  That statement presupposes that
    the fp32 error is below T's spacing at the result, which the aligned set guarantees for every element (|result| >= 0.25: spacing >=
    2^-12 in fp16, the fp32 bound <= 24 * 2^-24 * 4.7 = 6.7e-6).  It cannot hold where a result cancels far below its M: on the "signed"
    set at (130, 1028, 8, 12), fp16, r = 1, one element of 133640 has the exact value 3.579e-05 (fp16 spacing there 6e-08) with
    M = 14.1; the kernel's fp32 value is off by 0.17 * 2^-24 * M -- deep inside the fp32 bound -- and lands two fp16 steps away.
    16-bit, "signed" operands, therefore take the bound that IS derivable there: the fp32 bound plus half of T's spacing at the stored
    value (the one further rounding)."""
    n, k, rp, rc = shape
    worst = 0.0
    for kind in KINDS:
        o = twin_operands(shape, kind)
        for r in TWIN_R:
            want, want_b = twin_reference(shape, r, kind)
            bits, bias = twin_run(lib, device, shape, dt, r, kind=kind)
            bound = (rp + rc + 4) * 2.0 ** -24 * o["M"]
            if dt == F32:
                err = np.abs(bits.view(np.float32).astype(np.float64) - want)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (shape, kind, r, float((err / bound).max()))
            elif kind == "aligned":
                assert np.abs(want).min() >= 0.25 and o["M"].max() <= 4.7          # the premise above
                step = np.abs(ordinal(bits) - nearest_ordinal(want, dt))
                worst = max(worst, float(step.max()))
                assert (step <= 1).all(), (shape, dt, r, int(step.max()), int((step > 1).sum()))
            else:
                od = ordinal(bits)
                v = from_ordinal(od, dt)
                half = 0.5 * np.maximum(np.abs(from_ordinal(od + 1, dt) - v), np.abs(v - from_ordinal(od - 1, dt)))
                err = np.abs(v - want)
                assert (err <= bound + half).all(), (shape, dt, kind, r, float((err / (bound + half)).max()))
            # fma(1 - r, bias_pre, r * bias_cur): three roundings (1 - r, the product, the fma) on at most |bias_pre| + |bias_cur|
            bb = 3 * 2.0 ** -24 * (np.abs(o["bias_pre"]).astype(np.float64) + np.abs(o["bias_cur"]))
            assert (np.abs(bias.astype(np.float64) - want_b) <= bb).all(), (shape, dt, kind, r)
            exact = None
            if r == 0.0 and rp == 0:
                exact, exact_b = o["w_pre"], o["bias_pre"]
            if r == 1.0 and rc == 0:
                exact, exact_b = o["w_cur"], o["bias_cur"]
            if exact is not None:
                cvt = torch.from_numpy(exact.copy()).to(TORCH[dt]).view(INT[dt]).numpy()
                assert np.array_equal(bits, cvt), (shape, dt, kind, r, "not cvt(W) bit for bit")
                assert np.array_equal(bias, exact_b), (shape, dt, kind, r)
            if kind == "signed":
                bits2, none = twin_run(lib, device, shape, dt, r, with_bias=False, kind=kind)
                assert none is None and np.array_equal(bits2, bits), (shape, dt, r)
    return worst


def check_twin_abi(lib, device):
    from img2img_turbo_amd import _capi as K
    w = torch.ones(4, 8, dtype=torch.float32, device=device)
    a = torch.ones(2, 8, dtype=torch.float32, device=device)
    b = torch.ones(4, 2, dtype=torch.float32, device=device)
    bias = torch.zeros(4, dtype=torch.float32, device=device)
    buf = canaries(PAD + 32 + PAD, F32, device)

    def params(**kw):
        p = K.TwinFoldParams()
        p.dst, p.w_pre, p.w_cur, p.N, p.K = buf.data_ptr() + 4 * PAD, w.data_ptr(), w.data_ptr(), 4, 8
        for k_, v in kw.items():
            setattr(p, k_, v)
        return p
    bad = [params(dst=0), params(w_pre=0), params(w_cur=0), params(K=6), params(K=0), params(N=0), params(rank_pre=-1),
           params(rank_pre=2), params(rank_pre=2, a_pre=a.data_ptr()), params(rank_cur=2, b_cur=b.data_ptr()),
           params(bias=bias.data_ptr()), params(bias=bias.data_ptr(), bias_pre=bias.data_ptr())]
    for i, p in enumerate(bad):
        assert twin_call(lib, device, F32, p) == BAD_ARG, i
        assert lib.lib.i2i_last_error().decode().startswith("twin_fold:"), i
        with pytest.raises(K.I2IError):
            lib.check(BAD_ARG)
    assert twin_call(lib, device, 7, params()) == BAD_ARG and "dtype" in lib.lib.i2i_last_error().decode()
    assert (buf.cpu().numpy() == CANARY[F32]).all()            # nothing ran
    assert lib.lib.i2i_twin_fold(None, F32, None) == BAD_ARG
    # the op form through i2i_run (capi.hip's dispatch) equals the direct entry
    from img2img_turbo_amd import ops as O
    shape = (5, 4, 0, 3)
    o = twin_operands(shape)
    t = {k_: dev(o[k_], device) for k_ in ("w_pre", "w_cur", "a_cur", "b_cur", "bias_pre", "bias_cur")}
    rg = torch.tensor([0.4, 0.4], dtype=torch.float32, device=device)
    dst = torch.zeros(5, 4, dtype=torch.bfloat16, device=device)
    bo = torch.zeros(5, dtype=torch.float32, device=device)
    opcode, p = O.twin_fold(dst, bo, (t["w_pre"], None, None), (t["w_cur"], t["a_cur"], t["b_cur"]), rg, bias_pre=t["bias_pre"], bias_cur=t["bias_cur"])
    assert opcode == K.OP_TWIN_FOLD and p.rank_pre == 0 and p.rank_cur == 3
    prog = K.Program()
    prog.add(opcode, BF16, p, "twin")
    prog.freeze()
    lib.run(prog, torch.cuda.current_stream().cuda_stream if device != "cpu" else 0)
    sync(device)
    bits, bias_direct = twin_run(lib, device, shape, BF16, 0.4)
    assert np.array_equal(dst.cpu().view(torch.int16).numpy(), bits) and np.array_equal(bo.cpu().numpy(), bias_direct)


# ---------------------------------------------------------------------------------------------------------------- grouped merge
# (N, K, rank, use_gamma, destination, row0): N in {1, 4, 5, 130}, K in {4, 72, 1028}, rank in {0, 1, 8, 12}; layers 1 and 4 are the row
# slices 1..4 and 5..9 of ONE [10][72] tensor "S" whose row 0 nobody writes; layer 3 spans two x-tiles and 33 row blocks
GROUP_LAYERS = [(1, 4, 0, 1, "d0", 0), (4, 72, 1, 0, "S", 1), (5, 4, 12, 1, "d2", 0), (130, 1028, 8, 0, "d3", 0), (5, 72, 12, 1, "S", 5), (1, 1028, 0, 0, "d5", 0)]
GROUP_DST = {"d0": 1 * 4, "S": 10 * 72, "d2": 5 * 4, "d3": 130 * 1028, "d5": 1 * 1028}
GROUP_RG = [(0.4, 0.4), (1.0, 0.7)]


@functools.lru_cache(maxsize=None)
def group_operands():
    g = np.random.RandomState(77)
    out = []
    for n, k, rank, _g, _d, _r in GROUP_LAYERS:
        out.append(tuple(g.standard_normal(s).astype(np.float32) for s in ((n, k), (rank, k), (n, rank))))
    return out


class GroupSetup:
    """The six layers on `device` with ONE arena of destinations (canaries between and around them) per consumer: `arena` for the grouped
    launch, `arena_ref` for six i2i_lora_merge calls with the same operands."""

    def __init__(self, device, dt):
        from img2img_turbo_amd import _capi as K
        self.device, self.dt = device, dt
        self.rg = torch.tensor(GROUP_RG[0], dtype=torch.float32, device=device)
        self.offsets, n = {}, PAD
        for name, elems in GROUP_DST.items():
            self.offsets[name] = n
            n += (elems + PAD + 7) // 8 * 8              # the next destination starts 16-byte aligned, at least PAD canaries later
        self.size = n
        self.arena, self.arena_ref = canaries(n, dt, device), canaries(n, dt, device)
        self.keep, self.layers, self.layers_ref = [], [], []
        for (nrow, k, rank, use_gamma, dname, row0), (w0, a, b) in zip(GROUP_LAYERS, group_operands()):
            w0d, ad, bd = dev(w0, device), dev(a, device), dev(b, device)
            self.keep += [w0d, ad, bd]
            for arena, layers in ((self.arena, self.layers), (self.arena_ref, self.layers_ref)):
                p = K.LoraMergeParams()
                p.dst = arena.data_ptr() + (self.offsets[dname] + row0 * k) * arena.element_size()
                p.w0, p.N, p.K, p.rank, p.use_gamma, p.rg = w0d.data_ptr(), nrow, k, rank, use_gamma, self.rg.data_ptr()
                if rank:
                    p.a, p.b = ad.data_ptr(), bd.data_ptr()
                layers.append(p)

    def written_mask(self):
        m = np.zeros(self.size, dtype=bool)
        for nrow, k, _r, _g, dname, row0 in GROUP_LAYERS:
            s = self.offsets[dname] + row0 * k
            m[s:s + nrow * k] = True
        return m

    def run_reference(self, lib):
        for p in self.layers_ref:
            assert lib.lib.i2i_lora_merge(C.addressof(p), self.dt, hip_stream(self.device)) == 0, lib.lib.i2i_last_error().decode()
        sync(self.device)
        return self.arena_ref.cpu().numpy()

    def compare(self, lib, what):
        sync(self.device)
        got, want = self.arena.cpu().numpy(), self.run_reference(lib)
        m = self.written_mask()
        can = np.array(CANARY[self.dt]).astype(got.dtype)
        assert (got[~m] == can).all(), (what, "canary", int((got[~m] != can).sum()))
        assert (want[m] != can).any()                          # the reference really wrote
        assert np.array_equal(got, want), (what, int((got != want).sum()))
        return got.copy()

    def set_rg(self, rg):
        self.rg.copy_(torch.tensor(rg, dtype=torch.float32))
        sync(self.device)

    def wipe(self):
        self.arena.copy_(canaries(self.size, self.dt, self.device))
        self.arena_ref.copy_(canaries(self.size, self.dt, self.device))


def check_group(lib, device, dt):
    """One launch over six layers = six i2i_lora_merge calls, bit for bit, at both (r, gamma); the second run sees the rewritten rg."""
    s = GroupSetup(device, dt)
    g = lib.merge_group_create(s.layers, dt)
    try:
        lib.merge_group_run(g, hip_stream(device).value if device != "cpu" else 0)
        first = s.compare(lib, "first run")
        s.set_rg(GROUP_RG[1])
        lib.merge_group_run(g, hip_stream(device).value if device != "cpu" else 0)
        second = s.compare(lib, "after rewriting rg")
        assert not np.array_equal(first, second)
    finally:
        lib.merge_group_destroy(g)
    return s


def check_group_abi(lib, device):
    from img2img_turbo_amd import _capi as K
    s = GroupSetup(device, BF16)
    ks = torch.ones(1028, dtype=torch.float32, device=device)
    cs = torch.zeros(130, dtype=torch.float32, device=device)

    def attempt(layers, n=None, dt=BF16):
        arr = (K.LoraMergeParams * max(len(layers), 1))(*layers)
        g = C.c_void_p(0xDEAD)
        rc = lib.lib.i2i_merge_group_create(C.addressof(arr) if layers else None, len(layers) if n is None else n, dt, C.byref(g))
        assert g.value is None or rc == 0, "a failed create must clear the handle"
        return rc, lib.lib.i2i_last_error().decode()

    def copy_of(i, **kw):
        p = K.LoraMergeParams.from_buffer_copy(s.layers[i])
        for k_, v in kw.items():
            setattr(p, k_, v)
        return p
    cases = [(2, copy_of(2, K=6)), (0, copy_of(0, dst=0)), (3, copy_of(3, a=0)), (5, copy_of(5, N=0)), (4, copy_of(4, rank=-1)),
             (3, copy_of(3, kscale=ks.data_ptr(), kshift=ks.data_ptr(), colsum=cs.data_ptr(), bias_out=cs.data_ptr())),      # the LayerNorm-fold form stays per layer
             (1, copy_of(1, kscale=ks.data_ptr()))]
    for idx, bad in cases:
        layers = list(s.layers)
        layers[idx] = bad
        rc, msg = attempt(layers)
        assert rc == BAD_ARG and ("layer %d:" % idx) in msg, (idx, rc, msg)
    assert attempt([], 0)[0] == BAD_ARG and attempt(s.layers, dt=9)[0] == BAD_ARG
    assert lib.lib.i2i_merge_group_create(None, 3, BF16, None) == BAD_ARG
    assert lib.lib.i2i_merge_group_run(None, None) == BAD_ARG and lib.lib.i2i_merge_group_destroy(None) == 0
    sync(device)
    assert (s.arena.cpu().numpy() == np.array(CANARY[BF16]).astype(np.int16)).all()


# ---------------------------------------------------------------------------------------------------------------- models
def make_model(lib, device, sketch, dtype=torch.float32, live_scale=True, seed=2):
    from oracle import TINY_UNET, TINY_VAE
    from oracle.synth import make_pix2pix_weights
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.weights import GeneratorWeights
    mw = make_pix2pix_weights(TINY_UNET, TINY_VAE, seed=seed, sketch=sketch)
    gw = GeneratorWeights(mw.unet, mw.vae, mw.unet_arch, mw.vae_arch, mw.unet_scaling, mw.vae_scaling, mw.vae_b2a)
    return mw, Pix2Pix_Turbo(weights=gw, device=device, dtype=dtype, lib=lib, live_scale=live_scale)


def model_inputs(device, h, w):
    from oracle import TINY_UNET
    from oracle.synth import make_inputs
    return make_inputs("sketch", 1, h, w, TINY_UNET.cross_attention_dim)


def check_live_equals_per_layer(lib, device, h, w):
    """A checkpoint without TwinConv: the scale program (grouped launch + the LayerNorm-fold layers) writes the bits the per-layer loop
    writes, so the stochastic forward is bit-identical with the flag on and off along r = 0.4 -> 0.8 -> 0.4, and r returns to its bits."""
    x, cap, eps, nm = model_inputs(device, h, w)
    outs = {}
    for live in (False, True):
        _, model = make_model(lib, device, sketch=False, live_scale=live)
        outs[live] = [model(x.to(device), caption_enc=cap.to(device), eps=eps.to(device), deterministic=False, r=r, noise_map=nm.to(device)).cpu()
                      for r in (0.4, 0.8, 0.4)]
        if live:
            for pk in model._packers.values():
                sp = pk.scale_program()
                assert pk.live_scale and sp.n_grouped > 0 and len(sp.groups) == 1 and sp.n_grouped + sp.prog.n == sp.n_layers and not pk._refolds
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(outs[True][0], outs[True][2]) and not torch.equal(outs[True][0], outs[True][1])


def export_live(model, plan, path):
    from img2img_turbo_amd.plan_file import export_plan
    return export_plan(plan, path, live_scale=True)


def feed(lib, h, plan, x, cap, eps, nm):
    lib.plan_write(h, "x", x.to(plan.x_in.dtype).contiguous())
    lib.plan_write(h, "ctx", cap.to(plan.ctx.dtype).reshape(plan.ctx.shape).contiguous())
    lib.plan_write(h, "eps", eps.to(plan.eps.dtype).contiguous())
    lib.plan_write(h, "noise", nm.to(plan.noise.dtype).expand_as(plan.noise).contiguous())


def check_plan_round_trip(lib, device, tmp_path, h, w):
    """A TwinConv model with live_scale: the file exported at r = 1 and moved to r = 0.4 with i2i_plan_set_scale computes the Python
    model's r = 0.4 bits, and set back to 1 the bits of the export scale.  Returns what the other plan-file checks reuse."""
    x, cap, eps, nm = model_inputs(device, h, w)
    _, model = make_model(lib, device, sketch=True, live_scale=True)
    kw = dict(caption_enc=cap.to(device), eps=eps.to(device), deterministic=False, noise_map=nm.to(device))
    out04 = model(x.to(device), r=0.4, **kw).cpu()
    out1 = model(x.to(device), r=1.0, **kw).cpu()
    assert not torch.equal(out04, out1)
    plan = list(model._plans.values())[0]
    assert plan.r == 1.0
    path = str(tmp_path / "live.i2iplan")
    info = export_live(model, plan, path)
    n_merges = sum(len(pk._merges) for pk in (plan.pu, plan.pv))
    assert info["ops"] == plan.prog.n and info["scale_ops"] == n_merges + 1          # every adapted layer + the TwinConv fold
    with open(path, "rb") as f:
        assert f.read(8) == b"I2IPLAN2"
    hnd = lib.plan_load(path)
    try:
        assert lib.plan_has_scale(hnd)
        ops, n = C.c_void_p(), C.c_int()
        lib.check(lib.lib.i2i_plan_ops(hnd, C.byref(ops), C.byref(n)))
        assert n.value == plan.prog.n                                                # the forward only
        feed(lib, hnd, plan, x, cap, eps, nm)
        st = hip_stream(device).value if device != "cpu" else 0
        lib.plan_set_scale(hnd, 0.4, 0.4, st)
        lib.plan_run(hnd, st)
        got = lib.plan_read(hnd, "out", torch.empty_like(plan.out, device="cpu"))
        assert torch.equal(got.float(), out04.float()), float((got.float() - out04.float()).abs().max())
        lib.plan_set_scale(hnd, 1.0, 1.0, st)
        lib.plan_run(hnd, st)
        got = lib.plan_read(hnd, "out", torch.empty_like(plan.out, device="cpu"))
        assert torch.equal(got.float(), out1.float()), float((got.float() - out1.float()).abs().max())
    finally:
        lib.plan_destroy(hnd)
    return dict(model=model, plan=plan, path=path, x=x, cap=cap, eps=eps, nm=nm, out04=out04, out1=out1)


def header_fields(blob):
    """(n_ops, n_bufs, n_relocs, n_io, n_scale, offset of the relocation table) of a v2 file."""
    _abi, _sz, n_ops, n_bufs, n_relocs, n_io = struct.unpack_from("<6I", blob, 8)
    n_scale = struct.unpack_from("<I", blob, 32)[0]
    return n_ops, n_bufs, n_relocs, n_io, n_scale, 40 + 16 * n_bufs + 48 * n_io

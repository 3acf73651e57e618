"""Cases and backend-independent checks shared by tests/test_randn_emu.py (CPU emulator) and tests/test_randn_gpu.py (MI355X): the seeded
noise op (i2i_randn, csrc/elementwise.hip) against tests/randn_ref.py, the oracle of the contract in include/i2i_turbo.h.  The kernel
runs one thread per Philox counter (4 elements) on at most 1024 workgroups of 256: 2^20 elements per pass of its grid-stride loop."""
import ctypes as C
import functools

import numpy as np
import torch

import randn_ref

# 1, 3: a tail only; 4, 5: one counter and one element more; 255 .. 257: around 64 counters, with and without a ragged last
# counter; 396 = 4 * 9 * 11, the tiny model's latent at 72 x 88; 16385: many workgroups + a one-element tail; 2^20 + 3: one counter more
# than a whole grid pass, so the stride loop runs
SIZES = [1, 3, 4, 5, 255, 256, 257, 396, 16385]
BIG = (1 << 20) + 3
SEEDS = [0, 42, (1 << 40) + 7]                 # the last one exercises the high key word
STEPS = [0, 1, 0xFFFFFFFF]
STREAMS = [0, 2]
COMBOS = [(s, t, m) for s in SEEDS for t in STEPS for m in STREAMS]
NORMAL_COMBOS = [(42, 0, 0), (0, 1, 2), ((1 << 40) + 7, 0xFFFFFFFF, 2)]
OFFSETS = [0, 1]                               # elements past a 16-byte boundary: 1 = no 128-bit store is possible
PAD = 8                                        # canary elements on either side (a multiple of 4: the alignment is the offset's alone)
CANARY = 0x5AC3A55A
NORMAL, RAW, ADVANCE = 0, 1, 2

# |got - want| <= rad * TOL per element (include/i2i_turbo.h): logf within 1 ulp, halved by the square root (2^-24 relative); the correctly
# rounded sqrtf (2^-24); the pi-scaled sine / cosine within 4 * 2^-24 absolute; the final product (2^-24): 7 * 2^-24 < 2^-21.
TOL = 2.0 ** -21
ABS_MAX = 5.77                                 # sqrt(48 ln 2)


@functools.lru_cache(maxsize=None)
def want_raw(n, seed, step, stream):
    out = randn_ref.raw(n, seed, step, stream)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_normal(n, seed, step, stream):
    val, rad = randn_ref.normal(n, seed, step, stream)
    val.setflags(write=False)
    rad.setflags(write=False)
    return val, rad


# ---------------------------------------------------------------------------------------------------------------- device plumbing
def sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def state_tensor(words, device):
    """Four uint32 as the int32 device tensor the op reads."""
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32).copy()).to(device)


def read_state(state):
    return state.cpu().numpy().view(np.uint32).tolist()


def call(lib, device, dst_ptr, n, *, kind=RAW, seed=0, step=0, stream=0, state=None):
    """i2i_randn through the raw C entry; returns the status."""
    from img2img_turbo_amd import _capi as K
    p = K.RandnParams()
    p.dst, p.n, p.state = dst_ptr, n, (state.data_ptr() if state is not None else 0)
    p.seed, p.step, p.stream_id, p.kind = seed, step, stream, kind
    hip_stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None
    rc = lib.lib.i2i_randn(C.addressof(p), 0, hip_stream)
    sync(device)
    return rc


def guarded(n, offset, device):
    """An int32 buffer of canaries with room for n elements `offset` elements past a 16-byte boundary; returns (buffer, first index)."""
    buf = torch.from_numpy(np.full(PAD + offset + n + PAD + 4, CANARY, dtype=np.uint32).view(np.int32).copy()).to(device)
    assert buf.data_ptr() % 16 == 0
    return buf, PAD + offset


def fill_guarded(lib, device, n, offset, **kw):
    """One fill into a guarded buffer: returns the n words as uint32 after checking that nothing around them was written."""
    buf, first = guarded(n, offset, device)
    rc = call(lib, device, buf.data_ptr() + 4 * first, n, **kw)
    assert rc == 0, (rc, lib.lib.i2i_last_error().decode())
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:first] == CANARY).all() and (host[first + n:] == CANARY).all(), ("canary", n, offset, kw)
    return host[first:first + n]


# ---------------------------------------------------------------------------------------------------------------- shared checks
def check_raw(lib, device, n, combos=COMBOS, offsets=OFFSETS):
    for offset in offsets:
        for seed, step, stream in combos:
            got = fill_guarded(lib, device, n, offset, kind=RAW, seed=seed, step=step, stream=stream)
            want = want_raw(n, seed, step, stream)
            assert np.array_equal(got, want), (n, offset, seed, step, stream, int((got != want).sum()))


def check_state_form(lib, device):
    """The device-state form equals the immediate form; the reserved word is ignored, whatever it holds."""
    for n, offset in ((257, 1), (396, 0)):
        for seed, step, stream in COMBOS:
            want = want_raw(n, seed, step, stream)
            for reserved in (0, 0xDEADBEEF):
                words = [seed & 0xFFFFFFFF, seed >> 32, step, reserved]
                st = state_tensor(words, device)
                # (the immediates are garbage: the state overrides them)
                got = fill_guarded(lib, device, n, offset, kind=RAW, seed=0x1234567890, step=77, stream=stream, state=st)
                assert np.array_equal(got, want), (n, seed, step, stream, reserved)
                assert read_state(st) == words                 # a fill leaves the state alone


def normal_errors(lib, device, n, combos=NORMAL_COMBOS, offsets=OFFSETS):
    """max |err| / rad over the cases, after asserting the bound per element."""
    worst = 0.0
    for offset in offsets:
        for seed, step, stream in combos:
            bits = fill_guarded(lib, device, n, offset, kind=NORMAL, seed=seed, step=step, stream=stream)
            got = bits.view(np.float32).astype(np.float64)
            want, rad = want_normal(n, seed, step, stream)
            assert np.isfinite(got).all() and np.abs(got).max() <= ABS_MAX
            err = np.abs(got - want)
            zero = rad == 0
            assert (got[zero] == 0).all()
            rel = err[~zero] / rad[~zero]
            worst = max(worst, float(rel.max()) if rel.size else 0.0)
            assert (err <= rad * TOL).all(), (n, offset, seed, step, stream, float(rel.max()) / TOL)
    return worst


def corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def check_statistics(lib, device):
    """Seed 42, n = 16384: the gates of the op's OUTPUT (the oracle's own values: 0.26, 0.019, 0.64, 0.0009, 0.011, 0.012)."""
    from scipy import stats
    from img2img_turbo_amd import rng
    n = 16384

    def draw(step, stream):
        x = rng.randn((n,), 42, step, stream, device=device, lib=lib)
        sync(device)
        return x.cpu().numpy().astype(np.float64)
    x, x_step1, x_stream1 = draw(0, 0), draw(1, 0), draw(0, 1)
    figures = {"mean*sqrt(n)": abs(x.mean()) * np.sqrt(n), "var-1": abs(x.var() - 1.0), "ks_p": float(stats.kstest(x, "norm").pvalue),
               "rho_step": abs(corr(x, x_step1)), "rho_stream": abs(corr(x, x_stream1)), "rho_lag1": abs(corr(x[:-1], x[1:])),
               "max_abs": float(np.abs(x).max())}
    print("[randn] statistics, seed 42, n = 16384: " + ", ".join("%s %.4g" % kv for kv in figures.items()))
    assert np.isfinite(x).all() and figures["max_abs"] <= ABS_MAX
    assert figures["mean*sqrt(n)"] < 4
    assert figures["var-1"] < 0.05
    assert figures["ks_p"] > 1e-3
    assert figures["rho_step"] < 0.04 and figures["rho_stream"] < 0.04 and figures["rho_lag1"] < 0.04


def check_advance(lib, device):
    """Advance takes the step from 5 to 6 and from 0xffffffff to 0 and touches nothing else; the program-op form equals the direct entry."""
    from img2img_turbo_amd import _capi as K, ops as O
    for step, after in ((5, 6), (0xFFFFFFFF, 0)):
        words = [0x89ABCDEF, 0x01234567, step, 0xDEADBEEF]
        buf = state_tensor([CANARY] * 4 + words + [CANARY] * 4, device)
        st = buf[4:8]
        assert call(lib, device, 0, 0, kind=ADVANCE, state=st) == 0
        assert read_state(buf) == [CANARY] * 4 + words[:2] + [after, words[3]] + [CANARY] * 4
    # one program: normal fill, raw fill, advance, raw fill -- through i2i_run (capi.hip's dispatch), as a plan records them
    seed, n = (1 << 40) + 7, 396
    st = state_tensor([seed & 0xFFFFFFFF, seed >> 32, 0xFFFFFFFF, 3], device)
    a = torch.zeros(n, dtype=torch.float32, device=device)
    b = torch.zeros(n, dtype=torch.int32, device=device)
    c = torch.zeros(n, dtype=torch.int32, device=device)
    prog = K.Program()
    prog.add(*_op(O.randn(a, state=st, stream_id=0)), "normal")
    prog.add(*_op(O.randn(b, state=st, stream_id=2, kind=K.RANDN_RAW)), "raw")
    prog.add(*_op(O.randn(None, state=st, kind=K.RANDN_ADVANCE)), "advance")
    prog.add(*_op(O.randn(c, state=st, stream_id=2, kind=K.RANDN_RAW)), "raw after")
    prog.freeze()
    lib.run(prog, torch.cuda.current_stream().cuda_stream if device != "cpu" else 0)
    sync(device)
    direct = fill_guarded(lib, device, n, 0, kind=NORMAL, seed=seed, step=0xFFFFFFFF, stream=0)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), direct)
    assert np.array_equal(b.cpu().numpy().view(np.uint32), want_raw(n, seed, 0xFFFFFFFF, 2))
    assert np.array_equal(c.cpu().numpy().view(np.uint32), want_raw(n, seed, 0, 2))            # the step wrapped to 0 in between
    assert read_state(st) == [seed & 0xFFFFFFFF, seed >> 32, 0, 3]


def _op(built):
    from img2img_turbo_amd import _capi as K
    return built[0], K.F32, built[1]


def check_abi(lib, device):
    import pytest
    from img2img_turbo_amd import _capi as K
    buf, first = guarded(16, 0, device)
    dst = buf.data_ptr() + 4 * first
    st = state_tensor([1, 2, 3, 4], device)
    bad = [dict(dst_ptr=0, n=16),                       # NULL dst with n > 0
           dict(dst_ptr=dst, n=-1),                     # n < 0
           dict(dst_ptr=dst, n=16, kind=3), dict(dst_ptr=dst, n=16, kind=-1),       # unknown kind
           dict(dst_ptr=dst, n=16, kind=ADVANCE),       # advance without state
           dict(dst_ptr=dst + 2, n=8)]                  # not 4-byte aligned
    for kw in bad:
        rc = call(lib, device, kw.pop("dst_ptr"), kw.pop("n"), **kw)
        assert rc == -1, (kw, rc)                              # I2I_ERR_BAD_ARG
        assert lib.lib.i2i_last_error().decode().startswith("randn:"), kw
        assert (buf.cpu().numpy().view(np.uint32) == CANARY).all(), kw            # dst untouched
        with pytest.raises(K.I2IError):
            lib.check(rc)
    # n = 0 is a no-op, with or without a destination
    assert call(lib, device, 0, 0, kind=NORMAL) == 0 and call(lib, device, dst, 0, kind=RAW, state=st) == 0
    assert (buf.cpu().numpy().view(np.uint32) == CANARY).all() and read_state(st) == [1, 2, 3, 4]


def check_module(lib, device):
    """img2img_turbo_amd.rng: the eager forms and the state packing."""
    from img2img_turbo_amd import rng
    assert rng.pack_state(42) == [42, 0, 0, 0] and rng.pack_state((1 << 40) + 7, 5) == [7, 1 << 8, 5, 0]
    assert rng.pack_state(-1, -1) == [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0]                    # reduced mod 2^64 / 2^32
    assert rng.pack_state((1 << 64) + 3, 1 << 32) == [3, 0, 0, 0]
    w = rng.raw_u32(396, (1 << 40) + 7, 1, 2, device=device, lib=lib)
    assert w.dtype == torch.int32 and np.array_equal(w.cpu().numpy().view(np.uint32), want_raw(396, (1 << 40) + 7, 1, 2))
    assert np.array_equal(rng.raw_u32(5, -1, device=device, lib=lib).cpu().numpy().view(np.uint32), want_raw(5, (1 << 64) - 1, 0, 0))
    x = rng.randn((2, 4, 9, 11), 7, 0, stream=2, device=device, lib=lib)
    assert x.shape == (2, 4, 9, 11) and x.dtype == torch.float32
    direct = fill_guarded(lib, device, 792, 0, kind=NORMAL, seed=7, step=0, stream=2)
    assert np.array_equal(x.cpu().numpy().reshape(-1).view(np.uint32), direct)
    # image 0 of a batch is the batch-1 draw (flat index)
    assert torch.equal(x[0], rng.randn((4, 9, 11), 7, 0, stream=2, device=device, lib=lib))
    # into a slice of an existing tensor
    big = torch.zeros(3, 396, device=device)
    rng.randn(None, 7, 0, stream=2, lib=lib, out=big[1])
    sync(device)
    assert torch.equal(big[1], x[0].reshape(-1)) and not big[0].any() and not big[2].any()


# ---------------------------------------------------------------------------------------------------------------- the pipeline
H, W = 72, 88


def make_model(lib, device, stochastic):
    from img2img_turbo_amd import arch
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.synth import make_pix2pix_weights
    w = make_pix2pix_weights(arch.TINY_UNET, arch.TINY_VAE, seed=1234, sketch=stochastic)
    return Pix2Pix_Turbo(weights=w, device=device, dtype=torch.float32, lib=lib)


def pipeline_inputs(n, device, h=H, w=W):
    from oracle import TINY_UNET
    g = torch.Generator().manual_seed(23)
    x = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    cap = torch.randn(1, 77, TINY_UNET.cross_attention_dim, generator=g)
    return x.to(device), cap.to(device)


def check_pipeline(lib, device, stochastic, h=H, w=W):
    """forward(seed=7) is forward() of the eager draws at (7, step 0), streams 0 and 2, bit for bit; the same seed twice gives the same
    image and seed 8 another; image 0 of the batch draws what a batch-1 run draws; seed= excludes eps= / noise_map=; without seed= the
    forward runs a plan that has no noise op.  (72 x 88 on the GPU; the emulator, which needs a second per thousand
    pixels of a forward, runs 24 x 40: a latent of 3 x 5, 60 elements per image -- whole counters and, over the batch, slices that start at
    every alignment the flat index produces.)"""
    import pytest
    from img2img_turbo_amd import rng
    model = make_model(lib, device, stochastic)
    x, cap = pipeline_inputs(2, device, h, w)
    kw = dict(caption_enc=cap, deterministic=not stochastic, r=0.4 if stochastic else 1.0)
    lat = (2, 4, h // 8, w // 8)
    out7 = model.forward(x, seed=7, **kw)
    assert len(model._plans) == 1
    plan = list(model._plans.values())[0]
    assert plan.rng and plan.rng_state.shape == (4,) and plan.rng_state.element_size() == 4
    assert read_state(plan.rng_state) == [7, 0, 1, 0]                      # one run: the step moved on
    eps = rng.randn(lat, 7, 0, stream=0, device=device, lib=lib)
    noise = rng.randn(lat, 7, 0, stream=2, device=device, lib=lib)
    assert torch.equal(plan.eps, eps) and (not stochastic or torch.equal(plan.noise, noise))
    assert (plan.noise is not None) == stochastic
    labels = plan.prog.labels
    assert labels[0] == "rng.eps" and labels[-1] == "rng.advance" and ("rng.noise" in labels) == stochastic
    eps2 = plan.eps.clone()
    # the explicit twin: seed=None, on a plan of its own without the op
    out_explicit = model.forward(x, eps=eps, noise_map=noise if stochastic else None, **kw)
    assert len(model._plans) == 2
    plain = [p for p in model._plans.values() if not p.rng]
    assert len(plain) == 1 and plain[0].rng_state is None and "rng.eps" not in plain[0].prog.labels
    assert torch.equal(out7, out_explicit)
    assert torch.equal(model.forward(x, seed=7, **kw), out7)
    out8 = model.forward(x, seed=8, **kw)
    assert out8.shape == out7.shape and not torch.equal(out8, out7)
    assert len(model._plans) == 2                                          # every seed on the one plan
    # batch 1 at the same seed: the noise of image 0
    model.forward(x[:1], seed=7, **kw)
    plan1 = [p for p in model._plans.values() if p.rng and p.B == 1][0]
    assert torch.equal(plan1.eps[0], eps2[0]) and (not stochastic or torch.equal(plan1.noise[0], noise[0]))
    with pytest.raises(ValueError):
        model.forward(x, seed=7, eps=eps, **kw)
    with pytest.raises(ValueError):
        model.forward(x, seed=7, noise_map=noise, **kw)
    if stochastic:
        with pytest.raises(ValueError):                                    # without seed= the noise map is still required
            model.forward(x, eps=eps, **kw)
    return model, plan, out7

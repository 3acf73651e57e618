"""Seeded Gaussian noise on the device: the callers' ``torch.manual_seed(seed); torch.randn(...)`` (src/inference_paired.py:58-60, the seed
slider of gradio_sketch2image.py:80-82) under a fully specified contract -- Philox4x32-10 counters + Box-Muller, spelled out at
i2i_randn_params (include/i2i_turbo.h); tests/randn_ref.py is its CPU oracle.  Bit parity with torch.randn is not a goal (its stream is
unspecified and differs between CUDA and ROCm).

The same (seed, step, stream) gives the same bits from Python, from a C host and from a replayed graph: planned forwards built with
``rng=True`` (ForwardPlan, get_plan) fill their "eps" / "noise" buffers with this op from a 16-byte device state (``pack_state``) and advance
the step at the end of every run.  Stream 0 is the posterior draw ("eps"), stream 2 the sketch model's noise map ("noise"); stream 1 is
reserved for the reference's numerically dead scheduler draw.  The element index is flat, so image 0 of a batch gets the noise a batch-1
call gets."""
import contextlib
import ctypes as C

import torch

from . import _capi

STREAM_EPS, STREAM_NOISE = 0, 2


def split_seed(seed):
    """(seed_lo, seed_hi) of the Philox key: the seed reduced mod 2^64 (negative and oversized ints wrap)."""
    s = int(seed) & (2 ** 64 - 1)
    return s & 0xFFFFFFFF, s >> 32


def pack_state(seed, step=0):
    """The four uint32 {seed_lo, seed_hi, step, reserved = 0} of the device state (a plan's ``rng_state``, a plan file's "seed")."""
    lo, hi = split_seed(seed)
    return [lo, hi, int(step) & 0xFFFFFFFF, 0]


def as_i32(word):
    """A uint32 as the int32 with the same bits (torch's fill_ / tensor() of an int32 tensor refuse values >= 2^31)."""
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >= (1 << 31) else word


def _fill(out, kind, seed, step, stream, state, lib):
    lib = lib or _capi.default_library()
    dev = out.device
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    assert out.is_contiguous() and out.element_size() == 4
    p = _capi.RandnParams()
    p.dst, p.n, p.state = out.data_ptr(), out.numel(), (state.data_ptr() if state is not None else 0)
    p.seed, p.step, p.stream_id, p.kind = int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF, kind
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        hip_stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        lib.check(lib.lib.i2i_randn(C.addressof(p), 0, hip_stream))
    return out


def randn(shape, seed, step=0, stream=0, device="cuda", lib=None, state=None, out=None):
    """fp32 normal deviates of ``shape`` on ``device``: element i (flat) of (seed, step, stream).  Asynchronous on the current stream.
    ``state``: a 4-word device tensor read at run time instead of seed / step; ``out``: fill this contiguous fp32 tensor (or slice)."""
    if out is None:
        out = torch.empty(tuple(shape) if not isinstance(shape, int) else (shape,), dtype=torch.float32, device=device)
    assert out.dtype == torch.float32
    return _fill(out, _capi.RANDN_NORMAL, seed, step, stream, state, lib)


def raw_u32(n, seed, step=0, stream=0, device="cuda", lib=None, state=None):
    """The raw Philox words of the first ``n`` elements, as an int32 tensor holding the uint32 bits (``.view(torch.uint32)`` or numpy's
    ``.view(np.uint32)`` to read them unsigned)."""
    return _fill(torch.empty(int(n), dtype=torch.int32, device=device), _capi.RANDN_RAW, seed, step, stream, state, lib)

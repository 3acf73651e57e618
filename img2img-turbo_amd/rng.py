"""Seeded Gaussian noise on the device: the callers' ``torch.manual_seed(seed); torch.randn(...)`` (src/inference_paired.py:58-60, the seed
slider of gradio_sketch2image.py:80-82) under a fully specified contract -- Philox4x32-10 counters + Box-Muller, spelled out at
i2i_randn_params (include/i2i_turbo.h); tests/randn_ref.py is its CPU oracle.  Bit parity with torch.randn is not a goal (its stream is
unspecified and differs between CUDA and ROCm).

The same (seed, step, stream) gives the same bits from Python, from a C host and from a replayed graph: planned forwards built with
``rng=True`` (ForwardPlan, get_plan) fill their "eps" / "noise" buffers with this op from a 16-byte device state (``pack_state``) and advance
the step at the end of every run.  Stream 0 is the posterior draw ("eps"), stream 2 the sketch model's noise map ("noise"); stream 1 is
reserved for the reference's numerically dead scheduler draw.  The element index is flat, so image 0 of a batch gets the noise a batch-1
call gets.

Per-image states (``rng="per_image"``, ``randn_batch``, i2i_randn_batch_params): one {seed, step} row per image of the batch, every
image's element index starting at 0 -- row b of the result is bit-identical to a batch-1 ``randn`` at image b's seed and step, whatever
slot a batching host gave the request and whatever the batch size.  That fixes the NOISE of a request; it does not make image b of a
batch-8 forward bit-equal to a batch-1 forward (the contraction kernels choose their routes by batch size)."""
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


def pack_states(seeds, steps=0):
    """[B][4] words, row b = pack_state(seeds[b], steps[b]) (a per-image plan's ``rng_state``, its plan file's 16 * B byte "seed").
    ``steps``: one int for every row, or a sequence of B."""
    seeds = list(seeds)
    steps = [steps] * len(seeds) if isinstance(steps, int) else list(steps)
    if len(steps) != len(seeds):
        raise ValueError("pack_states: %d seeds but %d steps" % (len(seeds), len(steps)))
    return [pack_state(s, t) for s, t in zip(seeds, steps)]


def states_tensor(seeds, steps=0, device="cuda"):
    """pack_states as an int32 [B, 4] device tensor holding the uint32 bits."""
    rows = [[as_i32(w) for w in row] for row in pack_states(seeds, steps)]
    return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 4).to(device)


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


BATCH_MAX_BLOCKS = 1024      # csrc/elementwise.hip RANDN_BATCH_MAX_BLOCKS: workgroups of one batch fill, over all images


def batch_pass_elements(batch):
    """Elements per image one pass of the batch kernel's grid-stride loop covers (256 threads x 4 elements per workgroup): an image with
    more than this many elements makes the loop run again (what a test of that loop has to exceed)."""
    return (BATCH_MAX_BLOCKS // max(1, min(int(batch), BATCH_MAX_BLOCKS))) * 256 * 4


def _fill_batch(out, kind, batch, per_image, states, stream, lib):
    lib = lib or _capi.default_library()
    dev = states.device
    assert (lib.backend == "emu") == (dev.type == "cpu"), "library backend %s cannot take a tensor on %s" % (lib.backend, dev)
    assert states.is_contiguous() and states.element_size() == 4 and states.numel() == 4 * batch, "states: 4-byte words [batch, 4]"
    p = _capi.RandnBatchParams()
    if out is not None:
        assert out.device == dev and out.is_contiguous() and out.element_size() == 4 and out.numel() == batch * per_image
        p.dst = out.data_ptr()
    p.per_image, p.batch, p.states, p.stream_id, p.kind = int(per_image), int(batch), states.data_ptr(), int(stream) & 0xFFFFFFFF, kind
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        hip_stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        lib.check(lib.lib.i2i_randn_batch(C.addressof(p), 0, hip_stream))
    return out


def _states_for(batch, seeds, steps, states, device):
    if states is not None:
        return states
    seeds = list(seeds)
    if len(seeds) != batch:
        raise ValueError("%d seeds for a batch of %d" % (len(seeds), batch))
    return states_tensor(seeds, steps, device)


def randn_batch(shape, seeds, steps=0, stream=0, device="cuda", lib=None, states=None, out=None):
    """fp32 normal deviates of ``shape`` = [B, ...]: image b is ``randn(shape[1:], seeds[b], steps[b], stream)`` bit for bit, in any slot
    (i2i_randn_batch_params).  ``steps``: an int or B ints.  ``states``: an int32 [B, 4] device tensor read at run time instead of seeds /
    steps; ``out``: fill this contiguous fp32 tensor (or slice) of B * prod(shape[1:]) elements.  Asynchronous on the current stream."""
    shape = tuple(shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=(states.device if states is not None else device))
    assert out.dtype == torch.float32
    batch = int(shape[0])
    st = _states_for(batch, seeds, steps, states, out.device)
    return _fill_batch(out, _capi.RANDN_NORMAL, batch, out.numel() // batch if batch else 0, st, stream, lib)


def raw_u32_batch(batch, per_image, seeds, steps=0, stream=0, device="cuda", lib=None, states=None, out=None):
    """The raw Philox words [batch, per_image] of the same elements, as int32 holding the uint32 bits (see raw_u32)."""
    if out is None:
        out = torch.empty((int(batch), int(per_image)), dtype=torch.int32, device=(states.device if states is not None else device))
    st = _states_for(int(batch), seeds, steps, states, out.device)
    return _fill_batch(out, _capi.RANDN_RAW, int(batch), int(per_image), st, stream, lib)


def advance_batch(states, lib=None):
    """states[b][2] += 1 (wrapping) for every row of the int32 [B, 4] device tensor: what a per-image plan runs at the end of a forward."""
    _fill_batch(None, _capi.RANDN_ADVANCE, states.shape[0], 0, states, 0, lib)
    return states

"""Device fingerprints: the eager face of I2I_OP_DIGEST (the contract: i2i_digest_params, include/i2i_turbo.h; the kernel:
csrc/elementwise.hip digest_kernel).

    rec = digest(t)                         # uint64 [1, 4] = {s0, s1, elements, 0} of t's bits, computed where t lives
    rec = digest(batch, images=B)           # one record per image of a batch-outermost tensor
    first_diff(model_a.fingerprint(), model_b.fingerprint())   # -> (label, image) of the first tap that differs, or None

Two tensors with the same bits in the same logical order have the same record, whatever their pitch, alignment or device; a changed, moved
or swapped element changes it.  This detects accidents -- it is not a cryptographic hash.
"""
import ctypes as C

import torch

from . import _capi as K
from . import ops as O

_CODE = {torch.uint8: K.U8, torch.float16: K.F16, torch.bfloat16: K.BF16, torch.float32: K.F32}
_BY_SIZE = {1: K.U8, 2: K.F16, 4: K.F32}         # any other type of 1 / 2 / 4 bytes: the value is the bit pattern, only the size matters


def dtype_code(t):
    code = _CODE.get(t.dtype, _BY_SIZE.get(t.element_size()))
    if code is None:
        raise K.I2IError("digest: elements of %d bytes (%s) have no fingerprint: view the tensor as uint8" % (t.element_size(), t.dtype))
    return code


def _view_of(t, images):
    """(rows, cols, ld, img_stride) of ``t`` as `images` views with one pitch: contiguous, or 2-D [rows, cols] / 2-D [images, cols] / 3-D
    [images, rows, cols] with a unit stride in the last dimension."""
    images = int(images)
    if t.is_contiguous() or t.numel() == 0 or images == 0:
        per = t.numel() // max(images, 1)
        assert per * max(images, 1) == t.numel(), "digest: %d elements do not split into %d images" % (t.numel(), images)
        return 1, per, per, per
    if t.dim() == 2 and images == 1 and t.stride(1) == 1:
        return t.shape[0], t.shape[1], t.stride(0), t.shape[0] * t.stride(0)
    if t.dim() == 2 and t.shape[0] == images and t.stride(1) == 1:          # one row per image, the images a stride apart
        return 1, t.shape[1], t.shape[1], t.stride(0)
    if t.dim() == 3 and t.shape[0] == images and t.stride(2) == 1:
        return t.shape[1], t.shape[2], t.stride(1), t.stride(0)
    raise K.I2IError("digest: give a contiguous tensor, a [rows, cols] / [images, cols] view or an [images, rows, cols] view whose last stride is 1 "
                     "(got shape %s strides %s)" % (tuple(t.shape), tuple(t.stride())))


def digest(t, images=1, index0=0, lib=None):
    """uint64 [images, 4] = {s0, s1, elements, 0} per image of ``t`` (uint8 / fp16 / bf16 / fp32, or any type of 1, 2 or 4 bytes; views with
    a pitch are taken as they are, their pads unread).  Eager: one launch on the current stream of t's device and a read-back.  ``index0``: the
    logical index of every image's first element (digest a buffer in pieces: digest(A || B) = digest(A) + digest(B, index0 = len A))."""
    lib = lib or K.default_library()
    rows, cols, ld, img_stride = _view_of(t, images)
    assert cols < 2 ** 31, "digest: a row of %d elements; digest the tensor in pieces (index0)" % cols
    rec = torch.zeros(max(int(images), 1), 4, dtype=torch.int64, device=t.device)
    opc, p = O.digest(t, rec, images=images, rows=rows, cols=cols, ld=ld, img_stride=img_stride, index0=index0)
    cuda = t.device.type == "cuda"
    stream = C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if cuda else None
    if cuda:
        with torch.cuda.device(t.device):
            lib.check(lib.lib.i2i_digest(C.addressof(p), dtype_code(t), stream))
    else:
        lib.check(lib.lib.i2i_digest(C.addressof(p), dtype_code(t), stream))
    return rec[:int(images)].cpu().view(torch.uint64)


def first_diff(a, b):
    """The first (label, image) at which two fingerprint lists [(label, uint64 [B, 4])] differ -- in program order, lowest image first -- or
    None if they are equal.  The lists must come from plans with the same taps."""
    assert [l for l, _ in a] == [l for l, _ in b], "first_diff: the two fingerprints have different taps"
    for (label, ra), (_, rb) in zip(a, b):
        ra, rb = torch.as_tensor(ra).view(torch.int64).reshape(-1, 4), torch.as_tensor(rb).view(torch.int64).reshape(-1, 4)
        assert ra.shape == rb.shape, "first_diff: tap %s has %d and %d images" % (label, ra.shape[0], rb.shape[0])
        bad = (ra != rb).any(dim=1).nonzero()
        if bad.numel():
            return label, int(bad[0])
    return None

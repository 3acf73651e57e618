"""CPU oracle of the numerical health scan (i2i_scan, the contract in the comment of i2i_scan_params, include/i2i_turbo.h).

Works on RAW BIT PATTERNS (uint32 for fp32, uint16 for bf16 / fp16), so NaN payloads, -0 and subnormals are handled explicitly and no
float conversion of the host can flush or canonicalise anything.  ``scan_ref`` returns the record ONE launch adds to a zeroed one;
``accumulate`` combines records the way the device does (integer adds, an unsigned max for word 5).
"""
import numpy as np

FMT = {"f32": dict(word=np.uint32, abs=0x7FFFFFFF, inf=0x7F800000, sign=0x80000000),
       "bf16": dict(word=np.uint16, abs=0x7FFF, inf=0x7F80, sign=0x8000),
       "f16": dict(word=np.uint16, abs=0x7FFF, inf=0x7C00, sign=0x8000)}


def widen(a, fmt):
    """fp32 bit patterns (uint32) of the finite, non-negative patterns ``a`` of format ``fmt`` (exact in every format)."""
    a = np.asarray(a, dtype=np.uint32)
    if fmt == "f32":
        return a.copy()
    if fmt == "bf16":
        return a << np.uint32(16)
    e, m = a >> np.uint32(10), a & np.uint32(0x3FF)
    normal = ((e + np.uint32(112)) << np.uint32(23)) | (m << np.uint32(13))
    sub = (m.astype(np.float64) * 2.0 ** -24).astype(np.float32).view(np.uint32)      # m * 2^-24: exact, a normal fp32 number (or 0)
    return np.where(e > 0, normal, sub).astype(np.uint32)


def scan_ref(array, cols, ld, limit, fmt="f32", rows=None):
    """array: flat raw patterns of a rows x cols view with row pitch ld (elements [cols, ld) of a row are ignored, whatever they hold)."""
    f = FMT[fmt]
    array = np.ascontiguousarray(array).reshape(-1)
    assert array.dtype == f["word"], (array.dtype, fmt)
    assert ld >= cols
    if rows is None:
        rows = 0 if (cols == 0 or array.size < cols) else (array.size - cols) // ld + 1
    rec = np.zeros(8, dtype=np.uint64)
    rec[0] = 1
    rec[6] = rows * cols
    if rows * cols:
        if ld == cols:
            v = array[:rows * cols]
        else:
            idx = (np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]).reshape(-1)
            v = array[idx]
        v = v.astype(np.uint32)
        a = v & np.uint32(f["abs"])
        neg = (v & np.uint32(f["sign"])) != 0
        rec[1] = np.count_nonzero(a > f["inf"])
        rec[2] = np.count_nonzero((a == f["inf"]) & ~neg)
        rec[3] = np.count_nonzero((a == f["inf"]) & neg)
        fin = a[a < f["inf"]]
        if fin.size:
            w = widen(fin, fmt)
            lim = np.float32(limit)
            rec[4] = np.count_nonzero(w.view(np.float32).astype(np.float64) > np.float64(lim))      # strict; exact in fp64
            rec[5] = int(w.max())                                                                    # non-negative fp32 patterns order like the values
    return rec


def accumulate(a, b):
    out = a + b
    out[5] = max(a[5], b[5])
    out[7] = 0
    return out


def bits_of(t):
    """Raw patterns of a torch tensor (cpu) as a flat numpy array, and the format name."""
    import torch
    t = t.detach().cpu().contiguous().reshape(-1)
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32), "f32"
    return t.view(torch.int16).numpy().view(np.uint16), {torch.bfloat16: "bf16", torch.float16: "f16"}[t.dtype]

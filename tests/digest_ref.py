"""CPU oracle of the device fingerprint (i2i_digest; the contract is the comment of i2i_digest_params in include/i2i_turbo.h): numpy on raw bit
patterns, uint64 arithmetic that wraps mod 2^64.  Nothing here knows about grids, chunks or alignment -- that is the point."""
import numpy as np

W = np.uint64(0x9E3779B97F4A7C15)
K1 = np.uint64(0xFF51AFD7ED558CCD)
K2 = np.uint64(0xC4CEB9FE1A85EC53)
K3 = np.uint64(0xD6E8FEB86659FD93)
WORD = {1: np.uint8, 2: np.uint16, 4: np.uint32}
BLOCK = 1 << 20


def _s(n):
    return np.uint64(n)


def mix(j, v):
    """(H0, H1) of index j (uint64 array) and value v (bit patterns, zero-extended): the MIXERS paragraph of the contract."""
    with np.errstate(over="ignore"):
        m = (np.asarray(j, dtype=np.uint64) * W) ^ np.asarray(v).astype(np.uint64)
        m = m ^ (m >> _s(33))
        m = m * K1
        m = m ^ (m >> _s(33))
        m = m * K2
        h0 = m ^ (m >> _s(33))
        t = (h0 ^ (h0 >> _s(31))) * K3
        h1 = t ^ (t >> _s(32))
    return h0, h1


def bits_of(t):
    """Raw words of a torch tensor (uint8 / fp16 / bf16 / fp32 / any integer type of 1, 2 or 4 bytes), flattened in memory order."""
    import torch
    t = t.detach().cpu().contiguous()
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.view(idt).numpy().view(WORD[t.element_size()]).reshape(-1)


def digest_ref(flat, rows, cols, ld=None, index0=0):
    """The record {s0, s1, elements, 0} of the rows x cols view (pitch ld) that starts at flat[0]; flat holds raw words."""
    ld = cols if ld is None else ld
    if rows * cols == 0:
        return np.zeros(4, dtype=np.uint64)
    flat = np.asarray(flat)
    s0 = s1 = np.uint64(0)
    with np.errstate(over="ignore"):
        for at in range(0, rows * cols, BLOCK):          # in blocks: a 16 MiB case would otherwise hold a dozen 128 MiB temporaries
            p = np.arange(at, min(at + BLOCK, rows * cols), dtype=np.int64)
            h0, h1 = mix(np.uint64(index0 & (2 ** 64 - 1)) + p.astype(np.uint64), flat[(p // cols) * ld + p % cols])
            s0, s1 = s0 + h0.sum(dtype=np.uint64), s1 + h1.sum(dtype=np.uint64)
    return np.array([s0, s1, rows * cols, 0], dtype=np.uint64)


def digest_batch_ref(flat, images, rows, cols, ld=None, img_stride=None, index0=0):
    ld = cols if ld is None else ld
    img_stride = rows * ld if img_stride is None else img_stride
    return np.stack([digest_ref(np.asarray(flat)[b * img_stride:], rows, cols, ld, index0) for b in range(images)]) if images else np.zeros((0, 4), np.uint64)


def add(a, b):
    with np.errstate(over="ignore"):
        return (np.asarray(a, dtype=np.uint64) + np.asarray(b, dtype=np.uint64)).astype(np.uint64)

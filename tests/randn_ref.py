"""CPU oracle of the seeded-noise contract (i2i_randn_params, include/i2i_turbo.h): Philox4x32-10 in integer numpy and the Box-Muller
transform in fp64.  Independent of the kernels: nothing here is shared with csrc/ or with img2img_turbo_amd/rng.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: two ints -> uint32 [..., 4] (Random123's philox4x32, 10 rounds)."""
    c = [np.asarray(ctr[..., j], dtype=np.uint64) for j in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def raw(n, seed, step=0, stream=0):
    """The first n words of (seed, step, stream): element i is lane i & 3 of counter {q lo, q hi, step, stream}, q = i >> 2."""
    seed = int(seed) % (1 << 64)
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    ctr = np.empty((nq, 4), dtype=np.uint32)
    ctr[:, 0] = (q & MASK).astype(np.uint32)
    ctr[:, 1] = (q >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = int(step) & 0xFFFFFFFF
    ctr[:, 3] = int(stream) & 0xFFFFFFFF
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]


def normal(n, seed, step=0, stream=0):
    """(values fp64 [n], rad fp64 [n]): the exact transform of the same words; rad is the Box-Muller radius of each element's pair."""
    w = raw(4 * ((n + 3) // 4), seed, step, stream).reshape(-1, 2)
    u1 = ((w[:, 0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> 8).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    val = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).reshape(-1)[:n]
    return val, np.repeat(rad, 2)[:n]

"""CPU oracle of the tiled forward's two ends (the contract above i2i_tile_request, include/i2i_turbo.h): the layout rule, the cut (numpy
slicing) and the integer feather blend, in int64 numpy.  Independent of the kernels: nothing here is shared with csrc/ or with
img2img_turbo_amd/image_ops.py."""
import numpy as np


def positions(L, t, ov):
    """x_k = min(k * s, L - t) for k < n = 1 + ceil((L - t) / s), s = t - ov."""
    assert t > 0 and t % 8 == 0 and ov % 8 == 0 and 0 <= ov <= t // 2 and L >= t, (L, t, ov)
    s = t - ov
    n = 1 + (L - t + s - 1) // s
    return [min(k * s, L - t) for k in range(n)]


def origins(h, w, tw, th, ov, xs=None, ys=None):
    """[(y0, x0)] of a request's tiles, row-major (ky outer, kx inner)."""
    xs = positions(w, tw, ov) if xs is None else xs
    ys = positions(h, th, ov) if ys is None else ys
    return [(y0, x0) for y0 in ys for x0 in xs]


def cut(a, org, tw, th, axes=(0, 1)):
    """The tiles of one request by slicing: ``a`` is [h, w, c] (axes (0, 1)) or [planes, h, w] (axes (1, 2)) -> [n, ...] tiles."""
    out = []
    for y0, x0 in org:
        sl = [slice(None)] * a.ndim
        sl[axes[0]], sl[axes[1]] = slice(y0, y0 + th), slice(x0, x0 + tw)
        out.append(a[tuple(sl)])
    return np.stack(out)


def feather(t, ramp):
    i = np.arange(t, dtype=np.int64)
    return np.minimum(np.minimum(i + 1, t - i), ramp)


def blend(tiles, h, w, org, ramp):
    """tiles uint8 [n, th, tw, c] at ``org`` -> (uint8 [h, w, c], whether some pixel has no cover): num = sum w * u8, den = sum w,
    out = (2 * num + den) // (2 * den), 0 without a cover."""
    n, th, tw, c = tiles.shape
    assert n == len(org) and 1 <= ramp <= 256
    wgt = np.outer(feather(th, ramp), feather(tw, ramp))
    assert wgt.min() >= 1
    num = np.zeros((h, w, c), dtype=np.int64)
    den = np.zeros((h, w), dtype=np.int64)
    for t, (y0, x0) in enumerate(org):
        num[y0:y0 + th, x0:x0 + tw] += wgt[:, :, None] * tiles[t].astype(np.int64)
        den[y0:y0 + th, x0:x0 + tw] += wgt
    assert (2 * num + den[:, :, None]).max() < 2 ** 32          # the bound the header states for the kernel's uint32 accumulators
    safe = np.maximum(den, 1)[:, :, None]
    out = np.where(den[:, :, None] > 0, (2 * num + den[:, :, None]) // (2 * safe), 0)
    assert out.max() <= 255
    return out.astype(np.uint8), bool((den == 0).any())

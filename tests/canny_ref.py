"""CPU oracle of the Canny contract in include/i2i_turbo.h (i2i_canny_u8_params): cv::Canny(src, low, high) for 8-bit input with aperture 3
and L2gradient = false, restated in integer arithmetic.  Whole-image vectorised numpy plus scipy.ndimage.label for the hysteresis; no
tiles, no device code -- written independently of the structure of the kernels in csrc/resize.hip.

OpenCV is not installed where this project is built and tested, so parity with cv2 itself is UNPINNED here;
tests/test_canny_emu.py::test_oracle_matches_opencv pins it wherever ``import cv2`` works.  If that test ever fails, this file and the
contract are what is wrong, not OpenCV.
"""
import numpy as np
from scipy import ndimage

TG22 = 13573          # tan(22.5 deg) * 2^15, as OpenCV rounds it


def thresholds(low, high):
    low, high = int(np.floor(low)), int(np.floor(high))
    return (high, low) if low > high else (low, high)


def sobel(img):
    """img uint8 [H, W, C] -> (dx, dy) int32 [H, W, C]: 3x3 Sobel with BORDER_REPLICATE."""
    p = np.pad(img.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = img.shape[:2]

    def at(dy, dx):
        return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    dx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    dy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return dx, dy


def gradient(img):
    """(dx, dy, mag) int32 [H, W] of the channel with the largest |dx| + |dy| per pixel (lowest channel on a tie)."""
    dx, dy = sobel(img)
    mag = np.abs(dx) + np.abs(dy)
    ch = np.argmax(mag, axis=2)[..., None]          # argmax returns the FIRST maximum
    pick = lambda a: np.take_along_axis(a, ch, axis=2)[..., 0]
    return pick(dx), pick(dy), pick(mag)


def classify(img, low, high):
    """Class map uint8 [H, W]: 0 none, 1 weak candidate, 2 strong candidate (after non-maximum suppression)."""
    low, high = thresholds(low, high)
    dx, dy, mag = gradient(img)
    H, W = mag.shape
    mp = np.pad(mag, 1, mode="constant")            # magnitude outside the image is 0

    def nb(r, c):                                   # mag[y + r][x + c]; c may be an array of per-pixel offsets
        yy = np.arange(H)[:, None] + 1 + r
        xx = np.arange(W)[None, :] + 1 + c
        return mp[yy, xx]
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    tg22x = x * TG22
    tg67x = tg22x + (x << 16)
    horiz = y < tg22x
    vert = ~horiz & (y > tg67x)
    s = np.where((dx ^ dy) < 0, -1, 1)
    keep = np.where(horiz, (mag > nb(0, -1)) & (mag >= nb(0, 1)),
                    np.where(vert, (mag > nb(-1, 0)) & (mag >= nb(1, 0)),
                             (mag > nb(-1, -s)) & (mag > nb(1, s))))
    cand = keep & (mag > low)
    return np.where(cand, np.where(mag > high, 2, 1), 0).astype(np.uint8)


def components(cls):
    """8-connected components of the candidates: (labels int32 [H, W] with 0 = none, count)."""
    return ndimage.label(cls > 0, structure=np.ones((3, 3), dtype=np.int32))


def hysteresis(cls):
    """bool [H, W]: candidates whose 8-connected component of candidates holds a strong pixel."""
    lab, n = components(cls)
    has_strong = np.zeros(n + 1, dtype=bool)
    has_strong[lab[cls == 2]] = True
    has_strong[0] = False
    return has_strong[lab]


def canny(img, low=100, high=200, out_channels=1):
    """img uint8 [H, W] or [H, W, C] -> uint8 [H, W, out_channels] (255 on edges)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    assert img.dtype == np.uint8 and img.ndim == 3 and 1 <= img.shape[2] <= 4
    edges = hysteresis(classify(img, low, high))
    return np.repeat((edges.astype(np.uint8) * 255)[..., None], out_channels, axis=2)


def canny_batch(images, low=100, high=200, out_channels=3):
    """images uint8 [N, H, W, C] -> uint8 [N, H, W, out_channels]."""
    return np.stack([canny(im, low, high, out_channels) for im in np.asarray(images)])


def geodesic_reach(cls):
    """Largest 8-connected geodesic distance (in steps through candidates) from the strong pixels to any candidate they reach."""
    cand = cls > 0
    seen = cls == 2
    steps = 0
    st = np.ones((3, 3), dtype=bool)
    while True:
        nxt = ndimage.binary_dilation(seen, structure=st) & cand
        if (nxt == seen).all():
            return steps
        seen = nxt
        steps += 1

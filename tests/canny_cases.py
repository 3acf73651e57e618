"""Inputs and backend-independent checks shared by tests/test_canny_emu.py (CPU emulator) and tests/test_canny_gpu.py (MI355X): the same
cases run through image_ops.canny_u8 on both, bit-exact against tests/canny_ref.py.  The kernels work on 64 x 16 tiles (csrc/resize.hip)."""
import ctypes as C
import functools

import numpy as np
import torch
from scipy import ndimage

import canny_ref

TILE_W, TILE_H = 64, 16

# (h, w): tiny, smaller than a tile, odd with w*c not a multiple of 4, and 3 x 3 tiles with a ragged last tile in both directions
SIZES = [(1, 1), (2, 3), (7, 5), (40, 56), (37, 53), (41, 150)]


@functools.lru_cache(maxsize=None)
def smooth_noise(n, h, w, c, seed=0):
    """Random bytes box-filtered 5 x 5, a different image per slot (raw noise makes every candidate strong; the box filter leaves ~30 % of
    the pixels weak candidates, a third or more of which hysteresis drops at thresholds (100, 200))."""
    rng = np.random.default_rng(1000 * seed + 17 * h + w + c)
    raw = rng.integers(0, 256, (n, h, w, c)).astype(np.float64)
    img = np.rint(ndimage.uniform_filter(raw, size=(1, 5, 5, 1), mode="nearest")).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def oracle(key, low=100, high=200, out_c=3):
    """Oracle result of a named input (computed once per session, read-only)."""
    out = canny_ref.canny_batch(IMAGES[key](), low, high, out_c)
    out.setflags(write=False)
    return out


def snake(h=96, w=136, c=3, seeded=True, y0=4, rows=None, x_margin=6):
    """A serpentine band of value 30 on 0 (5 pixels thick, row pitch 12, turning at alternate ends); ``seeded``: a 5 x 4 block of 120 at the
    start of the first band -- the only place whose gradient exceeds the high threshold."""
    img = np.zeros((h, w, c), dtype=np.uint8)
    rows = rows if rows is not None else (h - y0 - 5) // 12 + 1
    x_lo, x_hi = x_margin, w - x_margin
    for r in range(rows):
        y = y0 + 12 * r
        img[y:y + 5, x_lo:x_hi] = 30
        if r + 1 < rows:                                   # the turn: a vertical piece at alternating ends
            xs = slice(x_hi - 5, x_hi) if r % 2 == 0 else slice(x_lo, x_lo + 5)
            img[y:y + 12 + 5, xs] = 30
    if seeded:
        img[y0:y0 + 5, x_lo:x_lo + 4] = 120
    return img


def two_snakes():
    """Two separate snakes in one image (upper seeded, lower not): only the seeded one survives hysteresis."""
    img = np.zeros((96, 136, 3), dtype=np.uint8)
    img[:48] = snake(48, 136, 3, seeded=True)
    img[48:] = snake(48, 136, 3, seeded=False)
    return img


IMAGES = {
    "snake": lambda: snake()[None],
    "snake_seedless": lambda: snake(seeded=False)[None],
    "two_snakes": lambda: two_snakes()[None],
}
for _h, _w in SIZES:
    for _c in (1, 3, 4):
        IMAGES["noise_%dx%dx%d" % (_h, _w, _c)] = functools.partial(smooth_noise, 3, _h, _w, _c)

SIZE_CASES = [("noise_%dx%dx%d" % (h, w, c), oc) for (h, w) in SIZES for c, oc in ((1, 1), (3, 3), (4, 1), (3, 1), (1, 3))]


def class_stats(img, low=100, high=200):
    """Over a batch: (weak candidates / pixels, candidates dropped by hysteresis / candidates)."""
    weak = cand = dropped = pixels = 0
    for im in img:
        cls = canny_ref.classify(im, low, high)
        edges = canny_ref.hysteresis(cls)
        pixels += cls.size
        weak += int((cls == 1).sum())
        cand += int((cls > 0).sum())
        dropped += int(((cls > 0) & ~edges).sum())
    return weak / pixels, dropped / max(cand, 1)


# ---------------------------------------------------------------------------------------------------------------- device plumbing
def to_dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)          # (a copy: the cached inputs are read-only)


def run_canny(lib, device, img, low=100, high=200, out_c=3):
    from img2img_turbo_amd import image_ops
    out = image_ops.canny_u8(to_dev(img, device), low, high, out_c, lib=lib)
    return out.cpu().numpy()


def raw_call(lib, device, src, *, low=100, high=200, out_c=3, thr=None, ws=None, dst=None, c=None, null=None, ws_offset=0):
    """i2i_canny_u8 through the raw C entry.  Returns (status, dst tensor, ws tensor)."""
    from img2img_turbo_amd import _capi as K
    n, h, w, cc = src.shape
    if dst is None:
        dst = torch.full((n, h, w, max(out_c, 1)), 7, dtype=torch.uint8, device=device)
    if ws is None:
        ws = torch.empty(lib.canny_ws_bytes(n, h, w) + 32, dtype=torch.uint8, device=device)
    p = K.CannyU8Params()
    p.src, p.dst, p.ws = src.data_ptr(), dst.data_ptr(), ws.data_ptr() + ws_offset
    p.thr_dev = thr.data_ptr() if thr is not None else 0
    p.n, p.h, p.w, p.c, p.out_c, p.low, p.high = n, h, w, (cc if c is None else c), out_c, low, high
    if null:
        setattr(p, null, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None
    rc = lib.lib.i2i_canny_u8(C.addressof(p), 0, stream)
    if device != "cpu":
        torch.cuda.synchronize()
    return rc, dst, ws


# ---------------------------------------------------------------------------------------------------------------- shared checks
def check_sizes(lib, device, key, out_c):
    img = IMAGES[key]()
    h, w = img.shape[1:3]
    # On the oracle alone: the case cannot pass with hysteresis missing or with every candidate strong.  (Asked of the images of at least
    # 37 x 53 pixels; the 1 x 1, 2 x 3 and 7 x 5 ones hold between zero and a handful of candidates and are there for the borders.)
    if h * w >= 37 * 53:
        weak, dropped = class_stats(img)
        assert weak >= 0.10 and dropped >= 0.05, (key, weak, dropped)
    got = run_canny(lib, device, img, out_c=out_c)
    want = oracle(key, 100, 200, out_c)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (key, out_c, int((got != want).sum()))


def check_snakes(lib, device):
    img = IMAGES["snake"]()
    cls = canny_ref.classify(img[0], 100, 200)
    _, ncomp = canny_ref.components(cls)
    cand, strong = int((cls > 0).sum()), int((cls == 2).sum())
    reach = canny_ref.geodesic_reach(cls)
    print("[canny] snake: %d candidates in %d component(s), %d strong, geodesic reach %d steps" % (cand, ncomp, strong, reach))
    assert ncomp == 1 and 0 < strong < 0.02 * cand and reach >= 8 * max(TILE_W, TILE_H), (ncomp, strong, cand, reach)
    want = oracle("snake")
    assert int((want[0, :, :, 0] > 0).sum()) == cand          # the whole chain is an edge
    got = run_canny(lib, device, img)
    assert np.array_equal(got, want), int((got != want).sum())
    # the same image without the bright block: candidates, but nothing strong -> nothing at all
    twin = IMAGES["snake_seedless"]()
    cls0 = canny_ref.classify(twin[0], 100, 200)
    assert (cls0 > 0).sum() > 1000 and (cls0 == 2).sum() == 0
    got0 = run_canny(lib, device, twin)
    assert not got0.any() and np.array_equal(got0, oracle("snake_seedless"))
    # two snakes, one seeded: only that one survives
    two = IMAGES["two_snakes"]()
    want2 = oracle("two_snakes")
    assert want2[0, :48].any() and not want2[0, 48:].any() and (canny_ref.classify(two[0], 100, 200)[48:] > 0).sum() > 500
    got2 = run_canny(lib, device, two)
    assert np.array_equal(got2, want2), int((got2 != want2).sum())


def check_thresholds(lib, device):
    key = "noise_41x150x3"
    img = IMAGES[key]()
    src = to_dev(img, device)
    want = oracle(key)
    # low > high is swapped; float thresholds are floored
    assert np.array_equal(run_canny(lib, device, img, 200, 100), want)
    assert np.array_equal(run_canny(lib, device, img, 100.9, 200.9), want)
    want_b = oracle(key, 60, 120)
    assert not np.array_equal(want, want_b)
    # thr_dev overrides the struct's values; two runs of ONE op (same struct, same workspace) with different contents
    thr = torch.tensor([60, 120], dtype=torch.int32, device=device)
    rc, dst, ws = raw_call(lib, device, src, low=1, high=2, thr=thr)
    assert rc == 0 and np.array_equal(dst.cpu().numpy(), want_b)
    thr.copy_(torch.tensor([200, 100], dtype=torch.int32))     # (swapped on the device too)
    rc, dst, ws = raw_call(lib, device, src, low=1, high=2, thr=thr, ws=ws, dst=dst)
    assert rc == 0 and np.array_equal(dst.cpu().numpy(), want)
    # a dirty workspace: nothing has to be zeroed, and nothing is carried from run to run
    ws.fill_(0xFF)
    rc, d1, ws = raw_call(lib, device, src, ws=ws)
    first = d1.cpu().numpy().copy()
    rc2, d2, ws = raw_call(lib, device, src, ws=ws)
    assert rc == 0 and rc2 == 0 and np.array_equal(first, want) and np.array_equal(d2.cpu().numpy(), want)


def check_abi(lib, device):
    from img2img_turbo_amd import _capi as K
    src = to_dev(IMAGES["noise_7x5x3"](), device)
    bad = [dict(null="src"), dict(null="dst"), dict(null="ws"), dict(c=5), dict(c=0), dict(out_c=2), dict(ws_offset=4)]
    for kw in bad:
        rc, dst, _ = raw_call(lib, device, src, **kw)
        assert rc == -1, (kw, rc)                              # I2I_ERR_BAD_ARG
        assert lib.lib.i2i_last_error().decode().startswith("canny_u8:"), kw
        assert bool((dst == 7).all()), kw                      # dst untouched
        with __import__("pytest").raises(K.I2IError):
            lib.check(rc)
    f = lib.canny_ws_bytes
    assert f(1, 1, 1) >= 9 and f(1, 1, 1) % 16 == 0 and f(0, 4, 4) == 0
    for a, b in (((1, 37, 53), (2, 37, 53)), ((2, 37, 53), (2, 38, 53)), ((2, 37, 53), (2, 37, 54)), ((8, 512, 512), (8, 512, 513))):
        assert f(*a) <= f(*b) and f(*a) >= 9 * a[0] * a[1] * a[2]
    assert f(8, 512, 512) < f(16, 512, 512) and f(8, 512, 512) < f(8, 1024, 512) and f(8, 512, 512) < f(8, 512, 1024)


def pipeline_inputs(n, h, w):
    """Photos of an odd size for the tiny architecture, the text states and the posterior noise (as test_u8_pipeline_with_device_side_resize)."""
    from oracle import TINY_UNET
    g = torch.Generator().manual_seed(11)
    img = np.concatenate([smooth_noise(1, h, w, 3, seed=5 + i) for i in range(n)])
    cap = torch.randn(1, 77, TINY_UNET.cross_attention_dim, generator=g)
    eps = torch.randn(n, 4, h // 8, w // 8, generator=g)
    return img, cap, eps


def host_edges(img, low, high):
    """The script on the host: Pillow's LANCZOS resize to a multiple of 8, then the oracle's Canny replicated to 3 channels."""
    from PIL import Image
    n, h, w, _ = img.shape
    res = np.stack([np.asarray(Image.fromarray(im, "RGB").resize((w - w % 8, h - h % 8), Image.LANCZOS)) for im in img])
    return canny_ref.canny_batch(res, low, high, 3)


def check_pipeline(lib, device, model, n=2, h=77, w=93):
    """forward_u8(resize=..., canny=...) equals forward_u8 of the host-made edge maps, bit for bit; other thresholds reuse the plan.
    (The emulator runs one 37 x 45 photo: a forward of the tiny model costs it a second per thousand pixels.)"""
    img, cap, eps = pipeline_inputs(n, h, w)
    capd, epsd = cap.to(device), eps.to(device)
    outs = {}
    for thr in ((100, 200), (40, 90)):
        edges = host_edges(img, *thr)
        assert edges.any() and not edges.all()
        out_dev = model.forward_u8(to_dev(img, device), caption_enc=capd, eps=epsd, resize="multiple_of_8", canny=thr)
        out_host = model.forward_u8(to_dev(edges, device), caption_enc=capd, eps=epsd)
        assert out_dev.shape == (n, h - h % 8, w - w % 8, 3) and torch.equal(out_dev, out_host), thr
        outs[thr] = out_dev.cpu()
        # one plan with the Canny op in front and the plain uint8 plan of the host twin: other thresholds do not re-plan
        assert len(model._plans) == 2 and sum(1 for p in model._plans.values() if p.canny) == 1, len(model._plans)
    assert not torch.equal(outs[(100, 200)], outs[(40, 90)])
    with __import__("pytest").raises(ValueError):
        model.forward_u8(to_dev(img, device), caption_enc=capd, eps=epsd, resize="multiple_of_8", canny=True, sketch=True)
    return img, cap, eps, outs

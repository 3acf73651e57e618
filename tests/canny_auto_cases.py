"""Inputs and backend-independent checks shared by tests/test_canny_auto_emu.py (CPU emulator) and tests/test_canny_auto_gpu.py (MI355X):
the automatic Canny thresholds (i2i_canny_auto_thr, csrc/resize.hip) against tests/canny_auto_ref.py, bit for bit, through the raw C entry,
the eager forms of image_ops, the planned forward and the model class.  The histogram kernel walks an image in 16-byte chunks from the
first 16-byte boundary behind ITS start (byte loads in front and behind), a workgroup is sized for 1024 chunks, and a launch is capped at
1024 workgroups -- the shapes below are the smallest that reach each of those paths."""
import ctypes as C
import functools

import numpy as np
import torch

import canny_auto_ref as ar
import canny_cases as cc
import canny_ref

S33 = 21627                      # sigma_to_q16(0.33)
THR_SENTINEL, MED_SENTINEL = -7, 0xABCD


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


def _two_valued(h, w, c, k, lo=40, hi=200, seed=0):
    """k bytes of `lo` and the rest `hi`, shuffled."""
    flat = np.full(h * w * c, hi, dtype=np.uint8)
    flat[:k] = lo
    np.random.default_rng(seed + k).shuffle(flat)
    return flat.reshape(h, w, c)


def _odd_m2():
    """8 x 8 x 3: N = 192 is even and the two middle values differ (100 | 101): m2 = 201 is odd."""
    return _two_valued(8, 8, 3, 96, lo=100, hi=101)[None]


def _many():
    return np.random.default_rng(5).integers(0, 256, (1030, 3, 3, 1), dtype=np.uint8)


# name -> (images uint8 [n, h, w, c], sigma_q16 per image)
CASES = {
    "1x1x1": lambda: (np.full((1, 1, 1, 1), 77, dtype=np.uint8), [S33]),
    "8x8x3_odd_m2": lambda: (_odd_m2(), [S33]),
    "37x29x3": lambda: (cc.smooth_noise(1, 37, 29, 3, seed=2), [S33]),                    # N = 3219: odd, head and tail both non-empty
    "batch3_unaligned": lambda: (cc.smooth_noise(3, 37, 29, 3, seed=3), [S33] * 3),       # images start 3219 bytes apart
    "c1": lambda: (cc.smooth_noise(2, 19, 23, 1, seed=4), [S33] * 2),
    "c2": lambda: (cc.smooth_noise(2, 19, 23, 2, seed=4), [S33] * 2),
    "c4": lambda: (cc.smooth_noise(2, 19, 23, 4, seed=4), [S33] * 2),
    "zeros": lambda: (np.zeros((1, 16, 16, 3), dtype=np.uint8), [S33]),                   # m2 = 0 -> (0, 0)
    "all_255": lambda: (np.full((1, 16, 16, 3), 255, dtype=np.uint8), [S33]),             # high clamps to 255
    "split_even": lambda: (np.stack([_two_valued(10, 10, 1, k) for k in (49, 50, 51)]), [S33] * 3),      # N = 100: the split at N / 2 +- 1
    "split_odd": lambda: (np.stack([_two_valued(9, 11, 1, k) for k in (49, 50)]), [S33] * 2),            # N = 99: one middle element
    "one_bin_256x256x3": lambda: (np.full((1, 256, 256, 3), 131, dtype=np.uint8), [S33]),                # LDS contention; 12 workgroups
    "noise_2x96x128x3": lambda: (cc.smooth_noise(2, 96, 128, 3, seed=6), [S33] * 2),                     # 3 workgroups per image
    "many_images": lambda: (_many(), [S33] * 1030),                                                      # more images than grid rows
    "sigma_edges": lambda: (cc.smooth_noise(4, 21, 17, 3, seed=7), [0, 65536, 100000, 16384]),           # 0, 1, above 1 (clamped), 0.25
    "manual_slot": lambda: (cc.smooth_noise(3, 21, 17, 3, seed=8), [S33, -1, 32768]),
}
CASE_NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    img, sig = CASES[name]()
    return _frozen(img), tuple(sig)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(thr, median2) of a case on sentinel-filled outputs (computed once per session)."""
    img, sig = case(name)
    n = len(img)
    thr, med = ar.auto_thresholds(img, sig, np.full((n, 2), THR_SENTINEL), np.full(n, MED_SENTINEL))
    thr.setflags(write=False)
    med.setflags(write=False)
    return thr, med


# ---------------------------------------------------------------------------------------------------------------- device plumbing
def device_bytes(a, device, offset=0):
    """The array's bytes in device memory starting ``offset`` bytes behind an allocation's start: (owner tensor, address)."""
    flat = torch.from_numpy(np.array(a).reshape(-1))
    buf = torch.zeros(flat.numel() + offset + 16, dtype=torch.uint8, device=device)
    buf[offset:offset + flat.numel()] = flat.to(device)
    return buf, buf.data_ptr() + offset


def raw_call(lib, device, img, sig, *, offset=0, ws=None, null=None, want_median=True, params_null=False, **over):
    """i2i_canny_auto_thr through the raw C entry on sentinel-filled outputs.  ``over``: struct fields to overwrite (n, h, w, c) or
    ``X_offset`` = bytes added to pointer X.  Returns (status, thr tensor, median2 tensor, ws tensor)."""
    from img2img_turbo_amd import _capi as K
    n, h, w, c = img.shape
    keep, src = device_bytes(img, device, offset)
    sigma = torch.tensor(list(sig), dtype=torch.int32).to(device)
    thr = torch.full((n + 1, 2), THR_SENTINEL, dtype=torch.int32, device=device)           # (one spare row: room for a misaligned pointer)
    med = torch.full((n + 1,), MED_SENTINEL, dtype=torch.int32, device=device)
    if ws is None:
        ws = torch.full((lib.canny_auto_ws_bytes(n) + 32,), 0xFF, dtype=torch.uint8, device=device)
    p = K.CannyAutoThrParams()
    p.src, p.sigma_q16, p.thr, p.ws = src, sigma.data_ptr(), thr.data_ptr(), ws.data_ptr()
    p.median2 = med.data_ptr() if want_median else 0
    p.n, p.h, p.w, p.c = n, h, w, c
    for k, v in over.items():
        if k.endswith("_offset"):
            setattr(p, k[:-7], getattr(p, k[:-7]) + v)
        else:
            setattr(p, k, v)
    if null:
        setattr(p, null, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None
    rc = lib.lib.i2i_canny_auto_thr(None if params_null else C.addressof(p), 0, stream)
    if device != "cpu":
        torch.cuda.synchronize()
    del keep
    return rc, thr, med, ws


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- shared checks
def check_case(lib, device, name):
    """thr and median2 equal the oracle bit for bit on a workspace full of 0xFF, at the allocation's alignment and one byte behind it; a second
    call on the workspace the first one left gives the same."""
    img, sig = case(name)
    n = len(img)
    want_thr, want_med = oracle(name)
    for offset in (0, 1):
        rc, thr, med, ws = raw_call(lib, device, img, sig, offset=offset)
        assert rc == 0, lib.lib.i2i_last_error().decode()
        got_thr, got_med = thr.cpu().numpy()[:n], as_u32(med)[:n]
        assert np.array_equal(got_thr, want_thr), (name, offset, got_thr.tolist()[:4], want_thr.tolist()[:4])
        assert np.array_equal(got_med, want_med), (name, offset, got_med.tolist()[:4], want_med.tolist()[:4])
        assert (thr.cpu().numpy()[n:] == THR_SENTINEL).all() and as_u32(med)[n] == MED_SENTINEL            # nothing behind the table
    rc, thr2, med2, _ = raw_call(lib, device, img, sig, offset=1, ws=ws)
    assert rc == 0 and torch.equal(thr2, thr) and torch.equal(med2, med), name
    # median2 is optional
    rc, thr3, med3, _ = raw_call(lib, device, img, sig, want_median=False)
    assert rc == 0 and np.array_equal(thr3.cpu().numpy()[:n], want_thr) and bool((med3 == MED_SENTINEL).all()), name


def check_known_answers():
    """The oracle's own hand-checked values of the cases above."""
    assert oracle("zeros")[0].tolist() == [[0, 0]] and oracle("zeros")[1].tolist() == [0]
    assert oracle("all_255")[0].tolist() == [[(510 * (65536 - S33)) >> 17, 255]] and oracle("all_255")[1].tolist() == [510]
    assert oracle("8x8x3_odd_m2")[1].tolist() == [201]
    assert oracle("split_even")[1].tolist() == [400, 240, 80]          # 49 low bytes: both middles high; 50: one each; 51: both low
    assert oracle("split_odd")[1].tolist() == [400, 80]
    assert oracle("1x1x1")[1].tolist() == [154] and oracle("one_bin_256x256x3")[1].tolist() == [262]
    thr, med = oracle("sigma_edges")
    m = [int(v) for v in med]
    assert thr[0].tolist() == [m[0] >> 1, m[0] >> 1]                                      # sigma 0: low = high = floor(median)
    assert thr[1].tolist() == [0, min(255, m[1])] and thr[2].tolist() == [0, min(255, m[2])]          # sigma 1, and the clamp to it
    thr, med = oracle("manual_slot")
    assert thr[1].tolist() == [THR_SENTINEL] * 2 and med[1] == MED_SENTINEL and thr[0, 1] > thr[0, 0] >= 0


def check_errors(lib, device):
    """Every I2I_ERR_BAD_ARG case leaves thr (and median2) as they were; n == 0 is a successful no-op."""
    img, sig = case("sigma_edges")
    bad = [dict(null="src"), dict(null="sigma_q16"), dict(null="thr"), dict(null="ws"), dict(params_null=True), dict(c=0), dict(c=5),
           dict(n=-1), dict(h=-1), dict(w=-3), dict(h=0), dict(w=0), dict(h=30000, w=30000, c=4),      # N = 3.6e9 > 2^31 - 1
           dict(thr_offset=2), dict(sigma_q16_offset=1), dict(median2_offset=2), dict(ws_offset=4)]
    for kw in bad:
        rc, thr, med, _ = raw_call(lib, device, img, sig, **kw)
        assert rc == -1, (kw, rc)                                                          # I2I_ERR_BAD_ARG
        assert lib.lib.i2i_last_error().decode().startswith("canny_auto_thr:"), kw
        assert bool((thr == THR_SENTINEL).all()) and bool((med == MED_SENTINEL).all()), kw
    rc, thr, med, _ = raw_call(lib, device, img, sig, n=0)
    assert rc == 0 and bool((thr == THR_SENTINEL).all()) and bool((med == MED_SENTINEL).all())
    f = lib.canny_auto_ws_bytes
    assert f(0) == 0 and f(-3) == 0 and f(1) >= 1024 and f(8) >= 8 * 1024 and f(8) % 16 == 0 and f(1030) >= 1030 * 1024


def check_struct(lib):
    from img2img_turbo_amd import _capi as K
    import batch_cases as bc
    assert lib.lib.i2i_sizeof_op() == C.sizeof(K.Op) == bc.PARENT_SIZEOF_OP
    assert C.sizeof(K.CannyAutoThrParams) == 56 <= C.sizeof(K.IgemmParams)
    assert lib.lib.i2i_abi_version() == K.ABI_VERSION == 14 and K.OP_CANNY_AUTO_THR == 24


def check_eager(lib, device):
    """image_ops.canny_auto_thresholds (scalar sigma, per-image sigma with a None entry) and canny_u8(low="auto") against the oracle's pairs
    fed to the per-image entry, bit for bit, at 64 x 64 x 3."""
    import pytest
    from img2img_turbo_amd import image_ops
    assert image_ops.sigma_to_q16(0.33) == S33 and image_ops.sigma_to_q16(0.0) == 0 and image_ops.sigma_to_q16(1.0) == 65536
    img = cc.smooth_noise(3, 64, 64, 3, seed=12)
    src = cc.to_dev(img, device)
    thr, med = image_ops.canny_auto_thresholds(src, lib=lib)
    want_thr, want_med = ar.auto_thresholds(img, [S33] * 3)
    assert thr.dtype == torch.int32 and thr.shape == (3, 2) and np.array_equal(thr.cpu().numpy(), want_thr)
    assert np.array_equal(as_u32(med), want_med)
    thr2, med2 = image_ops.canny_auto_thresholds(src, [0.25, None, 0.5], lib=lib)
    w2, m2 = ar.auto_thresholds(img, [16384, -1, 32768])
    assert np.array_equal(thr2.cpu().numpy(), w2) and np.array_equal(as_u32(med2), m2) and thr2[1].tolist() == [0, 0]
    lows, highs = [int(v) for v in want_thr[:, 0]], [int(v) for v in want_thr[:, 1]]
    auto = image_ops.canny_u8(src, low="auto", lib=lib)
    manual = image_ops.canny_u8(src, lows, highs, lib=lib)
    assert torch.equal(auto, manual) and auto.any() and not auto.all()
    assert np.array_equal(auto.cpu().numpy(), np.stack([canny_ref.canny(img[b], lows[b], highs[b], 3) for b in range(3)]))
    auto25 = image_ops.canny_u8(src, low="auto", sigma=[0.25, 0.33, 0.5], out_channels=1, lib=lib)
    w3, _ = ar.auto_thresholds(img, [16384, S33, 32768])
    assert torch.equal(auto25, image_ops.canny_u8(src, w3[:, 0].tolist(), w3[:, 1].tolist(), 1, lib=lib))
    for bad in (dict(low="otsu"), dict(low="auto", sigma=[0.3, None, 0.3]), dict(low="auto", sigma=1.5), dict(low="auto", sigma=[0.3, 0.3])):
        with pytest.raises(ValueError):
            image_ops.canny_u8(src, lib=lib, **bad)


def check_program_op(lib, device):
    """The op through i2i_run (capi.hip's dispatch) chained with the per-image Canny op, as a plan records the two."""
    from img2img_turbo_amd import _capi as K, ops as O
    img = cc.smooth_noise(2, 37, 53, 3, seed=13)
    src = cc.to_dev(img, device)
    n, h, w, c = src.shape
    sigma = torch.tensor([S33, 16384], dtype=torch.int32).to(device)
    thr = torch.zeros(n, 2, dtype=torch.int32, device=device)
    med = torch.zeros(n, dtype=torch.int32, device=device)
    ws_a = torch.empty(lib.canny_auto_ws_bytes(n), dtype=torch.uint8, device=device)
    dst = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=device)
    ws = torch.empty(lib.canny_ws_bytes(n, h, w), dtype=torch.uint8, device=device)
    prog = K.Program()
    prog.add(*_dt(O.canny_auto_thr(src, sigma, thr, ws_a, n=n, h=h, w=w, c=c, median2=med)), "auto_thr")
    prog.add(*_dt(O.canny_u8_batch(src, dst, ws, thr, n=n, h=h, w=w, c=c, out_c=3)), "canny")
    lib.run(prog.freeze(), torch.cuda.current_stream().cuda_stream if device != "cpu" else 0)
    if device != "cpu":
        torch.cuda.synchronize()
    want_thr, want_med = ar.auto_thresholds(img, [S33, 16384])
    assert np.array_equal(thr.cpu().numpy(), want_thr) and np.array_equal(as_u32(med), want_med)
    assert np.array_equal(dst.cpu().numpy(), np.stack([canny_ref.canny(img[b], int(want_thr[b, 0]), int(want_thr[b, 1]), 3) for b in range(n)]))


def _dt(op):
    from img2img_turbo_amd import _capi as K
    return op[0], K.F32, op[1]


# ---------------------------------------------------------------------------------------------------------------- the planned forward
B = 3
MIX = [(40, 90), "auto", ("auto", 0.25)]                    # one request with its own sliders, two automatic ones


def mixed_expect(img, entries=MIX, default=0.33):
    """Per image, what the respective single-mode call gives: the host's (low, high) pairs of a mixed batch."""
    from img2img_turbo_amd.image_ops import sigma_to_q16
    pairs = []
    for b, e in enumerate(entries):
        if e == "auto" or (isinstance(e, tuple) and e[0] == "auto"):
            s = sigma_to_q16(default if e == "auto" else e[1])
            pairs.append(ar.thresholds(ar.median2(img[b]), s))
        else:
            pairs.append((int(e[0]), int(e[1])))
    return pairs


def check_forward(lib, device, h, w):
    """forward_u8(canny="auto", return_edges=True) is the eager chain (canny_u8(low="auto") then forward_u8 of the edge maps) and returns
    the edge map and the thresholds; ("auto", sigma); a batch mixing automatic and manual entries on the same plan gives per image what the
    single-mode call gives; set_canny_sigma between two replays of ONE captured graph moves the thresholds; return_edges on a plain
    (low, high) plan.  The model replays a captured graph on the GPU and runs the program op by op on the emulator (use_graph)."""
    import pytest
    import randn_cases as rc
    from img2img_turbo_amd import image_ops
    model = rc.make_model(lib, device, False)
    graph = model.use_graph
    try:
        img, cap, eps = cc.pipeline_inputs(B, h, w)
        imgd, capd, epsd = cc.to_dev(img, device), cap.to(device), eps.to(device)
        kw = dict(caption_enc=capd, eps=epsd)
        # 1. automatic for the whole batch
        out, edges, thr = model.forward_u8(imgd, canny="auto", return_edges=True, **kw)
        plan = model._last_plan
        assert plan.canny == "auto" and plan.canny_auto and plan.canny_thr.shape == (B, 2) and plan.prog.labels[0] == "input.canny_auto_thr"
        want_thr, want_med = ar.auto_thresholds(img, [S33] * B)
        assert thr.dtype == torch.int32 and np.array_equal(thr.cpu().numpy(), want_thr)
        assert np.array_equal(as_u32(plan.canny_median2), want_med)
        eager = image_ops.canny_u8(imgd, low="auto", lib=lib)
        assert edges.shape == (B, h, w, 3) and torch.equal(edges, eager) and edges.any() and not edges.all()
        assert torch.equal(out, model.forward_u8(eager, **kw))
        assert torch.equal(out, model.forward_u8(imgd, canny="auto", **kw))                 # without the flag: the image alone
        # 2. another sigma: the same plan (and graph), other thresholds
        out25, edges25, thr25 = model.forward_u8(imgd, canny=("auto", 0.25), return_edges=True, **kw)
        assert model._last_plan is plan and np.array_equal(thr25.cpu().numpy(), ar.auto_thresholds(img, [16384] * B)[0])
        assert torch.equal(edges25, image_ops.canny_u8(imgd, low="auto", sigma=0.25, lib=lib))
        # 3. a mixed batch on the same plan: per image what the single-mode call gives
        outm, edgesm, thrm = model.forward_u8(imgd, canny=MIX, return_edges=True, **kw)
        pairs = mixed_expect(img)
        assert model._last_plan is plan and thrm.cpu().tolist() == [list(p) for p in pairs]
        assert plan.canny_sigma.cpu().tolist() == [-1, S33, 16384]
        assert torch.equal(edgesm[0], image_ops.canny_u8(imgd[0:1], 40, 90, lib=lib)[0])
        assert torch.equal(edgesm[1], edges[1]) and torch.equal(edgesm[2], edges25[2])
        assert torch.equal(outm, model.forward_u8(edgesm, **kw))
        # 4. one captured graph (or the program), the sigma moved between two runs: no re-capture, other thresholds
        g = plan.graph
        for sigma, q in ((0.5, 32768), ([0.1, None, 0.33], None)):
            plan.set_canny_sigma(sigma)
            plan.replay() if graph else plan.run()
            if q is not None:
                want = ar.auto_thresholds(img, [q] * B)[0]
            else:                                                                          # image 1 keeps the pair the previous run computed
                want = ar.auto_thresholds(img, [image_ops.sigma_to_q16(0.1), -1, S33], thr=ar.auto_thresholds(img, [32768] * B)[0])[0]
            assert np.array_equal(plan.canny_thr.cpu().numpy(), want), sigma
            assert plan.graph is g
        assert torch.equal(plan.canny_edges, image_ops.canny_u8(imgd, want[:, 0].tolist(), want[:, 1].tolist(), lib=lib))
        # 5. return_edges on a plan with hand-set thresholds: the same image, plus the edge map of the eager call
        plain = model.forward_u8(imgd, canny=(100, 200), **kw)
        plain2, e2 = model.forward_u8(imgd, canny=(100, 200), return_edges=True, **kw)
        assert model._last_plan is not plan and not model._last_plan.canny_auto
        assert torch.equal(plain, plain2) and torch.equal(e2, image_ops.canny_u8(imgd, 100, 200, lib=lib))
        with pytest.raises(ValueError):
            model.forward_u8(imgd, return_edges=True, **kw)
        with pytest.raises(ValueError):
            model.forward_u8(imgd, canny=["auto", (1, 2)], **kw)                            # 2 entries for a batch of 3
        with pytest.raises(ValueError):
            model.forward_u8(imgd, canny="otsu", **kw)
        return model, img, cap, eps
    except BaseException:
        model.release_plans()
        raise


# ---------------------------------------------------------------------------------------------------------------- BICUBIC tables
BICUBIC_SIZES = [((97, 61), (96, 56)), ((33, 47), (64, 64)), ((1280, 720), (512, 512))]      # (width, height) in -> out; the second is an upscale


def parent_lanczos_coeffs(in_size, out_size):
    """image_ops.lanczos_coeffs as it was before resample_coeffs existed (the regression reference of the LANCZOS tables)."""
    import math

    def sinc(x):
        if x == 0.0:
            return 1.0
        x = x * math.pi
        return math.sin(x) / x

    def lanczos(x):
        return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ww = 0.0
        for x in range(xmax):
            wt = lanczos((x + xmin - center + 0.5) * ss)
            kk[xx, x] = wt
            ww += wt
        if ww != 0.0:
            for x in range(xmax):
                kk[xx, x] /= ww
        bounds[xx] = (xmin, xmax)
    ik = np.where(kk < 0, (-0.5 + kk * (1 << 22)).astype(np.int64), (0.5 + kk * (1 << 22)).astype(np.int64)).astype(np.int32)
    return ksize, bounds, ik


TABLE_PAIRS = [(97, 96), (61, 56), (33, 64), (47, 64), (1280, 512), (720, 512), (5, 5), (1, 7), (300, 7)]


def check_tables(lib):
    """i2i_resample_tables == image_ops.resample_coeffs for both filters; the LANCZOS names return what they returned before."""
    import pytest
    from img2img_turbo_amd import _capi as K, image_ops
    for n_in, n_out in TABLE_PAIRS:
        for filt in ("bicubic", "lanczos"):
            ksize, bounds, coeffs = image_ops.resample_coeffs(n_in, n_out, filt)
            got_k, got_b, got_c = lib.resample_tables(filt, n_in, n_out)
            assert got_k == ksize and np.array_equal(got_b, bounds) and np.array_equal(got_c, coeffs), (filt, n_in, n_out)
            wide_k, wide_b, wide_c = lib.resample_tables(filt, n_in, n_out, ksize + 2)
            assert wide_k == ksize and np.array_equal(wide_b, bounds) and np.array_equal(wide_c[:, :ksize], coeffs) and not wide_c[:, ksize:].any()
        pk, pb, pc = parent_lanczos_coeffs(n_in, n_out)
        for k, b, c in (image_ops.lanczos_coeffs(n_in, n_out), lib.lanczos_tables(n_in, n_out), image_ops.resample_coeffs(n_in, n_out, "lanczos")):
            assert k == pk and np.array_equal(b, pb) and np.array_equal(c, pc), (n_in, n_out)
        bk = image_ops.resample_coeffs(n_in, n_out, "bicubic")[0]
        assert bk <= pk and bk == 2 * int(np.ceil(2.0 * max(n_in / n_out, 1.0))) + 1
    assert lib.lib.i2i_resample_ksize(7, 10, 10) == -1 and lib.lib.i2i_last_error().decode().startswith("resample_ksize:")
    with pytest.raises(K.I2IError):
        lib.resample_tables(2, 10, 10)
    with pytest.raises(ValueError):
        image_ops.resample_coeffs(10, 10, "nearest")


def check_bicubic(lib, device, sizes):
    """lanczos_resize_u8(..., resample="bicubic") equals Image.resize(size) of the installed Pillow (no filter argument: its default), bit
    for bit, for RGB and single-channel images; the ragged entry and forward_u8's keyword reach the same tables."""
    from PIL import Image
    from img2img_turbo_amd import image_ops
    (wi, hi), (wo, ho) = sizes
    rng = np.random.default_rng(wi + hi)
    for c, mode in ((3, "RGB"), (1, "L")):
        img = rng.integers(0, 256, (2, hi, wi, c), dtype=np.uint8)
        want = np.stack([np.asarray(Image.fromarray(im if c > 1 else im[..., 0], mode).resize((wo, ho))).reshape(ho, wo, c) for im in img])
        got = image_ops.lanczos_resize_u8(cc.to_dev(img, device), (wo, ho), lib, resample="bicubic")
        assert np.array_equal(got.cpu().numpy(), want), (sizes, c, int((got.cpu().numpy() != want).sum()))
        if c == 3:
            lanczos = image_ops.lanczos_resize_u8(cc.to_dev(img, device), (wo, ho), lib)
            assert not torch.equal(lanczos, got)                                          # the default filter did not move
            rag = image_ops.lanczos_resize_u8_ragged([cc.to_dev(img[0], device), cc.to_dev(img[1, :hi - 3], device)], (wo, ho), lib, resample="bicubic")
            assert np.array_equal(rag[0].cpu().numpy(), want[0])

"""Canny edge detection (i2i_canny_u8, csrc/resize.hip) on an MI355X: the cases of tests/test_canny_emu.py (shared through
tests/canny_cases.py), bit-exact against the CPU oracle tests/canny_ref.py, plus the captured-graph form of the pipeline and one timing
line."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import canny_cases as cc
import canny_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key,out_c", cc.SIZE_CASES)
def test_canny_sizes(gpu_lib, key, out_c):
    cc.check_sizes(gpu_lib, "cuda", key, out_c)


def test_canny_long_chain_across_tiles(gpu_lib):
    cc.check_snakes(gpu_lib, "cuda")


def test_canny_thresholds_and_dirty_workspace(gpu_lib):
    cc.check_thresholds(gpu_lib, "cuda")


def test_canny_abi(gpu_lib):
    cc.check_abi(gpu_lib, "cuda")


def test_canny_run_to_run_identical_on_a_busy_image(gpu_lib):
    """Many components merged across many tile edges by concurrently running workgroups: the result is the oracle's, every time."""
    img = cc.smooth_noise(2, 203, 331, 3, seed=9)
    want = canny_ref.canny_batch(img, 60, 120, 3)
    src = cc.to_dev(img, "cuda")
    from img2img_turbo_amd import image_ops
    for _ in range(5):
        got = image_ops.canny_u8(src, 60, 120, 3, lib=gpu_lib).cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())


def test_canny_pipeline_and_graph(gpu_lib):
    """photo -> LANCZOS resize -> Canny -> generator -> uint8 image on the device against the host twin (Pillow + the oracle); then the
    plan's program captured with i2i_graph_create and replayed twice with different "canny_thr" contents."""
    from img2img_turbo_amd import arch
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.synth import make_pix2pix_weights
    w = make_pix2pix_weights(arch.TINY_UNET, arch.TINY_VAE, seed=1234)
    model = Pix2Pix_Turbo(weights=w, device="cuda", dtype=torch.float32, lib=gpu_lib)
    img, cap, eps, outs = cc.check_pipeline(gpu_lib, "cuda", model)
    plan = [p for p in model._plans.values() if p.canny][0]
    from PIL import Image
    resized = np.stack([np.asarray(Image.fromarray(im, "RGB").resize((88, 72), Image.LANCZOS)) for im in img])
    plan.x_in.copy_(torch.from_numpy(resized))
    plan.ctx.copy_(cap.reshape(plan.ctx.shape))
    plan.eps.copy_(eps)
    g = gpu_lib.graph_create(plan.prog)
    try:
        for thr in ((40, 90), (100, 200)):
            plan.canny_thr.copy_(torch.tensor(thr, dtype=torch.int32))
            gpu_lib.graph_launch(g, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(plan.out.cpu(), outs[thr]), thr
    finally:
        gpu_lib.graph_destroy(g)
        model.release_plans()


def test_canny_timing_line(gpu_lib):
    """8 x 512 x 512 x 3 (the headline batch): correctness against the oracle on one slot, then 10 timed runs after a warm-up.  No gate:
    the parent has no device path to compare with; the oracle's time per image is printed beside it as a stand-in for a one-thread CPU
    Canny (numpy + scipy.ndimage.label, not OpenCV)."""
    from img2img_turbo_amd import image_ops
    img = cc.smooth_noise(8, 512, 512, 3, seed=3)
    src = cc.to_dev(img, "cuda")
    out = image_ops.canny_u8(src, 100, 200, 3, lib=gpu_lib)
    t0 = time.perf_counter()
    want0 = canny_ref.canny(img[0], 100, 200, 3)
    t_host = time.perf_counter() - t0
    assert np.array_equal(out[0].cpu().numpy(), want0)
    n, h, w, c = src.shape
    dst = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda")
    ws = torch.empty(gpu_lib.canny_ws_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    rc, _, _ = cc.raw_call(gpu_lib, "cuda", src, dst=dst, ws=ws)          # warm-up (synchronises)
    assert rc == 0 and torch.equal(dst, out)
    from img2img_turbo_amd import _capi as K
    p = K.CannyU8Params()
    p.src, p.dst, p.ws, p.thr_dev = src.data_ptr(), dst.data_ptr(), ws.data_ptr(), 0
    p.n, p.h, p.w, p.c, p.out_c, p.low, p.high = n, h, w, c, 3, 100, 200
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
    ev[0].record()
    for i in range(10):
        gpu_lib.check(gpu_lib.lib.i2i_canny_u8(C.addressof(p), 0, stream))
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(10))
    print("[canny] 8x512x512x3 -> 3 channels: median %.3f ms, min %.3f ms, max %.3f ms over 10 runs (5 launches each); "
          "host oracle (numpy + scipy, one image) %.1f ms -> %.0f ms for the batch on one thread"
          % (ms[5], ms[0], ms[-1], t_host * 1e3, t_host * 8e3))
    assert torch.equal(dst, out)

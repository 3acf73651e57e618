"""Automatic per-image Canny thresholds (i2i_canny_auto_thr, csrc/resize.hip) on an MI355X: the cases of tests/test_canny_auto_emu.py
(shared through tests/canny_auto_cases.py), bit-exact against the CPU oracle tests/canny_auto_ref.py, the planned forward replayed as a
captured graph, Pillow's BICUBIC tables through the resize kernels, and one timing line against the host route the op replaces."""
import time

import numpy as np
import pytest
import torch

import canny_auto_cases as ac
import canny_auto_ref as ar
import canny_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_canny_auto_cases(gpu_lib, name):
    ac.check_case(gpu_lib, "cuda", name)


def test_canny_auto_errors(gpu_lib):
    ac.check_errors(gpu_lib, "cuda")


def test_canny_auto_abi_is_additive(gpu_lib):
    ac.check_struct(gpu_lib)


def test_canny_auto_eager(gpu_lib):
    ac.check_eager(gpu_lib, "cuda")


def test_canny_auto_program_op(gpu_lib):
    ac.check_program_op(gpu_lib, "cuda")


def test_canny_auto_forward_and_graph(gpu_lib):
    """The model class at 72 x 88 through the captured graph: automatic, ("auto", sigma), a mixed batch, set_canny_sigma between replays
    without re-capture, return_edges on a hand-set plan."""
    model, _, _, _ = ac.check_forward(gpu_lib, "cuda", 72, 88)
    assert model.use_graph
    model.release_plans()


def test_resample_tables(gpu_lib):
    ac.check_tables(gpu_lib)


@pytest.mark.parametrize("sizes", ac.BICUBIC_SIZES)
def test_bicubic_resize_matches_pillow_default(gpu_lib, sizes):
    ac.check_bicubic(gpu_lib, "cuda", sizes)


def test_canny_auto_timing_line(gpu_lib):
    """8 x 512 x 512 x 3 images of natural statistics (low-pass filtered noise): the three launches as a captured graph against the host
    route they replace -- download, np.median per image, two fills per image, with the synchronisation --, median of 10 after a warm-up.
    The only assertion: the device route is faster than the host route measured in the same process."""
    from img2img_turbo_amd import _capi as K, ops as O
    img = cc.smooth_noise(8, 512, 512, 3, seed=21)
    src = cc.to_dev(img, "cuda")
    n, h, w, c = src.shape
    sigma = torch.full((n,), ac.S33, dtype=torch.int32, device="cuda")
    thr = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    med = torch.zeros(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(gpu_lib.canny_auto_ws_bytes(n), dtype=torch.uint8, device="cuda")
    prog = K.Program()
    opcode, params = O.canny_auto_thr(src, sigma, thr, ws, n=n, h=h, w=w, c=c, median2=med)
    prog.add(opcode, K.F32, params, "auto_thr")
    g = gpu_lib.graph_create(prog.freeze())
    stream = torch.cuda.current_stream().cuda_stream
    try:
        gpu_lib.graph_launch(g, stream)                     # warm-up
        torch.cuda.synchronize()
        want_thr, want_med = ar.auto_thresholds(img, [ac.S33] * n)
        assert np.array_equal(thr.cpu().numpy(), want_thr) and np.array_equal(ac.as_u32(med), want_med)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
        ev[0].record()
        for i in range(10):
            gpu_lib.graph_launch(g, stream)
            ev[i + 1].record()
        torch.cuda.synchronize()
        dev_ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(10))
    finally:
        gpu_lib.graph_destroy(g)
    thr_host = torch.zeros(n, 2, dtype=torch.int32, device="cuda")

    def host_route():
        t0 = time.perf_counter()
        a = src.cpu().numpy()
        for b in range(n):
            m = float(np.median(a[b]))
            thr_host[b, 0:1].fill_(int(max(0, (1.0 - 0.33) * m)))
            thr_host[b, 1:2].fill_(int(min(255, (1.0 + 0.33) * m)))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    host_route()                                            # warm-up
    host_ms = sorted(host_route() for _ in range(10))
    assert int((thr_host.cpu() - thr.cpu()).abs().max()) <= 1          # (the float form of the rule: within 1 of the contract)
    print("[canny_auto] 8x512x512x3 thresholds: device (3 launches, captured graph) median %.3f ms, min %.3f, max %.3f; host route "
          "(.cpu(), np.median per image, 2 fills per image, synchronise) median %.2f ms, min %.2f, max %.2f"
          % (dev_ms[5], dev_ms[0], dev_ms[-1], host_ms[5], host_ms[0], host_ms[-1]))
    assert dev_ms[5] < host_ms[5], (dev_ms[5], host_ms[5])

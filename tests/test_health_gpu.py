"""Numerical health scan on an MI355X: the cases of tests/health_cases.py bit-equal to tests/health_ref.py, the planned forward with
health= (eager + graph replays), the poisoned fp16 / bf16 pair, every label of the SD-Turbo architecture, and the timing line."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import health_cases as hc

pytestmark = pytest.mark.gpu
IDS = ["f32", "bf16", "f16"]
DEV = "cuda:0"


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_scan_small_views(gpu_lib, dtype):
    hc.check_small(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_scan_classes(gpu_lib, dtype):
    hc.check_classes(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_scan_strides(gpu_lib, dtype):
    hc.check_strides(gpu_lib, DEV, dtype)


def test_scan_refusals(gpu_lib):
    hc.check_refusals(gpu_lib, DEV)


def test_forward_stages_eager_and_graph(gpu_lib):
    """health="stages": one eager run and two graph replays accumulate runs == 3; the image is the one of a model without scans."""
    x, cap, eps = hc.tiny_inputs(DEV, 2, 72, 88)
    dt = torch.bfloat16
    plain = hc.make_model(gpu_lib, DEV, dt, None)
    want = plain(x, caption_enc=cap, eps=eps)
    model = hc.make_model(gpu_lib, DEV, dt, "stages")
    plan = model.get_plan(2, 72, 88)
    model.stage(plan, x, cap, eps)
    plan.run()
    eager = plan.out.clone()
    plan.replay()
    plan.replay()
    model._last_plan = plan
    assert torch.equal(eager, want) and torch.equal(plan.out, want)
    rep = model.health_report()
    assert [d["label"] for d in rep] == hc.stage_names(model.weights)
    one = None
    for d, (t, rows, cols, _) in zip(rep, plan.health_taps):
        assert d["runs"] == 3 and d["elements"] == 3 * rows * cols and d["max_abs"] > 0, d
        assert d["n_nan"] == d["n_pos_inf"] == d["n_neg_inf"] == 0, d
    assert model.health_first_bad() is None
    model.health_reset()
    assert not hc.records(plan).any()
    # and through forward(): same image, one more run on the zeroed records
    assert torch.equal(model(x, caption_enc=cap, eps=eps), want)
    assert all(d["runs"] == 1 for d in model.health_report())
    plain.release_plans()
    model.release_plans()


def test_poison(gpu_lib):
    hc.check_poison(gpu_lib, DEV, 72, 88)


def test_sd_turbo_labels(gpu_lib):
    """SD-Turbo architecture, batch 1, 64 x 64, health="all": every real label gets a record with one run and its element count."""
    from test_e2e_gpu import gw, sd_weights
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from oracle import SD_TURBO_UNET
    mw = sd_weights("pix2pix", seed=1234 + 1)
    model = Pix2Pix_Turbo(weights=gw(mw), device=DEV, dtype=torch.bfloat16, lib=gpu_lib, health="all")
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    cap = torch.randn(1, 77, SD_TURBO_UNET.cross_attention_dim, generator=g).to(DEV)
    eps = torch.randn(1, 4, 8, 8, generator=g).to(DEV)
    out = model(x, caption_enc=cap, eps=eps)
    plan = model._last_plan
    rep = model.health_report()
    stages = hc.stage_names(model.weights)
    labels = [d["label"] for d in rep]
    assert [l for l in labels if l in stages] == stages and set(plan.taps) <= set(labels)
    for d, (t, rows, cols, _) in zip(rep, plan.health_taps):
        assert d["runs"] == 1 and d["elements"] == rows * cols, d
    bad = model.health_first_bad()
    print("[health] SD-Turbo architecture, synthetic weights, bf16, 64 x 64: %d taps, %d scanned bytes, first non-finite: %s; largest max_abs %.4g at %s"
          % (len(rep), sum(r * c * t.element_size() for t, r, c, _ in plan.health_taps), bad and bad["label"],
             max(d["max_abs"] for d in rep), max(rep, key=lambda d: d["max_abs"])["label"]))
    assert bad is None and torch.isfinite(out.float()).all()
    model.release_plans()


def test_health_timing_line(gpu_lib):
    """Prints (does not gate): i2i_scan over one 8 x 512 x 512 x 128 bf16 tensor, median of 10 after a warm-up, and i2i_calib_stream over the
    same byte count in the same process -- bytes per second, the copy counted with its read and its write."""
    from img2img_turbo_amd import _capi as K
    n = 8 * 512 * 512 * 128
    x = (torch.rand(n, device=DEV) - 0.5).to(torch.bfloat16)
    y = torch.empty_like(x)
    rec = hc.new_rec(DEV)
    p = K.ScanParams()
    p.x, p.rows, p.cols, p.ld, p.limit, p.rec = x.data_ptr(), 8 * 512 * 512, 128, 128, 1.0e30, rec.data_ptr()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts))
    t_scan = timed(lambda: gpu_lib.check(gpu_lib.lib.i2i_scan(C.addressof(p), K.BF16, s)))
    t_copy = timed(lambda: gpu_lib.check(gpu_lib.lib.i2i_calib_stream(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_size_t(2 * n), s)))
    got = hc.read_rec(rec)
    assert got[0] == 11 and got[6] == 11 * n and got[1:5].tolist() == [0, 0, 0, 0]
    print("[health] scan %.3f ms = %.2f TB/s read; copy stream %.3f ms = %.2f TB/s (read + write) over %d MiB"
          % (t_scan * 1e3, 2 * n / t_scan / 1e12, t_copy * 1e3, 4 * n / t_copy / 1e12, 2 * n >> 20))

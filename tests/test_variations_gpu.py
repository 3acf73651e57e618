"""Variations on an MI355X: the cases of tests/variations_cases.py (the emulator runs them in tests/test_variations_emu.py) -- i2i_repeat against
torch.repeat_interleave bit for bit, ForwardPlan / Pix2Pix_Turbo with ``variations=V`` against the oracle, seeds through a captured graph, one
plan-file round trip -- and the timing line."""
import numpy as np
import pytest
import torch

import variations_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_struct_size(gpu_lib):
    vc.check_struct_size(gpu_lib)


@pytest.mark.parametrize("name", list(vc.REPEAT_CASES))
def test_repeat(gpu_lib, name):
    vc.check_repeat(gpu_lib, DEV, name)


def test_repeat_errors(gpu_lib):
    vc.check_repeat_errors(gpu_lib, DEV)


def test_encoder_runs_once(gpu_lib):
    vc.check_encoder_once(gpu_lib, DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("stochastic", [False, True], ids=["deterministic", "twinconv_r0.4"])
@pytest.mark.parametrize("shape", vc.PARITY_SHAPES, ids=lambda s: "B%dV%d_%dx%d" % s)
def test_parity_with_the_oracle(gpu_lib, shape, stochastic, dtype):
    vc.check_parity(gpu_lib, DEV, shape, stochastic, dtype)


def test_v1_is_todays_forward(gpu_lib):
    vc.check_v1(gpu_lib, DEV)


@pytest.mark.parametrize("stochastic", [False, True], ids=["deterministic", "stochastic"])
def test_seeds_and_captured_graph(gpu_lib, stochastic):
    vc.check_seeds(gpu_lib, DEV, stochastic, graph=True, h=72, w=88)


def test_forward_u8_canny(gpu_lib):
    vc.check_u8_canny(gpu_lib, DEV)


def test_plan_file_round_trip(gpu_lib, tmp_path):
    vc.check_plan_file(gpu_lib, DEV, tmp_path, h=72, w=88)


def test_per_image_health_raises(gpu_lib):
    vc.check_health_per_image_raises(gpu_lib, DEV)


def test_variations_timing_line(gpu_lib):
    """Prints (does not gate): SD-Turbo-size synthetic weights, bf16, 512 x 512, B = 2 inputs x V = 4 variations as a captured graph, against the
    captured graph of the plain batch-8 plan fed the repeated inputs (the program a caller had to run before) -- blocks of 10 replays
    interleaved, the median per arm after a warm-up -- and the repeat launch's own time from a per-op timed run.  Asserted: nothing about
    time; the images are finite, and the largest difference between the two arms is printed (the encoder runs at batch 2 in one and 8 in
    the other, so the contraction kernels may choose other tiles: not bit-equal by contract)."""
    from oracle import SD_TURBO_UNET, SD_TURBO_VAE
    from oracle.synth import make_pix2pix_weights
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    B, V, S = 2, 4, 512
    mw = make_pix2pix_weights(SD_TURBO_UNET, SD_TURBO_VAE)
    model = Pix2Pix_Turbo(weights=vc.gw(mw), device=DEV, dtype=torch.bfloat16)
    try:
        g = torch.Generator().manual_seed(3)
        x = (torch.rand(B, 1, S, S, generator=g) < 0.08).float().expand(B, 3, S, S).contiguous().to(DEV)
        cap = torch.randn(1, 77, SD_TURBO_UNET.cross_attention_dim, generator=g).to(DEV)
        eps = torch.randn(B * V, 4, S // 8, S // 8, generator=g).to(DEV)
        pv = model.get_plan(B, S, S, variations=V)
        p8 = model.get_plan(B * V, S, S)
        model.stage(pv, x, cap, eps)
        model.stage(p8, x.repeat_interleave(V, 0), cap, eps)
        for p in (pv, p8):
            p.replay()                                    # capture + warm-up
            p.replay()
        torch.cuda.synchronize()

        def block(p, n=10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                p.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / n

        tv, t8 = [], []
        for _ in range(10):                               # interleaved blocks: drift of the box lands on both arms
            tv.append(block(pv))
            t8.append(block(p8))
        mv, m8 = float(np.median(tv)), float(np.median(t8))
        ms = pv.run_timed()
        i_rep = pv.prog.labels.index("variations.repeat")
        enc = lambda p, t: sum(v for v, l in zip(t, p.prog.labels) if l.startswith(("input.", "encoder.")))
        ms8 = p8.run_timed()
        rep_bytes = pv.op_bytes[i_rep]
        print("[variations] B=%d x V=%d, %dx%d bf16, captured graphs, median of 10 interleaved blocks of 10 replays: variations plan %.3f ms "
              "(%.3f .. %.3f), plain batch-%d plan on repeated inputs %.3f ms (%.3f .. %.3f): saving %.3f ms = %.1f %%; per-op timed run: "
              "repeat launch %.4f ms (%.0f MiB read + written = %.2f TB/s), input + encoder ops %.3f ms at batch %d against %.3f ms at batch %d; "
              "%d ops against %d"
              % (B, V, S, S, mv, min(tv), max(tv), B * V, m8, min(t8), max(t8), m8 - mv, 100.0 * (m8 - mv) / m8, ms[i_rep], rep_bytes / 2 ** 20,
                 rep_bytes / max(ms[i_rep], 1e-6) / 1e9, enc(pv, ms), B, enc(p8, ms8), B * V, pv.prog.n, p8.prog.n))
        err = (pv.out.float() - p8.out.float()).abs().max().item()
        print("[variations] max-abs difference between the two arms' images: %.3e" % err)
        assert pv.out.shape == p8.out.shape == (B * V, 3, S, S) and bool(torch.isfinite(pv.out.float()).all()) and err == err
    finally:
        model.release_plans()

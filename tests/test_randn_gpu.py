"""Seeded Gaussian noise on the device (i2i_randn, csrc/elementwise.hip; img2img_turbo_amd/rng.py) on an MI355X: the cases of
tests/test_randn_emu.py (shared through tests/randn_cases.py) against the CPU oracle tests/randn_ref.py, plus the captured-graph form of
the pipeline, the plan-file round trip and one timing line."""
import ctypes as C

import numpy as np
import pytest
import torch

import randn_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", rc.SIZES + [rc.BIG])
def test_randn_raw(gpu_lib, n):
    rc.check_raw(gpu_lib, "cuda", n)


def test_randn_device_state_equals_immediates(gpu_lib):
    rc.check_state_form(gpu_lib, "cuda")


@pytest.mark.parametrize("n", rc.SIZES + [rc.BIG])
def test_randn_normal(gpu_lib, n):
    worst = rc.normal_errors(gpu_lib, "cuda", n)
    print("[randn] MI355X, n = %d: max |err| / rad = %.3g (bound %.3g)" % (n, worst, rc.TOL))


def test_randn_statistics(gpu_lib):
    rc.check_statistics(gpu_lib, "cuda")


def test_randn_state_and_advance(gpu_lib):
    rc.check_advance(gpu_lib, "cuda")


def test_randn_abi(gpu_lib):
    rc.check_abi(gpu_lib, "cuda")


def test_randn_module(gpu_lib):
    rc.check_module(gpu_lib, "cuda")


@pytest.mark.parametrize("stochastic", [False, True])
def test_randn_pipeline_and_graph(gpu_lib, stochastic):
    """The pipeline checks, then the rng plan's program captured with i2i_graph_create: set_seed(3) and three launches draw steps 0, 1, 2
    without the host; writing the state back to step 0 reproduces launch 0's image bit for bit."""
    from img2img_turbo_amd import rng
    model, plan, _ = rc.check_pipeline(gpu_lib, "cuda", stochastic)
    try:
        plan._prepare()                                   # (this plan's r on the shared weights)
        g = gpu_lib.graph_create(plan.prog)
        try:
            stream = torch.cuda.current_stream().cuda_stream
            plan.set_seed(3)
            outs = []
            for k in range(3):
                gpu_lib.graph_launch(g, stream)
                torch.cuda.synchronize()
                assert torch.equal(plan.eps, rng.randn(plan.eps.shape, 3, k, stream=0, lib=gpu_lib)), k
                if stochastic:
                    assert torch.equal(plan.noise, rng.randn(plan.noise.shape, 3, k, stream=2, lib=gpu_lib)), k
                assert rc.read_state(plan.rng_state)[:3] == [3, 0, k + 1]
                outs.append(plan.out.clone())
            assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
            plan.set_seed(3, 0)
            gpu_lib.graph_launch(g, stream)
            torch.cuda.synchronize()
            assert torch.equal(plan.out, outs[0]) and rc.read_state(plan.rng_state)[:3] == [3, 0, 1]
        finally:
            gpu_lib.graph_destroy(g)
    finally:
        model.release_plans()


def test_randn_plan_file(gpu_lib, tmp_path):
    """The plan-file round trip once, eager: export with a seed, load through i2i_plan_load, write another seed, run."""
    from img2img_turbo_amd import arch, plan_file, rng
    model = rc.make_model(gpu_lib, "cuda", False)
    try:
        x, cap = rc.pipeline_inputs(1, "cuda")
        plan = model.get_plan(1, rc.H, rc.W, rng=True)
        plan.set_seed(11)
        info = plan_file.export_plan(plan, str(tmp_path / "seeded.i2iplan"))
        assert info["io"]["seed"] == 16
        want = model.forward(x, caption_enc=cap, seed=12)
        eps = plan.eps.cpu()
        h = gpu_lib.plan_load(str(tmp_path / "seeded.i2iplan"))
        try:
            assert gpu_lib.plan_io(h, "seed")[1] == 16
            assert rc.read_state(gpu_lib.plan_read(h, "seed", torch.zeros(4, dtype=torch.int32))) == [11, 0, 0, 0]
            gpu_lib.plan_write(h, "x", x.cpu())
            gpu_lib.plan_write(h, "ctx", cap.cpu())
            gpu_lib.plan_write(h, "seed", rc.state_tensor(rng.pack_state(12), "cpu"))
            gpu_lib.plan_run(h, torch.cuda.current_stream().cuda_stream)
            assert torch.equal(gpu_lib.plan_read(h, "out", torch.zeros(1, 3, rc.H, rc.W)), want.cpu())
            assert torch.equal(gpu_lib.plan_read(h, "eps", torch.zeros(1, 4, rc.H // 8, rc.W // 8)), eps)
            assert rc.read_state(gpu_lib.plan_read(h, "seed", torch.zeros(4, dtype=torch.int32))) == [12, 0, 1, 0]
        finally:
            gpu_lib.plan_destroy(h)
    finally:
        model.release_plans()


def test_randn_timing_line(gpu_lib):
    """[8, 4, 64, 64] (the headline batch's latent): ten fills after a warm-up, beside the path it replaces -- torch.randn of that shape plus
    copy_ into a preallocated buffer -- timed the same way.  Print only, no gate."""
    from img2img_turbo_amd import _capi as K
    shape = (8, 4, 64, 64)
    dst = torch.empty(shape, dtype=torch.float32, device="cuda")
    p = K.RandnParams()
    p.dst, p.n, p.state, p.seed, p.step, p.stream_id, p.kind = dst.data_ptr(), dst.numel(), 0, 42, 0, 0, K.RANDN_NORMAL
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ours():
        gpu_lib.check(gpu_lib.lib.i2i_randn(C.addressof(p), 0, stream))

    def parent():
        dst.copy_(torch.randn(shape, device="cuda", dtype=torch.float32))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
        ev[0].record()
        for i in range(10):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(10))
    t_parent, t_ours = timed(parent), timed(ours)
    want, rad = rc.want_normal(dst.numel(), 42, 0, 0)
    got = dst.cpu().numpy().reshape(-1).astype(np.float64)
    assert (np.abs(got - want) <= rad * rc.TOL).all()
    print("[randn] 8x4x64x64 fp32: i2i_randn median %.4f ms (min %.4f, max %.4f); torch.randn + copy_ median %.4f ms (min %.4f, max %.4f); 10 runs each"
          % (t_ours[5], t_ours[0], t_ours[-1], t_parent[5], t_parent[0], t_parent[-1]))

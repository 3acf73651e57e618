"""Per-image request parameters of a batch on an MI355X: the cases of tests/test_batch_emu.py (shared through tests/batch_cases.py) --
i2i_randn_batch and i2i_canny_u8_batch against the single-image ops on the same library and against the CPU oracles -- plus the captured-graph
form of the per-image forward, the plan-file round trip and one timing line."""

import pytest
import torch

import batch_cases as bc
import randn_cases as rc

pytestmark = pytest.mark.gpu


def test_batch_abi_is_additive(gpu_lib):
    bc.check_struct_size(gpu_lib)


@pytest.mark.parametrize("per_image", bc.SIZES + [bc.big_size()])
def test_randn_batch_raw(gpu_lib, per_image):
    bc.check_raw(gpu_lib, "cuda", per_image)


@pytest.mark.parametrize("per_image", bc.SIZES + [bc.big_size()])
def test_randn_batch_normal(gpu_lib, per_image):
    """Bit-equal to i2i_randn on the same library (whose distance to the fp64 oracle tests/test_randn_gpu.py asserts)."""
    bc.check_normal(gpu_lib, "cuda", per_image, oracle=False)


def test_randn_batch_advance(gpu_lib):
    bc.check_advance(gpu_lib, "cuda")


def test_randn_batch_errors(gpu_lib):
    bc.check_errors(gpu_lib, "cuda")


def test_randn_batch_module(gpu_lib):
    bc.check_module(gpu_lib, "cuda")


def test_canny_batch(gpu_lib):
    bc.check_canny(gpu_lib, "cuda")


@pytest.mark.parametrize("stochastic", [False, True])
def test_batch_forward_and_graph(gpu_lib, stochastic):
    """The forward checks with the three replays made by a hipGraph captured from the per-image plan's program (i2i_graph_create)."""
    graphs = []

    def replay(plan):
        if not graphs:
            graphs.append(gpu_lib.graph_create(plan.prog))
        gpu_lib.graph_launch(graphs[0], torch.cuda.current_stream().cuda_stream)

    model = None
    try:
        model, _ = bc.check_forward(gpu_lib, "cuda", stochastic, replay=replay)
        assert len(graphs) == 1
    finally:
        torch.cuda.synchronize()
        for g in graphs:
            gpu_lib.graph_destroy(g)
        if model is not None:
            model.release_plans()


def test_batch_forward_eager_replays(gpu_lib):
    """The same three replays through plan.run() (i2i_run), deterministic model."""
    model, _ = bc.check_forward(gpu_lib, "cuda", False)
    model.release_plans()


def test_batch_forward_canny(gpu_lib):
    bc.check_forward_canny(gpu_lib, "cuda")


def test_batch_plan_file(gpu_lib, tmp_path):
    """Export the B = 3 per-image plan, load it through i2i_plan_load, write a 48-byte "seed", run; then a scalar-seed plan file of the same
    model, which still loads and runs."""
    from img2img_turbo_amd import plan_file, rng
    model = rc.make_model(gpu_lib, "cuda", False)
    try:
        x, cap = rc.pipeline_inputs(bc.B, "cuda")
        plan = model.get_plan(bc.B, rc.H, rc.W, rng="per_image")
        bc.check_plan_file(gpu_lib, "cuda", tmp_path, model, plan, x, cap, bc.FWD_SEEDS)
        flat = model.get_plan(bc.B, rc.H, rc.W, rng=True)
        flat.set_seed(9)
        spath = str(tmp_path / "scalar.i2iplan")
        assert plan_file.export_plan(flat, spath)["io"]["seed"] == 16
        want = model.forward(x, caption_enc=cap, seed=9).cpu()
        h = gpu_lib.plan_load(spath)
        try:
            gpu_lib.plan_write(h, "x", x.cpu())
            gpu_lib.plan_write(h, "ctx", cap.cpu())
            gpu_lib.plan_run(h, torch.cuda.current_stream().cuda_stream)
            assert torch.equal(gpu_lib.plan_read(h, "out", torch.zeros_like(want)), want)
            assert torch.equal(gpu_lib.plan_read(h, "eps", torch.zeros(bc.B, 4, rc.H // 8, rc.W // 8)),
                               rng.randn((bc.B, 4, rc.H // 8, rc.W // 8), 9, 0, lib=gpu_lib).cpu())
        finally:
            gpu_lib.plan_destroy(h)
    finally:
        model.release_plans()


def test_randn_batch_timing_line(gpu_lib):
    """[8, 4, 64, 64] (the headline batch's latent), one state per image: ONE i2i_randn_batch launch beside what a host has to do for the same
    bits without it -- eight i2i_randn launches on the eight slices, each from its own 16-byte state.  Both as a captured hipGraph
    (i2i_graph_create), 20 warm-up replays, then the median of 200 timed replays each, interleaved in blocks of 20 so that a clock change
    hits both.  Print only, no gate."""
    from img2img_turbo_amd import _capi as K, ops as O, rng
    shape = (8, 4, 64, 64)
    seeds = list(range(100, 108))
    a = torch.zeros(shape, dtype=torch.float32, device="cuda")
    b = torch.zeros(shape, dtype=torch.float32, device="cuda")
    st = rng.states_tensor(seeds, 0, "cuda")
    one, eight = K.Program(), K.Program()
    one.add(*rc._op(O.randn_batch(a, st, batch=8, stream_id=0)), "randn_batch")
    for i in range(8):
        eight.add(*rc._op(O.randn(b[i], state=st[i], stream_id=0)), "randn %d" % i)
    one.freeze()
    eight.freeze()
    stream = torch.cuda.current_stream().cuda_stream
    g_one, g_eight = gpu_lib.graph_create(one), gpu_lib.graph_create(eight)
    try:
        times = {id(g_one): [], id(g_eight): []}
        for g in (g_one, g_eight):
            for _ in range(20):
                gpu_lib.graph_launch(g, stream)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))          # the same bits
        for _ in range(10):
            for g in (g_one, g_eight):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
                ev[0].record()
                for i in range(20):
                    gpu_lib.graph_launch(g, stream)
                    ev[i + 1].record()
                torch.cuda.synchronize()
                times[id(g)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(20)]
        t1, t8 = sorted(times[id(g_one)]), sorted(times[id(g_eight)])
        print("[randn_batch] 8x4x64x64 fp32, per-image states, hipGraph replays: 1 x i2i_randn_batch median %.4f ms (min %.4f, p90 %.4f); "
              "8 x i2i_randn median %.4f ms (min %.4f, p90 %.4f); 200 replays each"
              % (t1[100], t1[0], t1[180], t8[100], t8[0], t8[180]))
    finally:
        torch.cuda.synchronize()
        gpu_lib.graph_destroy(g_one)
        gpu_lib.graph_destroy(g_eight)

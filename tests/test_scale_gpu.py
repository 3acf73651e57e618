"""The LoRA scale as device state for every host, on the MI355X: TwinConv fold kernel, grouped merge (also captured in a graph), the
scale program of a live_scale model and the plan-file round trip with i2i_plan_set_scale (tests/scale_cases.py has the cases)."""
import numpy as np
import pytest
import torch

import scale_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 64, 64


@pytest.mark.parametrize("dt", [S.F32, S.BF16, S.F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", S.TWIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_twin_fold_against_fp64(gpu_lib, shape, dt):
    worst = S.check_twin(gpu_lib, DEV, shape, dt)
    print("[twin_fold] %s dtype %d: worst %s = %.3f" % (shape, dt, "err / bound" if dt == S.F32 else "steps from the exact rounding", worst))


def test_twin_fold_abi(gpu_lib):
    S.check_twin_abi(gpu_lib, DEV)


@pytest.mark.parametrize("dt", [S.F32, S.BF16, S.F16], ids=["f32", "bf16", "f16"])
def test_grouped_merge_is_six_per_layer_merges(gpu_lib, dt):
    S.check_group(gpu_lib, DEV, dt)


def test_grouped_merge_abi(gpu_lib):
    S.check_group_abi(gpu_lib, DEV)


def test_grouped_merge_captured_in_a_graph(gpu_lib):
    """The group launch recorded by torch.cuda.graph and replayed twice: the second replay reads the rewritten (r, gamma)."""
    s = S.GroupSetup(DEV, S.BF16)
    g = gpu_lib.merge_group_create(s.layers, S.BF16)
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gpu_lib.merge_group_run(g, torch.cuda.current_stream().cuda_stream)
        s.wipe()                                        # whatever the capture did or did not execute
        graph.replay()
        first = s.compare(gpu_lib, "first replay")
        s.wipe()
        s.set_rg(S.GROUP_RG[1])
        graph.replay()
        second = s.compare(gpu_lib, "second replay")
        assert not np.array_equal(first, second)
        del graph
    finally:
        gpu_lib.merge_group_destroy(g)


def test_live_scale_equals_the_per_layer_path(gpu_lib):
    S.check_live_equals_per_layer(gpu_lib, DEV, H, W)


def test_plan_file_set_scale_round_trip(gpu_lib, tmp_path):
    S.check_plan_round_trip(gpu_lib, DEV, tmp_path, H, W)

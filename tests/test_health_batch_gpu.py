"""Per-image health on an MI355X: the cases of tests/health_batch_cases.py bit-equal to tests/health_ref.py per image, the verdict, the planned
forward with health_per_image (eager + graph replays, one bad request among three), and the timing line."""
import ctypes as C

import numpy as np
import pytest
import torch

import health_batch_cases as bc
import health_cases as hc

pytestmark = pytest.mark.gpu
IDS = ["f32", "bf16", "f16"]
DEV = "cuda:0"


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_misaligned_image_starts(gpu_lib, dtype):
    bc.check_misaligned(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_more_than_one_workgroup_per_image(gpu_lib, dtype):
    bc.check_multi_wg(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_second_pass_of_an_image_share(gpu_lib, dtype):
    bc.check_grid_pass(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_strided_views(gpu_lib, dtype):
    bc.check_strided(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_boundaries(gpu_lib, dtype):
    bc.check_boundaries(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_accumulation_and_neighbours(gpu_lib, dtype):
    bc.check_accumulate(gpu_lib, DEV, dtype)


def test_refusals(gpu_lib):
    bc.check_refusals(gpu_lib, DEV)


def test_verdict(gpu_lib):
    bc.check_verdict(gpu_lib, DEV)


def test_abi(gpu_lib):
    from img2img_turbo_amd import _capi as K
    assert gpu_lib.lib.i2i_abi_version() == 14 and gpu_lib.lib.i2i_sizeof_op() == C.sizeof(K.Op) == 368


def test_forward_clean(gpu_lib):
    bc.check_forward_clean(gpu_lib, DEV)


def test_forward_one_bad_request(gpu_lib):
    bc.check_forward_one_bad(gpu_lib, DEV)


def test_default_unchanged(gpu_lib):
    bc.check_default_unchanged(gpu_lib, DEV)


def test_health_batch_timing_line(gpu_lib):
    """Prints (does not gate): i2i_scan_batch over [8, 64, 64, 320] bf16 as a one-op hipGraph, median of 10 replays after a warm-up, beside
    i2i_scan over the same tensor measured the same way -- both read the same bytes once.  The records are checked all the same."""
    from img2img_turbo_amd import _capi as K
    from img2img_turbo_amd import ops as O
    images, rows, cols = 8, 64 * 64, 320
    x = (torch.rand(images * rows * cols, device=DEV) - 0.5).to(torch.bfloat16)
    rec_b = torch.zeros(images, 8, dtype=torch.int64, device=DEV)
    rec_w = hc.new_rec(DEV)
    assert rec_b.data_ptr() % 64 == 0
    stream = torch.cuda.current_stream().cuda_stream

    def timed(op):
        prog = K.Program()
        prog.add(op[0], K.BF16, op[1], "timing")
        prog.freeze()
        gpu_lib.run(prog, stream)                 # the warm-up, eager
        graph = gpu_lib.graph_create(prog)
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gpu_lib.graph_launch(graph, stream)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        gpu_lib.graph_destroy(graph)
        return float(np.median(ts)), float(min(ts)), float(max(ts))
    t_batch = timed(O.scan_batch(x, rec_b, images=images, rows=rows, cols=cols, limit=1.0e30))
    t_whole = timed(O.scan(x, rec_w, rows=images * rows, cols=cols, limit=1.0e30))
    got_b, got_w = rec_b.cpu().numpy().view(np.uint64), hc.read_rec(rec_w)
    assert (got_b[:, 0] == 11).all() and (got_b[:, 6] == 11 * rows * cols).all() and not got_b[:, 1:5].any()
    assert got_w[0] == 11 and got_w[6] == got_b[:, 6].sum() and got_w[5] == got_b[:, 5].max()
    nbytes = 2 * images * rows * cols
    print("[health] per-image scan %.4f ms (%.4f .. %.4f) = %.2f TB/s; whole-batch scan %.4f ms (%.4f .. %.4f) = %.2f TB/s; %d images, %.1f MiB, bf16, "
          "one-op graphs, median of 10" % (t_batch[0] * 1e3, t_batch[1] * 1e3, t_batch[2] * 1e3, nbytes / t_batch[0] / 1e12,
                                           t_whole[0] * 1e3, t_whole[1] * 1e3, t_whole[2] * 1e3, nbytes / t_whole[0] / 1e12, images, nbytes / 2 ** 20))

"""Device fingerprints on an MI355X: the cases of tests/digest_cases.py (the emulator runs the same ones in tests/test_digest_emu.py) against
tests/digest_ref.py bit for bit, the planned forward with fingerprint= (eager run against hipGraph replay), one plan-file round trip with
i2i_plan_verify, and the timing line."""
import ctypes as C

import numpy as np
import pytest
import torch

import digest_cases as dc
import digest_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_lengths_and_alignments(gpu_lib, fmt):
    dc.check_lengths(gpu_lib, DEV, fmt)


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_pitched_rows(gpu_lib, fmt):
    dc.check_pitched(gpu_lib, DEV, fmt)


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_several_images(gpu_lib, fmt):
    dc.check_images(gpu_lib, DEV, fmt)


def test_capped_grid_second_pass(gpu_lib):
    dc.check_capped_grid(gpu_lib, DEV)


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_index_carry(gpu_lib, fmt):
    dc.check_index_carry(gpu_lib, DEV, fmt)


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_piecewise_identity(gpu_lib, fmt):
    dc.check_piecewise(gpu_lib, DEV, fmt)


def test_accumulate_and_clear(gpu_lib):
    dc.check_accumulate_clear(gpu_lib, DEV)


def test_sensitivity(gpu_lib):
    dc.check_sensitivity(gpu_lib, DEV, every_bit=False)


def test_refusals_and_no_ops(gpu_lib):
    dc.check_refusals(gpu_lib, DEV)


def test_eager_digest_and_first_diff(gpu_lib):
    dc.check_eager(gpu_lib, DEV)


def test_default_unchanged(gpu_lib):
    dc.check_default_unchanged(gpu_lib, DEV)


def test_forward_eager_equals_graph_replay(gpu_lib):
    dc.check_repeatable(gpu_lib, DEV, graph=True)


def test_forward_images_independent(gpu_lib):
    dc.check_images_independent(gpu_lib, DEV)


def test_weights_fingerprint_follows_the_scale(gpu_lib):
    dc.check_weights_fingerprint(gpu_lib, DEV)


def test_io_labels(gpu_lib):
    dc.check_io(gpu_lib, DEV)


def test_plan_file_round_trip(gpu_lib, tmp_path):
    dc.check_plan_file_fingerprint(gpu_lib, DEV, tmp_path)


def test_plan_verify(gpu_lib, tmp_path):
    dc.check_plan_verify(gpu_lib, DEV, tmp_path)


def test_digest_timing_line(gpu_lib):
    """Prints (does not gate): i2i_digest over 8 x 512 x 512 x 128 bf16 (512 MiB) as a one-op hipGraph, median of 10 replays after a warm-up,
    beside i2i_scan over the same tensor measured the same way and i2i_calib_stream over the same bytes (one read + one write of them).
    Asserted: bit-equality only -- eleven launches add up to eleven times one, one launch equals two launches over the two halves of every
    image (other grids, the piecewise identity), and the first 2^20 elements of image 5 equal the oracle."""
    from img2img_turbo_amd import _capi as K
    from img2img_turbo_amd import ops as O
    images, per = 8, 512 * 512 * 128
    x = (torch.rand(images * per, device=DEV) - 0.5).to(torch.bfloat16)
    dst = torch.empty_like(x)
    rec = torch.zeros(images, 4, dtype=torch.int64, device=DEV)
    rec_scan = torch.zeros(8, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = 2 * images * per

    def median_of(launch):
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    def timed(op):
        prog = K.Program()
        prog.add(op[0], K.BF16, op[1], "timing")
        prog.freeze()
        gpu_lib.run(prog, stream)                 # the warm-up, eager
        graph = gpu_lib.graph_create(prog)
        t = median_of(lambda: gpu_lib.graph_launch(graph, stream))
        gpu_lib.graph_destroy(graph)
        return t
    t_dig = timed(O.digest(x, rec, images=images, rows=1, cols=per))
    t_scan = timed(O.scan(x, rec_scan, rows=images * 512 * 512, cols=128, limit=1.0e30))
    copy = lambda: gpu_lib.check(gpu_lib.lib.i2i_calib_stream(C.c_void_p(x.data_ptr()), C.c_void_p(dst.data_ptr()), nbytes, C.c_void_p(stream)))
    copy()
    t_copy = median_of(copy)
    print("[digest] i2i_digest %.4f ms (%.4f .. %.4f) = %.2f TB/s read, %.1f G elements/s; i2i_scan %.4f ms (%.4f .. %.4f) = %.2f TB/s; "
          "i2i_calib_stream %.4f ms (%.4f .. %.4f) = %.2f TB/s read + written; %d images, %.0f MiB, bf16, one-op graphs, median of 10"
          % (t_dig[0] * 1e3, t_dig[1] * 1e3, t_dig[2] * 1e3, nbytes / t_dig[0] / 1e12, images * per / t_dig[0] / 1e9,
             t_scan[0] * 1e3, t_scan[1] * 1e3, t_scan[2] * 1e3, nbytes / t_scan[0] / 1e12,
             t_copy[0] * 1e3, t_copy[1] * 1e3, t_copy[2] * 1e3, 2 * nbytes / t_copy[0] / 1e12, images, nbytes / 2 ** 20))
    from img2img_turbo_amd.digest import digest
    got = rec.cpu().numpy().view(np.uint64)
    one = digest(x, images=images, lib=gpu_lib).numpy()
    with np.errstate(over="ignore"):
        assert np.array_equal(got, one * np.uint64(11)) and (one[:, 2] == per).all()
    xv = x.view(images, per)
    halves = R.add(digest(xv[:, :per // 2], images=images, lib=gpu_lib).numpy(), digest(xv[:, per // 2:], images=images, index0=per // 2, lib=gpu_lib).numpy())
    assert np.array_equal(one, halves)
    assert np.array_equal(digest(xv[5, :2 ** 20], lib=gpu_lib).numpy()[0], R.digest_ref(R.bits_of(xv[5, :2 ** 20]), 1, 2 ** 20))
    assert torch.equal(dst, x)

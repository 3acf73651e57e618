"""Tiled forward at native resolution on an MI355X: the cases of tests/test_tile_emu.py (shared through tests/tile_cases.py) with valid
descriptors only, both model classes on a 2-D layout, and one timing line."""
import numpy as np
import pytest
import torch

import tile_cases as tc

pytestmark = pytest.mark.gpu


def test_tile_abi_is_additive(gpu_lib):
    tc.check_struct_size(gpu_lib)


@pytest.mark.parametrize("case", tc.POSITION_CASES, ids=lambda c: "L%d_t%d_ov%d" % c)
def test_tile_positions(gpu_lib, case):
    tc.check_positions(gpu_lib, *case)


def test_tile_positions_examples_and_errors(gpu_lib):
    tc.check_positions_examples(gpu_lib)
    tc.check_positions_errors(gpu_lib)


@pytest.mark.parametrize("name", sorted(tc.LAYOUTS))
def test_tile_cut_rgb(gpu_lib, name):
    tc.check_cut(gpu_lib, "cuda", name, 3)


@pytest.mark.parametrize("c", [1, 4])
def test_tile_cut_other_channel_counts(gpu_lib, c):
    tc.check_cut(gpu_lib, "cuda", "one_tile_24x16_ov8", c)
    tc.check_cut(gpu_lib, "cuda", "triple_16_ov8", c)


def test_tile_cut_fp32_planes(gpu_lib):
    tc.check_cut(gpu_lib, "cuda", "triple_16_ov8", f32=True)
    tc.check_cut(gpu_lib, "cuda", "one_tile_24x16_ov8", f32=True)
    tc.check_planes_eager(gpu_lib, "cuda")


@pytest.mark.parametrize("name", sorted(tc.LAYOUTS))
def test_tile_blend_rgb(gpu_lib, name):
    tc.check_blend(gpu_lib, "cuda", name, 3)


@pytest.mark.parametrize("c", [1, 4])
def test_tile_blend_other_channel_counts(gpu_lib, c):
    tc.check_blend(gpu_lib, "cuda", "triple_16_ov8", c)


@pytest.mark.parametrize("name", sorted(tc.LAYOUTS))
def test_tile_round_trip(gpu_lib, name):
    tc.check_round_trip(gpu_lib, "cuda", name, 3)


def test_tile_grid_independence(gpu_lib):
    tc.check_grid_independence(gpu_lib, "cuda")


def test_tile_one_graph_two_request_sets(gpu_lib):
    tc.check_graph(gpu_lib, "cuda")


def test_tile_bad_args(gpu_lib):
    tc.check_bad_args(gpu_lib, "cuda")


def test_tile_noise_rule(gpu_lib):
    tc.check_noise(gpu_lib, "cuda")


def test_tile_value_errors(gpu_lib):
    tc.check_value_errors(gpu_lib, "cuda")


MODEL_SIZES = [(56, 72), (32, 40)]           # 2 x 2 tiles of (40, 32) at overlap 8, and a request that is exactly one tile


def test_tile_pix2pix_forward_u8(gpu_lib):
    tc.check_pix2pix_tiled(gpu_lib, "cuda", MODEL_SIZES)


def test_tile_pix2pix_forward_u8_with_canny(gpu_lib):
    tc.check_pix2pix_tiled(gpu_lib, "cuda", MODEL_SIZES, canny=(100, 200), stacked=False)


def test_tile_pix2pix_forward_u8_bf16(gpu_lib):
    tc.check_pix2pix_tiled(gpu_lib, "cuda", MODEL_SIZES, dtype=torch.bfloat16, overlap=16, tile_batch=3, stacked=False)


def test_tile_cyclegan_forward_u8(gpu_lib):
    tc.check_cyclegan_tiled(gpu_lib, "cuda", MODEL_SIZES)


def test_tile_timing_line(gpu_lib):
    """One 1280 x 720 request, tile 512, overlap 64, six tiles: cut and blend as ONE captured graph (HIP events, one warm-up, the median
    of 10 replays), printed beside i2i_calib_stream over the same bytes (what the two ops read and write: the request and the tile batch,
    each once per op) and beside the pair of lanczos_resize_u8 calls (to 512 x 512 and back) the resize route spends on the same request,
    all in this process.  Print only; asserted: the tiled output has the request's shape and the round trip is exact."""
    import ctypes as C
    from img2img_turbo_amd import _capi as K, image_ops, ops as O
    h, w, t, ov = 720, 1280, 512, 64
    img = tc.to_dev(tc.photo(h, w, 7), "cuda")
    layout = image_ops.tile_layout([(h, w)], (t, t), ov)
    assert layout.T == 6 and layout.xs == [[0, 448, 768]] and layout.ys == [[0, 208]]
    table = layout.table(1, 3, 1, img.device)
    src = img.reshape(-1)
    tiles = torch.empty(6 * t * t * 3, dtype=torch.uint8, device="cuda")
    back = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
    prog = K.Program()
    prog.add(*_with_dtype(O.tile_cut(src, tiles, table.desc_dev, table.pos_dev, n=1, planes=1, px_bytes=3, tw=t, th=t, tiles_capacity=6,
                                     grid_units=table.units_cut)), "tile.cut")
    prog.add(*_with_dtype(O.tile_blend_u8(tiles, back, table.desc_dev, table.pos_dev, n=1, c=3, ramp=ov, tw=t, th=t, tiles_capacity=6,
                                          grid_units=table.units_blend)), "tile.blend")
    prog.freeze()
    stream = torch.cuda.current_stream().cuda_stream

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sorted(ms)

    g = gpu_lib.graph_create(prog)
    try:
        tg = events(lambda: gpu_lib.graph_launch(g, stream))
    finally:
        torch.cuda.synchronize()
        gpu_lib.graph_destroy(g)
    assert back.view(h, w, 3).shape == img.shape and torch.equal(back.view(h, w, 3), img)      # the round trip is exact
    moved = 2 * (h * w * 3 + 6 * t * t * 3)                                   # bytes read + written by the two ops together
    nbytes = (moved // 2 + 15) & ~15                                          # i2i_calib_stream moves 2 * bytes
    a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tcopy = events(lambda: gpu_lib.check(gpu_lib.lib.i2i_calib_stream(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), nbytes, C.c_void_p(stream))))
    tres = events(lambda: image_ops.lanczos_resize_u8(image_ops.lanczos_resize_u8(img[None], (512, 512), lib=gpu_lib), (w, h), lib=gpu_lib))
    print("[tile] 1280x720 RGB, tile 512, overlap 64, 6 tiles: cut + blend as one captured graph median %.4f ms (min %.4f, max %.4f) for %.1f MB "
          "moved = %.0f GB/s; i2i_calib_stream over the same bytes median %.4f ms (min %.4f, max %.4f) = %.0f GB/s: cut + blend run at %.2f of "
          "the copy rate; the resize route's two lanczos_resize_u8 calls (to 512x512 and back, eager, four launches) median %.4f ms (min %.4f, "
          "max %.4f); 10 runs each, HIP events" % (tg[5], tg[0], tg[-1], moved / 1e6, moved / tg[5] / 1e6, tcopy[5], tcopy[0], tcopy[-1],
                                                    2 * nbytes / tcopy[5] / 1e6, tcopy[5] / tg[5], tres[5], tres[0], tres[-1]))
    # the eager form on the same request: the request's shape, the same bits
    cut, lay = image_ops.tile_cut_u8(img[None], (t, t), ov, gpu_lib)
    out = image_ops.tile_blend_u8(cut, lay, gpu_lib, stack=True)
    assert out.shape == (1, h, w, 3) and torch.equal(out[0], img) and torch.equal(cut.reshape(-1), tiles)


def _with_dtype(op):
    from img2img_turbo_amd import _capi as K
    return op[0], K.F32, op[1]

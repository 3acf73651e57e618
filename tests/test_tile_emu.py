"""Tiled forward at native resolution on the CPU emulator: i2i_tile_positions (the layout rule), i2i_tile_cut (requests -> a dense tile
batch) and i2i_tile_blend_u8 (tile outputs -> requests, integer feather), image_ops.tile_* and ``tile=`` of Pix2Pix_Turbo /
CycleGAN_Turbo .forward_u8.  tests/test_tile_gpu.py runs the same cases (tests/tile_cases.py) on an MI355X; the wrong-descriptor cases run
here only.  The oracle is tests/tile_ref.py, bit-exact."""
import os

import pytest

import tile_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_LIB = os.path.join(ROOT, "img2img-turbo_amd", "csrc", "libi2i_turbo.so")


def test_tile_abi_is_additive(emu_lib):
    """sizeof(i2i_op) did not grow, the version did not move, the opcodes are 27 and 28, the descriptor is 48 bytes in both bindings."""
    tc.check_struct_size(emu_lib)


# ---------------------------------------------------------------------------------------------------------------- positions
@pytest.mark.parametrize("case", tc.POSITION_CASES, ids=lambda c: "L%d_t%d_ov%d" % c)
def test_tile_positions(emu_lib, case):
    tc.check_positions(emu_lib, *case)


@pytest.mark.parametrize("case", tc.POSITION_CASES, ids=lambda c: "L%d_t%d_ov%d" % c)
def test_tile_positions_product_library(case):
    """The same host code as hipcc compiled it into the product library (no GPU is touched: plain host C++)."""
    from img2img_turbo_amd import _capi
    assert os.path.exists(PRODUCT_LIB), "the product library is not built (python __graft_entry__.py)"
    tc.check_positions(_capi.Library(PRODUCT_LIB), *case)


def test_tile_positions_examples_and_errors(emu_lib):
    tc.check_positions_examples(emu_lib)
    tc.check_positions_errors(emu_lib)


# ---------------------------------------------------------------------------------------------------------------- cut and blend
@pytest.mark.parametrize("name", sorted(tc.LAYOUTS))
def test_tile_cut_rgb(emu_lib, name):
    tc.check_cut(emu_lib, "cpu", name, 3)


@pytest.mark.parametrize("c", [1, 4])
def test_tile_cut_other_channel_counts(emu_lib, c):
    tc.check_cut(emu_lib, "cpu", "one_tile_24x16_ov8", c)
    tc.check_cut(emu_lib, "cpu", "triple_16_ov8", c)


def test_tile_cut_fp32_planes(emu_lib):
    tc.check_cut(emu_lib, "cpu", "triple_16_ov8", f32=True)
    tc.check_cut(emu_lib, "cpu", "one_tile_24x16_ov8", f32=True)
    tc.check_planes_eager(emu_lib, "cpu")


@pytest.mark.parametrize("name", sorted(tc.LAYOUTS))
def test_tile_blend_rgb(emu_lib, name):
    tc.check_blend(emu_lib, "cpu", name, 3)


@pytest.mark.parametrize("c", [1, 4])
def test_tile_blend_other_channel_counts(emu_lib, c):
    tc.check_blend(emu_lib, "cpu", "triple_16_ov8", c)


@pytest.mark.parametrize("name", sorted(tc.LAYOUTS))
def test_tile_round_trip(emu_lib, name):
    tc.check_round_trip(emu_lib, "cpu", name, 3)


def test_tile_grid_independence(emu_lib):
    tc.check_grid_independence(emu_lib, "cpu")


def test_tile_one_graph_two_request_sets(emu_lib):
    tc.check_graph(emu_lib, "cpu")


def test_tile_bad_args(emu_lib):
    tc.check_bad_args(emu_lib, "cpu")


@pytest.mark.parametrize("what", tc.REJECTS, ids=lambda s: s.replace(" ", "_"))
def test_tile_rejected_descriptor(emu_lib, what):
    tc.check_rejection(emu_lib, "cpu", what)


# ---------------------------------------------------------------------------------------------------------------- the models
def test_tile_noise_rule(emu_lib):
    tc.check_noise(emu_lib, "cpu")


def test_tile_value_errors(emu_lib):
    tc.check_value_errors(emu_lib, "cpu")


@pytest.mark.slow
def test_tile_pix2pix_forward_u8_with_canny(emu_lib):
    """Two tiles of a 32 x 72 request and a request that is exactly one tile, as one chunk of 3 (one plan to build): 2 x 3 x 1280 = 7680
    pixels of forward.  The 2-D layout, remainder chunks, the plain branch, CycleGAN_Turbo and bf16 run on the GPU file."""
    tc.check_pix2pix_tiled(emu_lib, "cpu", [(32, 72), (32, 40)], canny=(100, 200), tile_batch=3, stacked=False)

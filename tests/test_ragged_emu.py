"""Mixed-size images in one batch on the CPU emulator: i2i_resize_u8_ragged (one separable LANCZOS pass over a ragged batch, descriptors
and tap tables read from device memory) and i2i_lanczos_tables (the tables for hosts that are not Python), image_ops.lanczos_resize_u8_ragged
and the list forms of Pix2Pix_Turbo / CycleGAN_Turbo .forward_u8.  tests/test_ragged_gpu.py runs the same cases (tests/ragged_cases.py) on an
MI355X; the descriptor-rejection cases run here only.  Oracles: image_ops.lanczos_resize_u8 on each image alone (c = 1 .. 4) and Pillow
(c = 1, 3), both bit-exact."""
import os

import pytest

import ragged_cases as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_LIB = os.path.join(ROOT, "img2img-turbo_amd", "csrc", "libi2i_turbo.so")


def test_ragged_abi_is_additive(emu_lib):
    """sizeof(i2i_op) did not grow, the version did not move, the opcode is 21, the descriptor is 48 bytes in both bindings."""
    rg.check_struct_size(emu_lib)


# ---------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("pair", rg.TABLE_PAIRS, ids=lambda p: "%dto%d" % p)
def test_lanczos_tables_emulator_library(emu_lib, pair):
    rg.check_tables(emu_lib, pair)


@pytest.mark.parametrize("pair", rg.TABLE_PAIRS, ids=lambda p: "%dto%d" % p)
def test_lanczos_tables_product_library(pair):
    """The same host code as hipcc compiled it into the product library (no GPU is touched: the tables are plain host C++)."""
    from img2img_turbo_amd import _capi
    assert os.path.exists(PRODUCT_LIB), "the product library is not built (python __graft_entry__.py)"
    rg.check_tables(_capi.Library(PRODUCT_LIB), pair)


def test_lanczos_tables_errors(emu_lib):
    rg.check_tables_errors(emu_lib)


def test_same_size_tables_are_the_identity():
    rg.check_identity_tables()


# ---------------------------------------------------------------------------------------------------------------- the resize
def test_ragged_in(emu_lib):
    rg.check_ragged_in(emu_lib, "cpu")


def test_ragged_out(emu_lib):
    rg.check_ragged_out(emu_lib, "cpu")


@pytest.mark.parametrize("c", [1, 4])
def test_ragged_other_channel_counts(emu_lib, c):
    rg.check_channels(emu_lib, "cpu", c)


def test_ragged_empty_slot_and_write_bounds(emu_lib):
    rg.check_write_bounds(emu_lib, "cpu")


def test_ragged_grid_independence(emu_lib):
    rg.check_grid_independence(emu_lib, "cpu")


def test_ragged_python_tables(emu_lib):
    rg.check_python_tables_too(emu_lib, "cpu")


def test_ragged_one_graph_two_requests(emu_lib):
    rg.check_graph(emu_lib, "cpu")


def test_ragged_bad_args(emu_lib):
    rg.check_bad_args(emu_lib, "cpu")


@pytest.mark.parametrize("what", rg.REJECTS, ids=lambda s: s.replace(" ", "_"))
def test_ragged_rejected_descriptor(emu_lib, what):
    rg.check_rejection(emu_lib, "cpu", what)


# ---------------------------------------------------------------------------------------------------------------- the models
@pytest.mark.slow
def test_ragged_pix2pix_forward_u8_list(emu_lib):
    rg.check_pix2pix_list(emu_lib, "cpu")


@pytest.mark.slow
def test_ragged_cyclegan_forward_u8_list(emu_lib):
    rg.check_cyclegan_list(emu_lib, "cpu")

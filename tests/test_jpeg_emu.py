"""JPEG encoding on the device, on the CPU emulator: the oracle tests/jpeg_ref.py against the installed Pillow, then i2i_jpeg_encode_u8,
i2i_jpeg_header, image_ops.jpeg_encode_u8 and ``jpeg=`` of Pix2Pix_Turbo / CycleGAN_Turbo .forward_u8 against the oracle and against Pillow.
tests/test_jpeg_gpu.py runs the same cases (tests/jpeg_cases.py) on an MI355X; the wrong-descriptor cases run here only.  Every comparison
is ``==`` on whole files."""
import os

import pytest

import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_LIB = os.path.join(ROOT, "img2img-turbo_amd", "csrc", "libi2i_turbo.so")
SIZE_IDS = ["%dx%d" % s for s in jc.SIZES]


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("size", jc.SIZES, ids=SIZE_IDS)
def test_oracle_matches_pillow(size):
    """Pins the oracle: whole files, 4 contents x 7 qualities x 2 subsamplings per size.  A Pillow that writes another header fails with
    the marker that differs; a difference in the scan is named as such."""
    assert jc.have_pillow_jpeg(), "this Pillow has no JPEG encoder (PIL.features.check('jpg')): the oracle cannot be pinned here"
    jc.check_oracle_matches_pillow(*size)


def test_cases_hold_what_they_are_for():
    jc.check_case_properties()
    jc.check_big_has_three_chunks()


# ---------------------------------------------------------------------------------------------------------------- the ABI and the host code
def test_jpeg_abi_is_additive(emu_lib):
    jc.check_abi(emu_lib)


def test_jpeg_header_host_code(emu_lib):
    jc.check_header(emu_lib)


def test_jpeg_header_product_library():
    """The same host code as hipcc compiled it into the product library (no GPU is touched: plain host C++)."""
    from img2img_turbo_amd import _capi
    assert os.path.exists(PRODUCT_LIB), "the product library is not built (python __graft_entry__.py)"
    lib = _capi.Library(PRODUCT_LIB)
    jc.check_header(lib)
    jc.check_abi(lib)


# ---------------------------------------------------------------------------------------------------------------- the encoder
@pytest.mark.parametrize("size", jc.SIZES, ids=SIZE_IDS)
def test_jpeg_grid(emu_lib, size):
    jc.check_grid(emu_lib, "cpu", *size)


def test_jpeg_ragged_batch(emu_lib):
    jc.check_ragged_batch(emu_lib, "cpu")


def test_jpeg_grid_independence(emu_lib):
    jc.check_grid_independence(emu_lib, "cpu")


def test_jpeg_overflow_is_flagged(emu_lib):
    jc.check_overflow(emu_lib, "cpu")


@pytest.mark.parametrize("what", jc.REJECTS, ids=lambda s: s.replace(" ", "_"))
def test_jpeg_rejected_descriptor(emu_lib, what):
    jc.check_rejection(emu_lib, "cpu", what)


def test_jpeg_bad_args(emu_lib):
    jc.check_bad_args(emu_lib, "cpu")


# ---------------------------------------------------------------------------------------------------------------- the models
@pytest.mark.slow
def test_jpeg_forward_u8(emu_lib):
    """Two forwards of the tiny model (one plan): the keyword, its parsing and the order of the files.  Both model classes, variations=,
    tile= and return_edges= run on the GPU file."""
    jc.check_forward_jpeg(emu_lib, "cpu", "pix2pix", light=True)

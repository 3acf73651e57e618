"""PNG encoding on the device, on the CPU emulator: the oracle tests/png_ref.py against the installed Pillow and zlib, then
i2i_png_encode_u8, i2i_png_bound, image_ops.png_encode_u8 and ``png=`` of Pix2Pix_Turbo.forward_u8 against the oracle.
tests/test_png_gpu.py runs the same cases (tests/png_cases.py) on an MI355X; the wrong-descriptor cases run here only.  Every comparison is
``==``."""
import os

import pytest

import png_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_LIB = os.path.join(ROOT, "img2img-turbo_amd", "csrc", "libi2i_turbo.so")
SIZE_IDS = ["%dx%d" % s for s in pc.SIZES]


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("size", pc.SIZES, ids=SIZE_IDS)
def test_oracle_matches_pillow(size):
    """5 contents x 2 channel counts per size: the container, the filtered stream (zlib.decompress of both), every CRC, the decoded
    pixels, the bound."""
    pc.check_oracle_matches_pillow(*size)


def test_cases_hold_what_they_are_for():
    pc.check_case_properties()
    pc.check_big_spans_three()


def test_repair_rule():
    pc.check_repair_rule()


def test_code_length_alphabet_repair_case():
    pc.check_cl_repair_case()


def test_litlen_repair_case():
    pc.check_litlen_repair_case()


# ---------------------------------------------------------------------------------------------------------------- the ABI and the host code
def test_png_abi_is_additive(emu_lib):
    pc.check_abi(emu_lib)


def test_png_bound_host_code(emu_lib):
    pc.check_bound(emu_lib)


def test_png_bound_product_library():
    """The same host code as hipcc compiled it into the product library (no GPU is touched: plain host C++)."""
    from img2img_turbo_amd import _capi
    assert os.path.exists(PRODUCT_LIB), "the product library is not built (python __graft_entry__.py)"
    lib = _capi.Library(PRODUCT_LIB)
    pc.check_bound(lib)
    pc.check_abi(lib)


# ---------------------------------------------------------------------------------------------------------------- the encoder
@pytest.mark.parametrize("size", pc.SIZES, ids=SIZE_IDS)
def test_png_grid(emu_lib, size):
    pc.check_grid(emu_lib, "cpu", *size)


def test_png_ragged_batch(emu_lib):
    pc.check_ragged_batch(emu_lib, "cpu")


def test_png_invert(emu_lib):
    pc.check_invert(emu_lib, "cpu")


def test_png_grid_independence(emu_lib):
    pc.check_grid_independence(emu_lib, "cpu")


def test_png_overflow_is_flagged(emu_lib):
    pc.check_overflow(emu_lib, "cpu")


@pytest.mark.parametrize("what", pc.REJECTS, ids=lambda s: s.replace(" ", "_"))
def test_png_rejected_descriptor(emu_lib, what):
    pc.check_rejection(emu_lib, "cpu", what)


def test_png_bad_args(emu_lib):
    pc.check_bad_args(emu_lib, "cpu")


# ---------------------------------------------------------------------------------------------------------------- the models
@pytest.mark.slow
def test_png_forward_u8(emu_lib):
    """Two forwards of the tiny model (one plan): the keyword and its refusals.  Both model classes, variations=, tile= and
    return_edges="png" run on the GPU file."""
    pc.check_forward_png(emu_lib, "cpu", "pix2pix", light=True)

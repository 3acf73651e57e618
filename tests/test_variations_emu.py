"""Variations on the CPU emulator: i2i_repeat (the contract of i2i_repeat_params, include/i2i_turbo.h) and ForwardPlan / Pix2Pix_Turbo with
``variations=V``.  The cases are tests/variations_cases.py, shared with tests/test_variations_gpu.py."""
import pytest
import torch

import variations_cases as vc


# ---------------------------------------------------------------------------------------------------------------- i2i_repeat
def test_struct_size(emu_lib):
    vc.check_struct_size(emu_lib)


@pytest.mark.parametrize("name", list(vc.REPEAT_CASES))
def test_repeat(emu_lib, name):
    vc.check_repeat(emu_lib, "cpu", name)


def test_repeat_errors(emu_lib):
    vc.check_repeat_errors(emu_lib, "cpu")


# ---------------------------------------------------------------------------------------------------------------- the planned forward
# (bf16 where the assertion is bit-equality between two runs of the library: the emulator's exact-fp32 MFMA path is several times slower)
@pytest.mark.slow
def test_encoder_runs_once(emu_lib):
    vc.check_encoder_once(emu_lib, "cpu", h=8, w=16, dtype=torch.bfloat16)


@pytest.mark.slow
@pytest.mark.parametrize("shape,stochastic,dtype", [((2, 3, 8, 16), True, torch.float32), ((1, 4, 8, 24), False, torch.bfloat16)],
                         ids=["B2V3_8x16_twinconv_r0.4_f32", "B1V4_8x24_deterministic_bf16"])
def test_parity_with_the_oracle(emu_lib, shape, stochastic, dtype):
    """The batch shapes, models and element types of the parity cases at emulator sizes (it needs about a second per thousand pixels of a
    forward); tests/test_variations_gpu.py runs all eight combinations at 64 x 64 and 72 x 88."""
    vc.check_parity(emu_lib, "cpu", shape, stochastic, dtype)


@pytest.mark.slow
def test_v1_is_todays_forward(emu_lib):
    vc.check_v1(emu_lib, "cpu", h=8, w=16, dtype=torch.bfloat16)


@pytest.mark.slow
def test_seeds(emu_lib):
    """The stochastic model (eps and the noise map); hipGraph capture and the deterministic model are the GPU test's."""
    vc.check_seeds(emu_lib, "cpu", True, graph=False, h=8, w=16, dtype=torch.bfloat16)


@pytest.mark.slow
def test_forward_u8_canny(emu_lib):
    vc.check_u8_canny(emu_lib, "cpu", h=16, w=16, dtype=torch.bfloat16)


@pytest.mark.slow
def test_plan_file_round_trip(emu_lib, tmp_path):
    vc.check_plan_file(emu_lib, "cpu", tmp_path, h=8, w=16, dtype=torch.bfloat16)


@pytest.mark.slow
def test_exporter_cli(emu_lib, tmp_path):
    vc.check_cli(emu_lib, "cpu", tmp_path)


def test_per_image_health_raises(emu_lib):
    vc.check_health_per_image_raises(emu_lib, "cpu")

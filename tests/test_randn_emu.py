"""Seeded Gaussian noise on the device (i2i_randn, csrc/elementwise.hip; img2img_turbo_amd/rng.py) on the CPU emulator, against
tests/randn_ref.py -- the oracle of the contract in include/i2i_turbo.h -- plus the oracle's own known answers.
tests/test_randn_gpu.py runs the same cases (tests/randn_cases.py) on an MI355X.

Measured max |err| / rad of the normal kind (bound 2^-21 = 4.77e-7): 1.6e-7 on the emulator (host logf, double-precision sine / cosine).
A transform with an fp32 product 2*pi*u2 and cosf / sinf, tried once as a mutation, reaches 4.26e-7 = 0.89 of the bound: it does NOT fail
test_randn_normal, contrary to what the issue behind the op expected (the angle's rounding error is at most 2^-22 + 1.75e-7 absolute)."""
import numpy as np
import pytest
import torch

import randn_cases as rc
import randn_ref


# ---------------------------------------------------------------------------------------------------------------- 1. the oracle itself
def test_oracle_known_answers():
    """Philox4x32-10 against the Random123 known-answer vectors (kat_vectors: philox4x32 10)."""
    kats = [([0, 0, 0, 0], (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kats:
        got = randn_ref.philox4x32_10(np.array(ctr, dtype=np.uint32), key)
        assert " ".join("%08x" % v for v in got) == want
    # the element map: element i is lane i & 3 of counter {i >> 2, 0, step, stream}, key {seed lo, seed hi}
    w = randn_ref.raw(7, (0x299F31D0 << 32) | 0xA4093822, 0x13198A2E, 0x03707344)
    assert w.dtype == np.uint32 and w.shape == (7,)
    for q in (0, 1):
        full = randn_ref.philox4x32_10(np.array([q, 0, 0x13198A2E, 0x03707344], dtype=np.uint32), (0xA4093822, 0x299F31D0))
        assert np.array_equal(w[4 * q:4 * q + 4], full[:len(w[4 * q:4 * q + 4])])
    assert np.array_equal(randn_ref.raw(4, 0)[:4], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8])
    # the transform: u1 = 1 (word 0xffffffxx) gives rad = 0, and the bound |x| <= sqrt(48 ln 2) is u1 = 2^-24
    val, rad = randn_ref.normal(16384, 42)
    assert val.dtype == np.float64 and np.abs(val).max() <= rc.ABS_MAX and rad.min() >= 0
    assert abs(np.sqrt(-2.0 * np.log(2.0 ** -24)) - np.sqrt(48 * np.log(2.0))) < 1e-12 and np.sqrt(48 * np.log(2.0)) < rc.ABS_MAX


# ---------------------------------------------------------------------------------------------------------------- 2. - 6. the kernel
@pytest.mark.parametrize("n", rc.SIZES)
def test_randn_raw(emu_lib, n):
    rc.check_raw(emu_lib, "cpu", n)


def test_randn_stride_loop(emu_lib):
    """2^20 + 3 elements: one Philox counter more than a whole pass of the grid."""
    rc.check_raw(emu_lib, "cpu", rc.BIG, combos=[(42, 1, 2)])
    rc.normal_errors(emu_lib, "cpu", rc.BIG, combos=[(42, 1, 2)], offsets=[1])


def test_randn_device_state_equals_immediates(emu_lib):
    rc.check_state_form(emu_lib, "cpu")


@pytest.mark.parametrize("n", rc.SIZES)
def test_randn_normal(emu_lib, n):
    worst = rc.normal_errors(emu_lib, "cpu", n)
    print("[randn] emulator, n = %d: max |err| / rad = %.3g (bound %.3g)" % (n, worst, rc.TOL))


def test_randn_statistics(emu_lib):
    rc.check_statistics(emu_lib, "cpu")


def test_randn_state_and_advance(emu_lib):
    rc.check_advance(emu_lib, "cpu")


def test_randn_abi(emu_lib):
    rc.check_abi(emu_lib, "cpu")


def test_randn_module(emu_lib):
    rc.check_module(emu_lib, "cpu")


# ---------------------------------------------------------------------------------------------------------------- 7., 9. the pipeline
@pytest.mark.slow
def test_randn_pipeline(emu_lib):
    """The stochastic model (both noise buffers) at 24 x 40; tests/test_randn_gpu.py runs both modes at 72 x 88.  (A forward of the tiny model
    costs the emulator some twenty seconds whatever its size.)"""
    model, _, _ = rc.check_pipeline(emu_lib, "cpu", True, h=24, w=40)
    model.release_plans()


@pytest.mark.slow
def test_randn_plan_file(emu_lib, tmp_path):
    """plan_file --seed: the io table holds "seed" (16 bytes, the exported value); a host that writes another seed and runs gets the
    "out" and "eps" of the Python replay at that seed, bit for bit, and the step has moved on."""
    from img2img_turbo_amd import arch, plan_file, rng
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.synth import make_pix2pix_weights
    path = str(tmp_path / "seeded.i2iplan")
    plan_file.main(["--out", path, "--synthetic", "--arch", "tiny", "--batch", "1", "--size", "16", "24", "--dtype", "f32", "--stochastic",
                    "--seed", str((1 << 40) + 7), "--device", "cpu", "--lib", emu_lib.path])
    w = make_pix2pix_weights(arch.TINY_UNET, arch.TINY_VAE, seed=1234, sketch=True)      # (the weights plan_file --synthetic --arch tiny makes)
    model = Pix2Pix_Turbo(weights=w, device="cpu", dtype=torch.float32, lib=emu_lib)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 3, 16, 24, generator=g) * 2 - 1
    cap = torch.randn(1, 77, arch.TINY_UNET.cross_attention_dim, generator=g)
    seed = 0xFEDCBA9876543210
    want = model.forward(x, caption_enc=cap, deterministic=False, r=0.4, seed=seed)
    plan = list(model._plans.values())[0]
    h = emu_lib.plan_load(path)
    try:
        assert emu_lib.plan_io(h, "seed")[1] == 16
        saved = emu_lib.plan_read(h, "seed", torch.zeros(4, dtype=torch.int32))
        assert rc.read_state(saved) == [7, 1 << 8, 0, 0]
        emu_lib.plan_write(h, "x", x)
        emu_lib.plan_write(h, "ctx", cap)
        emu_lib.plan_write(h, "seed", rc.state_tensor(rng.pack_state(seed), "cpu"))
        emu_lib.plan_run(h)
        assert torch.equal(emu_lib.plan_read(h, "out", torch.zeros(1, 3, 16, 24)), want)
        assert torch.equal(emu_lib.plan_read(h, "eps", torch.zeros(1, 4, 2, 3)), plan.eps)
        assert torch.equal(emu_lib.plan_read(h, "noise", torch.zeros(1, 4, 2, 3)), plan.noise)
        assert rc.read_state(emu_lib.plan_read(h, "seed", torch.zeros(4, dtype=torch.int32))) == rng.pack_state(seed, 1)
    finally:
        emu_lib.plan_destroy(h)
        model.release_plans()

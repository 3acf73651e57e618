"""Per-image request parameters of a batch on the CPU emulator: i2i_randn_batch (one noise state per image) and i2i_canny_u8_batch (one
threshold pair per image) -- the "ABI 14 additions" of include/i2i_turbo.h -- their eager forms (img2img_turbo_amd/rng.py, image_ops.py), the
planned forwards (ForwardPlan(rng="per_image" / canny="per_image"), forward(seed=[..])), plan files and examples/batch_host.c.
tests/test_batch_gpu.py runs the same cases (tests/batch_cases.py) on an MI355X.  The oracles are tests/randn_ref.py and tests/canny_ref.py,
applied per image; every comparison is bit-exact except the normal kind against the fp64 oracle (the existing contract's rad * 2^-21)."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import batch_cases as bc
import randn_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_batch_abi_is_additive(emu_lib):
    """sizeof(i2i_op) did not grow, the version did not move, the opcodes are 19 and 20."""
    bc.check_struct_size(emu_lib)


def test_batch_grid_cap_mirror():
    """rng.BATCH_MAX_BLOCKS (what big_size() is derived from) is the kernel launch's cap."""
    from img2img_turbo_amd import rng
    with open(os.path.join(ROOT, "img2img-turbo_amd", "csrc", "elementwise.hip")) as f:
        m = re.search(r"constexpr int RANDN_BATCH_MAX_BLOCKS = (\d+);", f.read())
    assert m and int(m.group(1)) == rng.BATCH_MAX_BLOCKS
    assert bc.big_size() == (rng.BATCH_MAX_BLOCKS // bc.B) * 1024 + 1


# ---------------------------------------------------------------------------------------------------------------- randn_batch
@pytest.mark.parametrize("per_image", bc.SIZES)
def test_randn_batch_raw(emu_lib, per_image):
    bc.check_raw(emu_lib, "cpu", per_image)


@pytest.mark.parametrize("per_image", bc.SIZES)
def test_randn_batch_normal(emu_lib, per_image):
    worst = bc.check_normal(emu_lib, "cpu", per_image, oracle=True)
    print("[randn_batch] emulator, per_image = %d: max |err| / rad = %.3g (bound %.3g)" % (per_image, worst, rc.TOL))


def test_randn_batch_stride_loop(emu_lib):
    """One Philox counter per image more than a pass of the capped grid covers at batch 3."""
    bc.check_raw(emu_lib, "cpu", bc.big_size())


def test_randn_batch_advance(emu_lib):
    bc.check_advance(emu_lib, "cpu")


def test_randn_batch_errors(emu_lib):
    bc.check_errors(emu_lib, "cpu")


def test_randn_batch_module(emu_lib):
    bc.check_module(emu_lib, "cpu")


# ---------------------------------------------------------------------------------------------------------------- Canny per image
def test_canny_batch(emu_lib):
    bc.check_canny(emu_lib, "cpu")


# ---------------------------------------------------------------------------------------------------------------- the planned forward
@pytest.mark.slow
@pytest.mark.parametrize("stochastic", [False, True])
def test_batch_forward(emu_lib, stochastic):
    """At 24 x 40 (a latent of 3 x 5: 60 elements per image), as the emulator's seeded-forward test; tests/test_batch_gpu.py runs 72 x 88."""
    model, _ = bc.check_forward(emu_lib, "cpu", stochastic, h=24, w=40)
    model.release_plans()


@pytest.mark.slow
def test_batch_forward_canny(emu_lib):
    bc.check_forward_canny(emu_lib, "cpu", h=24, w=40)


@pytest.mark.slow
def test_batch_plan_file_and_c_host(emu_lib, tmp_path):
    """The exported per-image plan through i2i_plan_load and through examples/batch_host.c (gcc against the emulator library); the
    command-line exporter's --seeds / --canny-per-image; a scalar-seed plan file still loads and runs."""
    from img2img_turbo_amd import plan_file, rng
    h, w = 16, 24
    model = rc.make_model(emu_lib, "cpu", False)
    try:
        x, cap = rc.pipeline_inputs(bc.B, "cpu", h, w)
        plan = model.get_plan(bc.B, h, w, rng="per_image")
        path, eps, want = bc.check_plan_file(emu_lib, "cpu", tmp_path, model, plan, x, cap, bc.FWD_SEEDS)
        # the same file through a host that is not Python
        if shutil.which("gcc"):
            exe = str(tmp_path / "batch_host")
            subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "batch_host.c"), "-o", exe,
                            "-L", os.path.dirname(emu_lib.path), "-l" + os.path.basename(emu_lib.path)[3:-3], "-Wl,-rpath," + os.path.dirname(emu_lib.path)],
                           check=True)
            files = {}
            for name, t in (("x", x), ("ctx", cap.reshape(plan.ctx.shape))):
                files[name] = str(tmp_path / (name + ".bin"))
                with open(files[name], "wb") as f:
                    f.write(t.contiguous().view(torch.uint8).numpy().tobytes())
            eps_out, out_out = str(tmp_path / "eps_out.bin"), str(tmp_path / "out_out.bin")
            env = dict(os.environ)
            env.pop("I2I_EMU_ASYNC", None)
            r = subprocess.run([exe, path, files["x"], files["ctx"], eps_out, out_out] + [str(s) for s in bc.FWD_SEEDS], capture_output=True, text=True, env=env)
            assert r.returncode == 0, r.stderr
            with open(eps_out, "rb") as f:
                assert torch.equal(torch.frombuffer(bytearray(f.read()), dtype=torch.int32), eps.view(torch.int32).reshape(-1))
            with open(out_out, "rb") as f:
                assert torch.equal(torch.frombuffer(bytearray(f.read()), dtype=torch.float32).reshape(want.shape), want)
            # a seed count that does not match the plan's table is refused with a message
            r = subprocess.run([exe, path, files["x"], files["ctx"], eps_out, out_out, "1", "2"], capture_output=True, text=True, env=env)
            assert r.returncode != 0 and "48 bytes" in r.stderr, r.stderr
        # the command-line exporter
        cli = str(tmp_path / "cli.i2iplan")
        plan_file.main(["--out", cli, "--synthetic", "--arch", "tiny", "--batch", "3", "--size", "16", "24", "--dtype", "f32", "--u8",
                        "--seeds", "5,0x10000000007,6", "--canny-per-image", "10", "20", "--device", "cpu", "--lib", emu_lib.path])
        hd = emu_lib.plan_load(cli)
        try:
            assert emu_lib.plan_io(hd, "seed")[1] == 48 and emu_lib.plan_io(hd, "canny_thr")[1] == 24
            assert rc.read_state(emu_lib.plan_read(hd, "seed", torch.zeros(12, dtype=torch.int32))) == [w_ for row in rng.pack_states([5, (1 << 40) + 7, 6]) for w_ in row]
            assert emu_lib.plan_read(hd, "canny_thr", torch.zeros(6, dtype=torch.int32)).tolist() == [10, 20] * 3
        finally:
            emu_lib.plan_destroy(hd)
        for bad in (["--seeds", "1,2"], ["--seeds", "1,2,3", "--seed", "4"], ["--seeds", "a,b,c"]):
            with pytest.raises(SystemExit):
                plan_file.main(["--out", cli + ".no", "--synthetic", "--arch", "tiny", "--batch", "3", "--size", "16", "24", "--dtype", "f32",
                                "--device", "cpu", "--lib", emu_lib.path] + bad)
        # a scalar-seed plan of the same model: 16 bytes for the whole batch, loads and runs as before
        flat = model.get_plan(bc.B, h, w, rng=True)
        flat.set_seed(9)
        spath = str(tmp_path / "scalar.i2iplan")
        assert plan_file.export_plan(flat, spath)["io"]["seed"] == 16
        want_flat = model.forward(x, caption_enc=cap, seed=9)
        hs = emu_lib.plan_load(spath)
        try:
            emu_lib.plan_write(hs, "x", x)
            emu_lib.plan_write(hs, "ctx", cap)
            emu_lib.plan_run(hs)
            assert torch.equal(emu_lib.plan_read(hs, "out", torch.zeros_like(want_flat)), want_flat)
            assert torch.equal(emu_lib.plan_read(hs, "eps", torch.zeros(bc.B, 4, h // 8, w // 8)), rng.randn((bc.B, 4, h // 8, w // 8), 9, 0, device="cpu", lib=emu_lib))
        finally:
            emu_lib.plan_destroy(hs)
    finally:
        model.release_plans()


def test_batch_host_example_builds_against_the_header(tmp_path):
    """The four C hosts under examples/ compile against the header with the additions (no library needed for -c)."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    for name in ("batch_host", "plan_host", "slider_host", "health_host"):
        subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "examples", name + ".c"),
                        "-o", str(tmp_path / (name + ".o"))], check=True)

"""Automatic per-image Canny thresholds (i2i_canny_auto_thr, csrc/resize.hip) on the CPU emulator, bit-exact against
tests/canny_auto_ref.py -- the oracle of the contract in include/i2i_turbo.h -- through the raw entry, image_ops, the planned forward, plan
files and examples/auto_canny_host.c; the edge map returned by forward_u8; Pillow's BICUBIC tables.  tests/test_canny_auto_gpu.py runs the
same cases (tests/canny_auto_cases.py) on an MI355X."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import canny_auto_cases as ac
import canny_auto_ref as ar
import canny_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the oracle itself
def test_integer_rule_matches_float_rule():
    """All 511 doubled medians at sigma 0.25 / 0.33 / 0.5: the integer form (the contract) and the float form of the rule differ by at most
    1 -- where sigma * 65536 is not an integer (0.33) the rounded sigma moves a product across an integer now and then."""
    from img2img_turbo_amd.image_ops import sigma_to_q16
    for sigma in (0.25, 0.33, 0.5):
        diffs = []
        for m2 in range(511):
            got, want = ar.thresholds(m2, sigma_to_q16(sigma)), ar.float_rule(m2, sigma)
            assert abs(got[0] - want[0]) <= 1 and abs(got[1] - want[1]) <= 1, (sigma, m2, got, want)
            if got != want:
                diffs.append((m2, got, want))
        print("[canny_auto] sigma %.2f: integer and float rule differ at %d of 511 doubled medians: %s" % (sigma, len(diffs), diffs))
        if sigma in (0.25, 0.5):                            # exact in q16: the two forms are the same function
            assert not diffs
    img = np.random.default_rng(1).integers(0, 256, (5, 6, 3), dtype=np.uint8)
    assert ar.median2(img) == int(2 * np.median(img)) and ar.median2(img[:3, :3]) == int(2 * np.median(img[:3, :3]))


def test_oracle_known_answers():
    ac.check_known_answers()


# ---------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_canny_auto_cases(emu_lib, name):
    ac.check_case(emu_lib, "cpu", name)


def test_canny_auto_errors(emu_lib):
    ac.check_errors(emu_lib, "cpu")


def test_canny_auto_abi_is_additive(emu_lib):
    ac.check_struct(emu_lib)


def test_canny_auto_eager(emu_lib):
    ac.check_eager(emu_lib, "cpu")


def test_canny_auto_program_op(emu_lib):
    ac.check_program_op(emu_lib, "cpu")


# ---------------------------------------------------------------------------------------------------------------- the planned forward
@pytest.mark.slow
def test_canny_auto_forward_plan_file_and_c_host(emu_lib, tmp_path):
    """The model class on the emulator (16 x 24 photos: a forward of the tiny model costs it a second per thousand pixels), then the plan
    exported, loaded through i2i_plan_load and run -- thresholds, edge map and image equal the Python run --, the same file through
    examples/auto_canny_host.c (gcc against the emulator library), and the command-line exporter's --canny-auto."""
    from img2img_turbo_amd import plan_file
    from img2img_turbo_amd.image_ops import sigma_to_q16
    h, w = 16, 24
    model, img, cap, eps = ac.check_forward(emu_lib, "cpu", h, w)
    try:
        imgd = torch.from_numpy(np.array(img))
        plan = model.get_plan(ac.B, h, w, u8_io=(1.0, 0.0), canny="auto")
        want_out, want_edges, want_thr = model.forward_u8(imgd, caption_enc=cap, eps=eps, canny=("auto", 0.25), return_edges=True)
        plan.set_canny_sigma(0.5)                           # what the file saves; the hosts below ask for 0.25
        path = str(tmp_path / "auto.i2iplan")
        info = plan_file.export_plan(plan, path)
        assert info["io"]["canny_sigma"] == 4 * ac.B and info["io"]["canny_median2"] == 4 * ac.B and info["io"]["canny_thr"] == 8 * ac.B
        assert info["io"]["canny_edges"] == ac.B * h * w * 3
        hd = emu_lib.plan_load(path)
        try:
            assert emu_lib.plan_read(hd, "canny_sigma", torch.zeros(ac.B, dtype=torch.int32)).tolist() == [32768] * ac.B
            emu_lib.plan_write(hd, "x", imgd)
            emu_lib.plan_write(hd, "ctx", cap.reshape(plan.ctx.shape).contiguous())
            emu_lib.plan_write(hd, "eps", eps)
            emu_lib.plan_write(hd, "canny_sigma", torch.tensor([sigma_to_q16(0.25)] * ac.B, dtype=torch.int32))
            emu_lib.plan_run(hd)
            assert torch.equal(emu_lib.plan_read(hd, "canny_thr", torch.zeros(ac.B, 2, dtype=torch.int32)), want_thr)
            assert torch.equal(emu_lib.plan_read(hd, "canny_edges", torch.zeros_like(want_edges)), want_edges)
            assert torch.equal(emu_lib.plan_read(hd, "out", torch.zeros_like(want_out)), want_out)
            med = emu_lib.plan_read(hd, "canny_median2", torch.zeros(ac.B, dtype=torch.int32))
            assert np.array_equal(ac.as_u32(med), ar.auto_thresholds(img, [16384] * ac.B)[1])
            # a manual request in the loaded plan: a negative sigma keeps the pair the host writes
            emu_lib.plan_write(hd, "canny_sigma", torch.tensor([-1, 16384, 16384], dtype=torch.int32))
            manual = want_thr.clone()
            manual[0] = torch.tensor([40, 90], dtype=torch.int32)
            emu_lib.plan_write(hd, "canny_thr", manual)
            emu_lib.plan_run(hd)
            assert torch.equal(emu_lib.plan_read(hd, "canny_thr", torch.zeros(ac.B, 2, dtype=torch.int32)), manual)
        finally:
            emu_lib.plan_destroy(hd)
        if shutil.which("gcc"):
            exe = str(tmp_path / "auto_canny_host")
            subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "auto_canny_host.c"), "-o", exe,
                            "-L", os.path.dirname(emu_lib.path), "-l" + os.path.basename(emu_lib.path)[3:-3], "-Wl,-rpath," + os.path.dirname(emu_lib.path)],
                           check=True)
            files = {}
            for name, t in (("x", imgd), ("ctx", cap.reshape(plan.ctx.shape)), ("eps", eps)):
                files[name] = str(tmp_path / (name + ".bin"))
                with open(files[name], "wb") as f:
                    f.write(t.contiguous().view(torch.uint8).numpy().tobytes())
            outs = [str(tmp_path / n) for n in ("thr.bin", "edges.bin", "out.bin")]
            env = dict(os.environ)
            env.pop("I2I_EMU_ASYNC", None)
            r = subprocess.run([exe, path, files["x"], files["ctx"], files["eps"]] + outs + ["0.25"], capture_output=True, text=True, env=env)
            assert r.returncode == 0, r.stderr
            assert "image 0: median %.1f -> low %d, high %d" % (ar.median2(img[0]) / 2.0, want_thr[0, 0], want_thr[0, 1]) in r.stdout, r.stdout
            for fn, want in zip(outs, (want_thr, want_edges, want_out)):
                with open(fn, "rb") as f:
                    assert torch.equal(torch.frombuffer(bytearray(f.read()), dtype=want.dtype).reshape(want.shape), want), fn
        # the command-line exporter
        cli = str(tmp_path / "cli.i2iplan")
        plan_file.main(["--out", cli, "--synthetic", "--arch", "tiny", "--batch", "2", "--size", "16", "24", "--dtype", "f32", "--u8",
                        "--canny-auto", "0.33", "--device", "cpu", "--lib", emu_lib.path])
        hc = emu_lib.plan_load(cli)
        try:
            assert emu_lib.plan_read(hc, "canny_sigma", torch.zeros(2, dtype=torch.int32)).tolist() == [ac.S33] * 2
            assert emu_lib.plan_io(hc, "canny_thr")[1] == 16 and emu_lib.plan_io(hc, "canny_edges")[1] == 2 * 16 * 24 * 3
        finally:
            emu_lib.plan_destroy(hc)
        for bad in (["--canny-auto", "0.33", "--canny", "1", "2"], ["--canny-auto", "1.5"]):
            with pytest.raises(SystemExit):
                plan_file.main(["--out", cli + ".no", "--synthetic", "--arch", "tiny", "--batch", "2", "--size", "16", "24", "--dtype", "f32", "--u8",
                                "--device", "cpu", "--lib", emu_lib.path] + bad)
    finally:
        model.release_plans()


def test_auto_canny_host_example_builds_against_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "examples", "auto_canny_host.c"),
                    "-o", str(tmp_path / "auto_canny_host.o")], check=True)


# ---------------------------------------------------------------------------------------------------------------- BICUBIC
def test_resample_tables(emu_lib):
    ac.check_tables(emu_lib)


@pytest.mark.parametrize("sizes", ac.BICUBIC_SIZES)
def test_bicubic_resize_matches_pillow_default(emu_lib, sizes):
    ac.check_bicubic(emu_lib, "cpu", sizes)

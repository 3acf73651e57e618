"""Per-image health (i2i_scan_batch / i2i_scan_verdict, csrc/elementwise.hip; ForwardPlan(health_per_image=True), plan.py) on the CPU emulator,
against tests/health_ref.py applied to every image's view.  tests/test_health_batch_gpu.py runs the same cases (tests/health_batch_cases.py) on
an MI355X."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import health_batch_cases as bc
import health_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["f32", "bf16", "f16"]


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_misaligned_image_starts(emu_lib, dtype):
    bc.check_misaligned(emu_lib, "cpu", dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_more_than_one_workgroup_per_image(emu_lib, dtype):
    bc.check_multi_wg(emu_lib, "cpu", dtype)


@pytest.mark.slow
@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_second_pass_of_an_image_share(emu_lib, dtype):
    bc.check_grid_pass(emu_lib, "cpu", dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_strided_views(emu_lib, dtype):
    bc.check_strided(emu_lib, "cpu", dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_boundaries(emu_lib, dtype):
    bc.check_boundaries(emu_lib, "cpu", dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_accumulation_and_neighbours(emu_lib, dtype):
    bc.check_accumulate(emu_lib, "cpu", dtype)


def test_refusals(emu_lib):
    bc.check_refusals(emu_lib, "cpu")


def test_verdict(emu_lib):
    bc.check_verdict(emu_lib, "cpu")


def test_op_layout_and_abi(emu_lib):
    from img2img_turbo_amd import _capi as K
    assert K.ABI_VERSION == 14 and emu_lib.lib.i2i_abi_version() == 14 and (K.OP_SCAN_BATCH, K.OP_SCAN_VERDICT) == (22, 23)
    assert ctypes.sizeof(K.ScanBatchParams) == 64 and ctypes.sizeof(K.ScanVerdictParams) == 32
    assert emu_lib.lib.i2i_sizeof_op() == ctypes.sizeof(K.Op) == 368                              # the union did not grow
    assert "i2i_scan_batch" in K.EXPORTS and "i2i_scan_verdict" in K.EXPORTS
    # through the program dispatcher (i2i_run): one scan_batch op between a CLEAR and a JUDGE
    from img2img_turbo_amd import ops as O
    x = torch.zeros(2, 3, 8, dtype=torch.float32)
    x[1, 2, 7] = float("inf")
    rec, ver = torch.full((2, 8), 7, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32)
    prog = K.Program()
    opc, p = O.scan_verdict(rec, ver, taps=1, images=2, mode=K.VERDICT_CLEAR)
    prog.add(opc, K.F32, p, "clear")
    opc, p = O.scan_batch(x, rec, images=2, rows=3, cols=8, limit=1.0)
    prog.add(opc, K.F32, p, "scan")
    opc, p = O.scan_verdict(rec, ver, taps=1, images=2, mode=K.VERDICT_JUDGE)
    prog.add(opc, K.F32, p, "judge")
    emu_lib.run(prog.freeze())
    assert rec.tolist() == [[1, 0, 0, 0, 0, 0, 24, 0], [1, 0, 1, 0, 0, 0, 24, 0]] and ver.tolist() == [[0, 0, 1, 0], [1, 0, 1, 1]]


# ---------------------------------------------------------------------------------------------------------------- the planned forward
@pytest.mark.slow
def test_forward_clean(emu_lib):
    bc.check_forward_clean(emu_lib, "cpu")


@pytest.mark.slow
def test_forward_one_bad_request(emu_lib):
    bc.check_forward_one_bad(emu_lib, "cpu")


def test_default_unchanged(emu_lib):
    bc.check_default_unchanged(emu_lib, "cpu")


@pytest.mark.slow
def test_plan_file_and_c_host(emu_lib, tmp_path):
    """python -m img2img_turbo_amd.plan_file --health stages --health-per-image -> i2i_plan_*: "verdict" and "health" equal the Python plan's bit
    for bit; examples/batch_health_host.c, built with gcc against the emulator library, exits 0 on the clean inputs and 3 on the batch whose
    second request carries a NaN, and names that request and its tap."""
    from img2img_turbo_amd import plan_file
    x, cap, eps = hc.tiny_inputs("cpu", bc.B, bc.H, bc.W)
    bad_eps = eps.clone()
    bad_eps[1, 0, 0, 0] = float("nan")
    path = str(tmp_path / "per_image.i2iplan")
    plan_file.main(["--out", path, "--batch", str(bc.B), "--size", str(bc.H), str(bc.W), "--dtype", "bf16", "--health", "stages", "--health-per-image",
                    "--synthetic", "--arch", "tiny", "--device", "cpu", "--lib", emu_lib.path])
    model = bc.make_model(emu_lib, "cpu")             # the same synthetic weights (seed 1234)
    plan = model.get_plan(bc.B, bc.H, bc.W)
    n = len(plan.health_labels)
    names = b"".join(l.encode() + b"\0" for l in plan.health_labels)
    info = plan_file.export_plan(plan, str(tmp_path / "twin.i2iplan"))
    assert info["io"]["health"] == 64 * n * bc.B and info["io"]["health_names"] == len(names) and info["io"]["verdict"] == 16 * bc.B
    h = emu_lib.plan_load(path)
    try:
        assert emu_lib.plan_io(h, "verdict")[1] == 16 * bc.B and emu_lib.plan_io(h, "health")[1] == 64 * n * bc.B
        assert not emu_lib.plan_read(h, "health", torch.zeros(n * bc.B, 8, dtype=torch.int64)).any()          # saved zeroed
        assert not emu_lib.plan_read(h, "verdict", torch.zeros(bc.B, 4, dtype=torch.int32)).any()
        assert bytes(emu_lib.plan_read(h, "health_names", torch.zeros(len(names), dtype=torch.uint8)).numpy()) == names
        for e in (eps, bad_eps, eps):                    # clean, one bad request, clean again: records per run, totals in the verdict
            model.stage(plan, x, cap, e)
            plan.run()
            emu_lib.plan_write(h, "x", x)
            emu_lib.plan_write(h, "ctx", cap.to(bc.DTYPE))
            emu_lib.plan_write(h, "eps", e)
            emu_lib.plan_run(h)
            got_v = emu_lib.plan_read(h, "verdict", torch.zeros(bc.B, 4, dtype=torch.int32)).numpy().view(np.uint32)
            got_r = emu_lib.plan_read(h, "health", torch.zeros(n * bc.B, 8, dtype=torch.int64)).numpy().view(np.uint64).reshape(n, bc.B, 8)
            assert np.array_equal(got_v, bc.verdict_rows(plan)) and np.array_equal(got_r, bc.records(plan))
            assert torch.equal(emu_lib.plan_read(h, "out", torch.zeros_like(plan.out)), plan.out)
        assert got_v.tolist() == [[0, 0, 3, 0], [0, 0, 3, 1], [0, 0, 3, 0]]
    finally:
        emu_lib.plan_destroy(h)
    exe = str(tmp_path / "batch_health_host")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "batch_health_host.c"), "-o", exe,
                    emu_lib.path, "-Wl,-rpath," + os.path.dirname(emu_lib.path)], check=True)
    files = {}
    for name, t in (("x", x), ("ctx", cap.to(bc.DTYPE)), ("eps", eps), ("bad_eps", bad_eps)):
        files[name] = str(tmp_path / (name + ".bin"))
        with open(files[name], "wb") as f:
            f.write(t.contiguous().view(torch.uint8).numpy().tobytes())
    at = plan.health_labels.index("latents")
    for eps_file, status in ((files["eps"], 0), (files["bad_eps"], 3)):
        r = subprocess.run([exe, path, files["x"], files["ctx"], eps_file], capture_output=True, text=True)
        assert r.returncode == status, (r.returncode, r.stdout, r.stderr)
        lines = r.stdout.strip().splitlines()
        assert len(lines) == bc.B + 1 and all(l.startswith("request %d: " % b) for b, l in enumerate(lines[:bc.B]))
        for b, l in enumerate(lines[:bc.B]):
            if status == 3 and b == 1:
                assert l.startswith("request 1: first non-finite tensor: %s " % plan.health_labels[at]) and l.endswith("runs 1 bad_runs 1"), l
            else:
                assert l.startswith("request %d: finite " % b) and l.endswith("runs 1 bad_runs 0"), l
        assert lines[-1].startswith("batch_health_host: %d of %d requests non-finite" % (1 if status else 0, bc.B))
    # a whole-batch health file has no "verdict": the host says so and exits 2
    model.release_plans()
    whole = hc.make_model(emu_lib, "cpu", bc.DTYPE, "stages")
    plan_file.export_plan(whole.get_plan(bc.B, bc.H, bc.W), str(tmp_path / "whole.i2iplan"))
    r = subprocess.run([exe, str(tmp_path / "whole.i2iplan"), files["x"], files["ctx"], files["eps"]], capture_output=True, text=True)
    assert r.returncode == 2 and "--health-per-image" in r.stderr
    whole.release_plans()

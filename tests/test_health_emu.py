"""Numerical health scan (i2i_scan, csrc/elementwise.hip; ForwardPlan(health=...), plan.py) on the CPU emulator, against tests/health_ref.py --
the oracle of the contract in include/i2i_turbo.h.  tests/test_health_gpu.py runs the same cases (tests/health_cases.py) on an MI355X."""
import os
import subprocess

import numpy as np
import pytest
import torch

import health_cases as hc
import health_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["f32", "bf16", "f16"]


def test_oracle_on_hand_made_words():
    """The oracle itself: a hand-counted fp16 row, padding ignored, widening exact."""
    row = np.array([0x7C00, 0xFC00, 0x7E00, 0x7C01, 0x8000, 0x0001, 0x3C00, 0xC400, 0x7E00, 0x7C00], dtype=np.uint16)     # last two = padding
    rec = health_ref.scan_ref(row, cols=8, ld=10, limit=2.0, fmt="f16", rows=1)
    assert rec.tolist() == [1, 2, 1, 1, 1, 0x40800000, 8, 0]                                   # -4 is the one value over 2; max |x| = 4.0
    assert health_ref.widen(np.array([1, 0x3FF, 0x400, 0x7BFF]), "f16").view(np.float32).tolist() == [2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 65504.0]
    assert health_ref.widen(np.array([0x3FC0]), "bf16").view(np.float32)[0] == 1.5
    both = health_ref.accumulate(rec, rec)
    assert both.tolist() == [2, 4, 2, 2, 2, 0x40800000, 16, 0]


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_scan_small_views(emu_lib, dtype):
    hc.check_small(emu_lib, "cpu", dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_scan_classes(emu_lib, dtype):
    hc.check_classes(emu_lib, "cpu", dtype)


@pytest.mark.slow
@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_scan_strides(emu_lib, dtype):
    hc.check_strides(emu_lib, "cpu", dtype)


def test_scan_refusals(emu_lib):
    hc.check_refusals(emu_lib, "cpu")


def test_op_layout_and_abi(emu_lib):
    from img2img_turbo_amd import _capi as K
    assert K.ABI_VERSION == 14 and emu_lib.lib.i2i_abi_version() == 14 and K.OP_SCAN == 18
    import ctypes
    assert ctypes.sizeof(K.ScanParams) == 48 and ctypes.sizeof(K.ScanParams) < ctypes.sizeof(K.IgemmParams)      # the union did not grow
    assert emu_lib.lib.i2i_sizeof_op() == ctypes.sizeof(K.Op) == 8 + ctypes.sizeof(K.IgemmParams)


# ---------------------------------------------------------------------------------------------------------------- the planned forward
@pytest.fixture(scope="module")
def forward_trio(emu_lib):
    """One tiny fp16 forward three ways, shared by the tests below: health="all", health=None, and the debug twin that keeps every
    intermediate.  (debug=True switches the GroupNorm statistics epilogues off; the other two plans do the same, so the three programs
    differ by the scan ops alone.)"""
    x, cap, eps = hc.tiny_inputs("cpu")
    dt = torch.float16
    out = {}
    for name, health, opts in (("all", "all", dict(fuse_gn_stats=False)), ("none", None, dict(fuse_gn_stats=False)), ("twin", "all", dict(debug=True))):
        m = hc.make_model(emu_lib, "cpu", dt, health, **opts)
        y = m(x, caption_enc=cap, eps=eps)
        out[name] = (m, m._last_plan if health else list(m._plans.values())[0], y)
    yield out
    for m, _, _ in out.values():
        m.release_plans()


@pytest.mark.slow
def test_forward_output_and_program_unchanged(forward_trio):
    (_, pa, ya), (_, pn, yn), (_, _, yt) = forward_trio["all"], forward_trio["none"], forward_trio["twin"]
    assert torch.equal(ya, yn) and torch.equal(ya, yt)
    from img2img_turbo_amd import _capi as K
    plain = [(o, l) for (o, _, _, l) in pa.prog.ops if o != K.OP_SCAN]
    assert plain == [(o, l) for (o, _, _, l) in pn.prog.ops]                  # the scans are insertions: nothing else moved
    assert pn.health_rec is None and not pn.health_labels and all(o != K.OP_SCAN for o, _, _, _ in pn.prog.ops)
    assert pa.pool.bytes == pn.pool.bytes                                    # no activation memory of their own


@pytest.mark.slow
def test_forward_labels(forward_trio):
    m, plan, _ = forward_trio["all"]
    labels = plan.health_labels
    assert plan.health_rec.shape == (len(labels), 8) and plan.health_rec.dtype == torch.uint64
    # program order: label i belongs to the i-th scan op of the program, which sits right behind the op of that name
    from img2img_turbo_amd import _capi as K
    scans = [(i, l) for i, (o, _, _, l) in enumerate(plan.prog.ops) if o == K.OP_SCAN]
    assert [l for _, l in scans] == ["health: " + l for l in labels]
    for i, l in scans:
        name = l[len("health: "):]
        if name in plan.taps:
            assert plan.prog.ops[i - 1][3] in (name, "health: " + name) or plan.prog.ops[i - 1][0] == K.OP_SCAN, (name, plan.prog.ops[i - 1][3])
    assert set(plan.taps) <= set(labels)
    stages = hc.stage_names(m.weights)
    assert [l for l in labels if l in stages] == stages                       # every stage boundary, in order
    # "stages" alone: planning needs no run
    from img2img_turbo_amd.plan import ForwardPlan
    ps = ForwardPlan(m.lib, m.weights, 1, 16, 24, torch.float16, "cpu", health="stages", packers=m._get_packers("a2b"))
    assert ps.health_labels == stages
    dts = {l: str(t.dtype) for l, (t, _, _, _) in zip(ps.health_labels, ps.health_taps)}
    assert dts["moments"] == dts["latents"] == dts["eps_prediction"] == "torch.float32" and dts["post_quant"] == "torch.float16"
    ps.release()


@pytest.mark.slow
def test_forward_records(forward_trio):
    (m, plan, _), (_, twin, _) = forward_trio["all"], forward_trio["twin"]
    assert plan.health_labels == twin.health_labels
    rec, rec_t = hc.records(plan), hc.records(twin)
    rep = m.health_report()
    stale = 0
    for i, label in enumerate(plan.health_labels):
        t, rows, cols, _ = plan.health_taps[i]
        want = hc.ref_of_tap(twin, i)
        assert rec[i][0] == 1 and rec[i][6] == rows * cols, label
        assert np.array_equal(rec[i], rec_t[i]), label
        if hc.overwritten_later(twin, i):          # (the decoder adds its skip convolutions in place: the twin holds the sum, the scan saw the addend)
            stale += 1
            want = rec[i]
        assert np.array_equal(rec[i], want), (label, rec[i].tolist(), want.tolist())
        d = rep[i]
        assert (d["label"], d["runs"], d["elements"], d["n_nan"]) == (label, 1, rows * cols, int(want[1]))
        assert np.float32(d["max_abs"]).view(np.uint32) == want[5] and d["dtype"] == str(t.dtype).replace("torch.", "")
    assert stale <= 2 * len(plan.va.block_out_channels)          # one conv tap + one stage tap per in-place skip convolution at most
    assert m.health_first_bad() is None
    # accumulation over a second run, then the reset
    plan.run()
    rec2 = hc.records(plan)
    assert all(rec2[i][0] == 2 and rec2[i][6] == 2 * rec[i][6] and rec2[i][5] == rec[i][5] for i in range(len(rec)))
    m.health_reset()
    assert not hc.records(plan).any()


@pytest.mark.slow
def test_poison(emu_lib):
    hc.check_poison(emu_lib, "cpu")


@pytest.mark.slow
def test_plan_file_and_c_host(emu_lib, tmp_path):
    """export -> i2i_plan_*: "health" equals the in-process records, "health_names" the labels; examples/health_host.c, built with gcc against
    the emulator library, exits 3 on the poisoned fp16 file and names the tap (and exits 0 on the bf16 one)."""
    from img2img_turbo_amd import plan_file
    x, cap, eps = hc.tiny_inputs("cpu")
    wts = hc.tiny_weights(poison=True)
    exe = str(tmp_path / "health_host")
    libdir = os.path.dirname(emu_lib.path)
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "health_host.c"), "-o", exe,
                    emu_lib.path, "-Wl,-rpath," + libdir], check=True)
    for dtype, tag, status in ((torch.float16, "f16", 3), (torch.bfloat16, "bf16", 0)):
        model = hc.make_model(emu_lib, "cpu", dtype, "stages", weights=wts)
        model(x, caption_enc=cap, eps=eps)
        plan = model._last_plan
        want = hc.records(plan)
        first = model.health_first_bad()          # (before the export: it zeroes the records it saves)
        path = str(tmp_path / ("health_%s.i2iplan" % tag))
        info = plan_file.export_plan(plan, path)
        n = len(plan.health_labels)
        names = b"".join(l.encode() + b"\0" for l in plan.health_labels)
        assert info["io"]["health"] == 64 * n and info["io"]["health_names"] == len(names)
        h = emu_lib.plan_load(path)
        try:
            assert not emu_lib.plan_read(h, "health", torch.zeros(n, 8, dtype=torch.int64)).any()          # saved zeroed
            assert bytes(emu_lib.plan_read(h, "health_names", torch.zeros(len(names), dtype=torch.uint8)).numpy()) == names
            emu_lib.plan_write(h, "x", x)
            emu_lib.plan_write(h, "ctx", cap.to(dtype))
            emu_lib.plan_write(h, "eps", eps)
            emu_lib.plan_run(h)
            got = emu_lib.plan_read(h, "health", torch.zeros(n, 8, dtype=torch.int64)).numpy().view(np.uint64)
            assert np.array_equal(got, want)
        finally:
            emu_lib.plan_destroy(h)
        files = {}
        for name, t in (("x", x), ("ctx", cap.to(dtype)), ("eps", eps)):
            files[name] = str(tmp_path / (name + "_" + tag + ".bin"))
            with open(files[name], "wb") as f:
                f.write(t.contiguous().view(torch.uint8).numpy().tobytes())
        r = subprocess.run([exe, path, files["x"], files["ctx"], files["eps"]], capture_output=True, text=True)
        assert r.returncode == status, (r.returncode, r.stdout, r.stderr)
        lines = r.stdout.strip().splitlines()
        assert len(lines) == n + 1 and [l.split()[0] for l in lines[:n]] == plan.health_labels
        assert not hc.records(plan).any()
        if status == 3:
            assert first is not None and lines[-1] == "health_host: first non-finite tensor: " + first["label"]
            assert first["label"] == "decoder.up_blocks.1"            # the stage that holds the poisoned convolution
        else:
            assert first is None and "all finite" in lines[-1]
        model.release_plans()

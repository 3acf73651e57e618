"""The LoRA scale as device state for every host, on the CPU emulator: TwinConv fold kernel, grouped merge, the scale program of a
live_scale model, plan files with a scale program and the C slider host (tests/scale_cases.py has the cases and the checks)."""
import os
import shutil
import struct
import subprocess

import pytest
import torch

import scale_cases as S

H, W = 24, 40          # a latent of 3 x 5: the emulator needs about a second per thousand pixels of a forward


@pytest.mark.parametrize("dt", [S.F32, S.BF16, S.F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", S.TWIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_twin_fold_against_fp64(emu_lib, shape, dt):
    worst = S.check_twin(emu_lib, "cpu", shape, dt)
    print("[twin_fold] %s dtype %d: worst %s = %.3f" % (shape, dt, "err / bound" if dt == S.F32 else "steps from the exact rounding", worst))


def test_twin_fold_abi(emu_lib):
    S.check_twin_abi(emu_lib, "cpu")


@pytest.mark.parametrize("dt", [S.F32, S.BF16, S.F16], ids=["f32", "bf16", "f16"])
def test_grouped_merge_is_six_per_layer_merges(emu_lib, dt):
    S.check_group(emu_lib, "cpu", dt)


def test_grouped_merge_abi(emu_lib):
    S.check_group_abi(emu_lib, "cpu")


@pytest.mark.slow
def test_live_scale_equals_the_per_layer_path(emu_lib):
    S.check_live_equals_per_layer(emu_lib, "cpu", H, W)


@pytest.mark.slow
def test_twinconv_live_scale_against_the_oracle_bf16(emu_lib):
    """The TwinConv checkpoint with the fold on the device, against the CPU oracle under the gate of
    tests/test_e2e_emu.py::test_pix2pix_stochastic_twinconv_bf16; set_scale on this path calls no host refold."""
    from oracle.pipeline import pix2pix_forward
    x, cap, eps, nm = S.model_inputs("cpu", 64, 64)
    mw, model = S.make_model(emu_lib, "cpu", sketch=True, dtype=torch.bfloat16, live_scale=True)
    for r in (0.3, 1.0):
        ref = pix2pix_forward(mw, x, cap, eps, deterministic=False, r=r, noise_map=nm)
        out = model(x, caption_enc=cap, eps=eps, deterministic=False, r=r, noise_map=nm)
        err = (out.float() - ref).abs().max().item()
        print("[live_scale twinconv bf16] r = %.1f: max-abs vs oracle %.4f" % (r, err))
        assert err < 0.25, err   # bf16 end-to-end, x14.6 scheduler amplification
    pu = model._packer("unet")
    assert pu._twin is not None and all(not pk._refolds for pk in model._packers.values())
    assert pu.scale_program().prog.labels[-1] == "scale.twin_fold"


@pytest.fixture(scope="module")
def live_file(emu_lib, tmp_path_factory):
    return S.check_plan_round_trip(emu_lib, "cpu", tmp_path_factory.mktemp("live_plan"), H, W)


@pytest.mark.slow
def test_plan_file_set_scale_round_trip(live_file):
    assert os.path.getsize(live_file["path"]) > 0


@pytest.mark.slow
def test_plan_file_without_the_flag_is_v1_and_refuses_set_scale(emu_lib, live_file, tmp_path):
    from img2img_turbo_amd import _capi as K
    from img2img_turbo_amd.plan_file import export_plan
    path = str(tmp_path / "fixed.i2iplan")
    info = export_plan(live_file["plan"], path)
    assert info["scale_ops"] == 0
    with open(path, "rb") as f:
        assert f.read(8) == b"I2IPLAN1"
    h = emu_lib.plan_load(path)
    try:
        assert not emu_lib.plan_has_scale(h)
        assert emu_lib.lib.i2i_plan_set_scale(h, 0.4, 0.4, None) == S.UNSUPPORTED
        assert "no scale program" in emu_lib.lib.i2i_last_error().decode()
        with pytest.raises(K.I2IError):
            emu_lib.plan_set_scale(h, 0.4)
        S.feed(emu_lib, h, live_file["plan"], live_file["x"], live_file["cap"], live_file["eps"], live_file["nm"])
        emu_lib.plan_run(h)
        got = emu_lib.plan_read(h, "out", torch.empty_like(live_file["plan"].out))
        assert torch.equal(got, live_file["out1"])                  # the export scale, merged into the weights
    finally:
        emu_lib.plan_destroy(h)
    # a model that folds its TwinConv on the host has no fold op to give to a C host
    _, host_fold = S.make_model(emu_lib, "cpu", sketch=True, live_scale=False)
    plan = host_fold.get_plan(1, H, W, stochastic=True, r=0.4)
    with pytest.raises(K.I2IError, match="live_scale=True"):
        export_plan(plan, path, live_scale=True)


@pytest.mark.slow
def test_damaged_v2_files_are_rejected(emu_lib, live_file, tmp_path):
    from img2img_turbo_amd import _capi as K
    with open(live_file["path"], "rb") as f:
        blob = f.read()
    n_ops, _n_bufs, n_relocs, _n_io, n_scale, rel0 = S.header_fields(blob)
    assert n_scale > 0
    damaged = {}
    for name, count in (("one_more", n_scale + 1), ("many_more", n_scale + 5000), ("huge", 0xFFFFFFFF)):      # scale-op count beyond the table
        b = bytearray(blob)
        struct.pack_into("<I", b, 32, count)
        damaged["count_" + name] = b
    # a relocation of a scale op moved onto a non-pointer field of its parameter struct (lora_merge.N / twin_fold.N)
    n_off = {K.OP_LORA_MERGE: K.Op.u.offset + K.LoraMergeParams.N.offset, K.OP_TWIN_FOLD: K.Op.u.offset + K.TwinFoldParams.N.offset}
    ops0 = rel0 + 24 * n_relocs
    hit = set()
    for i in range(n_relocs):
        op = struct.unpack_from("<I", blob, rel0 + 24 * i)[0]
        if op < n_ops:
            continue
        opcode = struct.unpack_from("<i", blob, ops0 + op * K.C.sizeof(K.Op))[0]
        if opcode in hit:
            continue
        hit.add(opcode)
        b = bytearray(blob)
        struct.pack_into("<I", b, rel0 + 24 * i + 4, n_off[opcode])
        damaged["reloc_opcode_%d" % opcode] = b
    assert hit == {K.OP_LORA_MERGE, K.OP_TWIN_FOLD}
    b = bytearray(blob)                                   # a scale program may only hold merges and folds
    struct.pack_into("<i", b, ops0 + n_ops * K.C.sizeof(K.Op), K.OP_NOP)
    damaged["foreign_scale_op"] = b
    damaged["truncated"] = blob[:len(blob) - 100]
    for name, b in damaged.items():
        p = str(tmp_path / (name + ".i2iplan"))
        with open(p, "wb") as f:
            f.write(bytes(b))
        with pytest.raises(K.I2IError):
            emu_lib.plan_load(p)
    assert emu_lib.plan_load(live_file["path"])           # the undamaged file still loads (the handle is left to the process)


@pytest.mark.slow
def test_slider_host_example(emu_lib, live_file, tmp_path):
    """examples/slider_host.c, built with the host C compiler against the emulator library and run as a child process at r = 0.4 and 1.0:
    its two output files are the Python model's outputs byte for byte."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert shutil.which("gcc"), "no host C compiler"
    exe = str(tmp_path / "slider_host")
    lib = emu_lib.path
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "slider_host.c"), "-o", exe,
                    "-L", os.path.dirname(lib), "-l" + os.path.basename(lib)[3:-3], "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    plan = live_file["plan"]
    files = {}
    for name, t in (("x", live_file["x"].to(plan.x_in.dtype)), ("ctx", live_file["cap"].to(plan.ctx.dtype).reshape(plan.ctx.shape)),
                    ("eps", live_file["eps"].to(plan.eps.dtype)), ("noise", live_file["nm"].to(plan.noise.dtype).expand_as(plan.noise))):
        files[name] = str(tmp_path / (name + ".bin"))
        with open(files[name], "wb") as f:
            f.write(t.contiguous().view(torch.uint8).numpy().tobytes())
    env = dict(os.environ)
    env.pop("I2I_EMU_ASYNC", None)
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, live_file["path"], files["x"], files["ctx"], files["eps"], files["noise"], prefix, "0.4", "1.0"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    for i, want in enumerate((live_file["out04"], live_file["out1"])):
        with open("%s_%d.bin" % (prefix, i), "rb") as f:
            assert f.read() == want.to(plan.out.dtype).contiguous().view(torch.uint8).numpy().tobytes(), "slider_host output %d differs from the Python model" % i
    # a v1 file is refused with a message, not run at the wrong scale
    from img2img_turbo_amd.plan_file import export_plan
    v1 = str(tmp_path / "fixed.i2iplan")
    export_plan(plan, v1)
    r = subprocess.run([exe, v1, files["x"], files["ctx"], files["eps"], files["noise"], prefix, "0.4"], capture_output=True, text=True, env=env)
    assert r.returncode == 2 and "no scale program" in r.stderr

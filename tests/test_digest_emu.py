"""Device fingerprints (i2i_digest, csrc/elementwise.hip; ForwardPlan(fingerprint=...), plan.py; the digest section of plan files and
i2i_plan_verify, csrc/plan_file.hip) on the CPU emulator, bit for bit against tests/digest_ref.py.  tests/test_digest_gpu.py runs the same
cases (tests/digest_cases.py) on an MI355X."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import digest_cases as dc
import digest_ref as R
import health_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixer_avalanche():
    """The oracle alone: flipping any of the 96 input bits of (j, v) flips every one of the 128 output bits of (H0, H1) with a frequency in
    [0.4, 0.6] over 4096 random inputs (a fair coin's standard deviation there is 0.0078: the band is twelve of them wide on each side)."""
    rs = np.random.RandomState(20240)
    n = 4096
    j = (rs.randint(0, 2 ** 32, size=n, dtype=np.int64).astype(np.uint64) << np.uint64(32)) | rs.randint(0, 2 ** 32, size=n, dtype=np.int64).astype(np.uint64)
    v = rs.randint(0, 2 ** 32, size=n, dtype=np.int64).astype(np.uint32)
    h0, h1 = R.mix(j, v)
    assert not np.array_equal(h0, h1)
    shifts = np.arange(64, dtype=np.uint64)
    for bit in range(96):
        a0, a1 = R.mix(j ^ np.uint64(1 << bit), v) if bit < 64 else R.mix(j, v ^ np.uint32(1 << (bit - 64)))
        for name, d in (("H0", h0 ^ a0), ("H1", h1 ^ a1)):
            freq = ((d[:, None] >> shifts[None, :]) & np.uint64(1)).mean(axis=0)
            assert freq.min() >= 0.4 and freq.max() <= 0.6, (bit, name, float(freq.min()), float(freq.max()))


def test_oracle_identities():
    """What the contract says follows from it, on the oracle: pieces add up, pitch and pads do not matter, position matters."""
    flat = dc.words(1000, 2, 1)
    whole = R.digest_ref(flat, 1, 1000)
    assert np.array_equal(whole, R.add(R.digest_ref(flat[:333], 1, 333), R.digest_ref(flat[333:], 1, 667, index0=333)))
    assert np.array_equal(whole, R.digest_ref(flat, 25, 40)) and whole[2] == 1000 and whole[3] == 0
    assert not np.array_equal(whole, R.digest_ref(flat[::-1].copy(), 1, 1000))


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_lengths_and_alignments(emu_lib, fmt):
    dc.check_lengths(emu_lib, "cpu", fmt)


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_pitched_rows(emu_lib, fmt):
    dc.check_pitched(emu_lib, "cpu", fmt)


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_several_images(emu_lib, fmt):
    dc.check_images(emu_lib, "cpu", fmt)


@pytest.mark.slow
def test_capped_grid_second_pass(emu_lib):
    dc.check_capped_grid(emu_lib, "cpu")


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_index_carry(emu_lib, fmt):
    dc.check_index_carry(emu_lib, "cpu", fmt)


@pytest.mark.parametrize("fmt", dc.FMTS)
def test_piecewise_identity(emu_lib, fmt):
    dc.check_piecewise(emu_lib, "cpu", fmt)


def test_accumulate_and_clear(emu_lib):
    dc.check_accumulate_clear(emu_lib, "cpu")


def test_sensitivity_every_bit(emu_lib):
    dc.check_sensitivity(emu_lib, "cpu", every_bit=True)


def test_refusals_and_no_ops(emu_lib):
    dc.check_refusals(emu_lib, "cpu")


def test_eager_digest_and_first_diff(emu_lib):
    dc.check_eager(emu_lib, "cpu")


def test_op_layout_and_abi(emu_lib):
    from img2img_turbo_amd import _capi as K
    from img2img_turbo_amd import ops as O
    assert K.ABI_VERSION == 14 and emu_lib.lib.i2i_abi_version() == 14 and K.OP_DIGEST == 25
    assert ctypes.sizeof(K.DigestParams) == 72
    assert emu_lib.lib.i2i_sizeof_op() == ctypes.sizeof(K.Op) == 368                              # the union did not grow
    assert "i2i_digest" in K.EXPORTS and "i2i_plan_verify" in K.EXPORTS
    # through the program dispatcher (i2i_run): CLEAR, then two images of an fp32 tensor
    x = torch.arange(48, dtype=torch.float32).reshape(2, 3, 8)
    rec = torch.full((3, 4), 7, dtype=torch.int64)
    prog = K.Program()
    opc, p = O.digest_clear(rec, n_records=2)
    prog.add(opc, K.F32, p, "clear")
    opc, p = O.digest(x, rec, images=2, rows=3, cols=8)
    prog.add(opc, K.F32, p, "digest")
    emu_lib.run(prog.freeze())
    assert np.array_equal(rec.numpy().view(np.uint64)[:2], R.digest_batch_ref(R.bits_of(x), 2, 3, 8)) and rec[2].tolist() == [7, 7, 7, 7]


# ---------------------------------------------------------------------------------------------------------------- the planned forward
def test_default_unchanged(emu_lib):
    dc.check_default_unchanged(emu_lib, "cpu")


@pytest.mark.slow
def test_forward_repeatable(emu_lib):
    dc.check_repeatable(emu_lib, "cpu", graph=False)


@pytest.mark.slow
def test_forward_images_independent(emu_lib):
    dc.check_images_independent(emu_lib, "cpu")


def test_weights_fingerprint_follows_the_scale(emu_lib):
    dc.check_weights_fingerprint(emu_lib, "cpu")


@pytest.mark.slow
def test_io_labels(emu_lib):
    dc.check_io(emu_lib, "cpu")


# ---------------------------------------------------------------------------------------------------------------- plan files
def test_plan_verify(emu_lib, tmp_path):
    dc.check_plan_verify(emu_lib, "cpu", tmp_path)


@pytest.mark.slow
def test_plan_file_fingerprint_and_c_host(emu_lib, tmp_path):
    """--fingerprint stages through i2i_plan_*, then examples/fingerprint_host.c built with gcc against the emulator library: it verifies the
    file, prints one line per tap and image, and with --twice exits 0; on a file with a flipped weight byte it exits 4."""
    path = dc.check_plan_file_fingerprint(emu_lib, "cpu", tmp_path)
    exe = str(tmp_path / "fingerprint_host")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "fingerprint_host.c"), "-o", exe,
                    emu_lib.path, "-Wl,-rpath," + os.path.dirname(emu_lib.path)], check=True)
    x, cap, eps = hc.tiny_inputs("cpu", dc.B, dc.H, dc.W)
    files = {}
    for name, t in (("x", x), ("ctx", cap.to(dc.DTYPE)), ("eps", eps)):
        files[name] = str(tmp_path / (name + ".bin"))
        with open(files[name], "wb") as f:
            f.write(t.contiguous().view(torch.uint8).numpy().tobytes())
    model = dc.make_model(emu_lib, "cpu", "stages")
    want, _ = dc.forward(model, x, cap, eps)
    r = subprocess.run([exe, path, files["x"], files["ctx"], files["eps"], "--twice"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = [l for l in r.stdout.splitlines() if l.startswith("tap ")]
    assert len(lines) == len(want) * dc.B
    for i, (label, rec) in enumerate(want):
        for b in range(dc.B):
            s0, s1, n = (int(v) & (2 ** 64 - 1) for v in rec.view(torch.int64)[b, :3].tolist())
            assert lines[i * dc.B + b] == "tap %s image %d: %016x %016x elements %d" % (label, b, s0, s1, n), lines[i * dc.B + b]
    assert "verified" in r.stdout
    at, recs = dc.digest_section(path)
    victim = max(recs, key=lambda q: q[4])
    raw = bytearray(open(path, "rb").read())
    raw[dc.buffer_table(path)[victim[0]][2] + 3] ^= 1
    bad = str(tmp_path / "bad.i2iplan")
    open(bad, "wb").write(bytes(raw))
    r = subprocess.run([exe, bad, files["x"], files["ctx"], files["eps"]], capture_output=True, text=True)
    assert r.returncode == 4 and ("buffer %d" % victim[0]) in r.stderr, (r.returncode, r.stdout, r.stderr)
    model.release_plans()

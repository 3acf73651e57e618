"""Canny edge detection (i2i_canny_u8, csrc/resize.hip) on the CPU emulator, bit-exact against tests/canny_ref.py -- the oracle of the
contract in include/i2i_turbo.h -- plus the oracle's own hand-checked known answers and, where OpenCV is installed, the pin against
cv2.Canny.  tests/test_canny_gpu.py runs the same cases (tests/canny_cases.py) on an MI355X."""
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

import canny_cases as cc
import canny_ref


# ---------------------------------------------------------------------------------------------------------------- 1. the oracle itself
def test_oracle_known_answers():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 11, 2), dtype=np.uint8)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    dx, dy = canny_ref.sobel(img)
    for ch in range(2):
        plane = img[..., ch].astype(np.int64)
        assert np.array_equal(dx[..., ch], ndimage.correlate(plane, kx, mode="nearest"))
        assert np.array_equal(dy[..., ch], ndimage.correlate(plane, kx.T, mode="nearest"))
    # a vertical step 0 | 200: columns 7 and 8 carry the same magnitude (800); `m > left && m >= right` keeps the LEFT one only
    gray = np.zeros((16, 16), dtype=np.uint8)
    gray[:, 8:] = 200
    _, _, mag = canny_ref.gradient(gray[..., None])
    assert (mag[:, 7] == 800).all() and (mag[:, 8] == 800).all() and mag[:, :7].max() == 0 and mag[:, 9:].max() == 0
    e = canny_ref.canny(gray)
    want = np.zeros((16, 16), dtype=np.uint8)
    want[:, 7] = 255
    assert e.shape == (16, 16, 1) and np.array_equal(e[..., 0], want)
    assert np.array_equal(canny_ref.canny(gray, out_channels=3), np.repeat(want[..., None], 3, axis=2))
    # a constant image has no edges
    assert not canny_ref.canny(np.full((16, 16, 3), 93, dtype=np.uint8)).any()
    # a step in channel 2 only: the pixel takes that channel's gradient
    rgb = np.zeros((16, 16, 3), dtype=np.uint8)
    rgb[..., 2] = gray
    assert np.array_equal(canny_ref.canny(rgb)[..., 0], want)
    # a tie between channels goes to the lowest index: equal magnitudes, opposite signs of dx
    tie = np.zeros((16, 16, 2), dtype=np.uint8)
    tie[..., 0] = gray
    tie[..., 1] = 200 - gray
    gdx, _, gmag = canny_ref.gradient(tie)
    assert (gmag[:, 7] == 800).all() and (gdx[:, 7] == 800).all()          # channel 0's +800, not channel 1's -800
    # hysteresis: a weak-only component is dropped, a weak one touching a strong pixel (diagonally) is kept
    cls = np.zeros((6, 8), dtype=np.uint8)
    cls[1, 1:4] = 1
    cls[2, 4] = 2
    cls[4, 0:3] = 1
    keep = canny_ref.hysteresis(cls)
    assert keep[1, 1:4].all() and keep[2, 4] and not keep[4].any() and keep.sum() == 4
    assert canny_ref.thresholds(200.7, 100.2) == (100, 200)


# ---------------------------------------------------------------------------------------------------------------- 2. - 5. the kernels
@pytest.mark.parametrize("key,out_c", cc.SIZE_CASES)
def test_canny_sizes(emu_lib, key, out_c):
    cc.check_sizes(emu_lib, "cpu", key, out_c)


def test_canny_long_chain_across_tiles(emu_lib):
    cc.check_snakes(emu_lib, "cpu")


def test_canny_thresholds_and_dirty_workspace(emu_lib):
    cc.check_thresholds(emu_lib, "cpu")


def test_canny_abi(emu_lib):
    cc.check_abi(emu_lib, "cpu")


def test_canny_program_op(emu_lib):
    """The op through i2i_run (capi.hip's dispatch), as a plan records it."""
    from img2img_turbo_amd import _capi as K, ops as O
    img = cc.to_dev(cc.IMAGES["noise_37x53x3"](), "cpu")
    n, h, w, c = img.shape
    dst = torch.zeros(n, h, w, 3, dtype=torch.uint8)
    ws = torch.empty(emu_lib.canny_ws_bytes(n, h, w), dtype=torch.uint8)
    prog = K.Program()
    opcode, params = O.canny_u8(img, dst, ws, n=n, h=h, w=w, c=c, out_c=3, low=100, high=200)
    prog.add(opcode, K.F32, params, "canny")
    emu_lib.run(prog.freeze())
    assert np.array_equal(dst.numpy(), cc.oracle("noise_37x53x3"))


# ---------------------------------------------------------------------------------------------------------------- 6. the pipeline
@pytest.mark.slow
def test_canny_pipeline_and_plan_file(emu_lib, tmp_path):
    """photo -> LANCZOS resize -> Canny -> generator -> uint8 image as one program, against the host twin (Pillow + the oracle); then the
    exported plan (plan_file --canny) reloaded through i2i_plan_load, fed "x" and "canny_thr", against the Python result."""
    from img2img_turbo_amd import arch, plan_file
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.synth import make_pix2pix_weights
    w = make_pix2pix_weights(arch.TINY_UNET, arch.TINY_VAE, seed=1234)          # (the weights plan_file --synthetic --arch tiny makes)
    model = Pix2Pix_Turbo(weights=w, device="cpu", dtype=torch.float32, lib=emu_lib)
    img, cap, eps, outs = cc.check_pipeline(emu_lib, "cpu", model, n=1, h=37, w=45)
    # the command-line exporter; the thresholds saved in the file are NOT the ones the host then asks for
    path = str(tmp_path / "canny.i2iplan")
    plan_file.main(["--out", path, "--synthetic", "--arch", "tiny", "--batch", "1", "--size", "32", "40", "--dtype", "f32", "--u8",
                    "--canny", "10", "20", "--device", "cpu", "--lib", emu_lib.path])
    with pytest.raises(SystemExit):
        plan_file.main(["--out", path + ".no", "--synthetic", "--arch", "tiny", "--canny", "10", "20", "--device", "cpu", "--lib", emu_lib.path])
    from PIL import Image
    resized = np.stack([np.asarray(Image.fromarray(im, "RGB").resize((40, 32), Image.LANCZOS)) for im in img])
    h = emu_lib.plan_load(path)
    try:
        assert emu_lib.plan_io(h, "canny_thr")[1] == 8
        emu_lib.plan_write(h, "x", torch.from_numpy(resized))
        emu_lib.plan_write(h, "ctx", cap.reshape(1, 77, -1).contiguous())
        emu_lib.plan_write(h, "eps", eps)
        saved = emu_lib.plan_read(h, "canny_thr", torch.zeros(2, dtype=torch.int32))
        assert saved.tolist() == [10, 20]
        thr = (40, 90)
        emu_lib.plan_write(h, "canny_thr", torch.tensor(thr, dtype=torch.int32))
        emu_lib.plan_run(h)
        got = emu_lib.plan_read(h, "out", torch.zeros(1, 32, 40, 3, dtype=torch.uint8))
        assert torch.equal(got, outs[thr]), thr
    finally:
        emu_lib.plan_destroy(h)


def test_plan_host_example_builds_against_the_header(tmp_path):
    """examples/plan_host.c still compiles against the v11 header (no library needed for -c)."""
    import shutil
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-c", os.path.join(root, "examples", "plan_host.c"),
                    "-o", str(tmp_path / "plan_host.o")], check=True)


# ---------------------------------------------------------------------------------------------------------------- 7. the pin
def test_oracle_matches_opencv():
    """Where OpenCV exists, the oracle (and with it the contract) is pinned against cv2.Canny.  If this fails, tests/canny_ref.py and the
    contract in include/i2i_turbo.h are what is wrong, not OpenCV."""
    cv2 = pytest.importorskip("cv2")
    keys = sorted({k for k, _ in cc.SIZE_CASES}) + ["snake", "snake_seedless", "two_snakes"]
    for key in keys:
        for im, want in zip(cc.IMAGES[key](), cc.oracle(key, 100, 200, 1)):
            src = np.ascontiguousarray(im if im.shape[2] > 1 else im[..., 0])
            assert np.array_equal(cv2.Canny(src, 100, 200), want[..., 0]), key

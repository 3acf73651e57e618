"""JPEG encoding on the device, on an MI355X: the cases of tests/test_jpeg_emu.py (shared through tests/jpeg_cases.py) with valid
descriptors only, both model classes, and one timing line."""
import io

import numpy as np
import pytest
import torch

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
SIZE_IDS = ["%dx%d" % s for s in jc.SIZES]


def test_jpeg_abi_is_additive(gpu_lib):
    jc.check_abi(gpu_lib)


def test_jpeg_header_host_code(gpu_lib):
    jc.check_header(gpu_lib)


@pytest.mark.parametrize("size", jc.SIZES, ids=SIZE_IDS)
def test_jpeg_grid(gpu_lib, size):
    jc.check_grid(gpu_lib, "cuda", *size)


def test_jpeg_ragged_batch(gpu_lib):
    jc.check_ragged_batch(gpu_lib, "cuda")


def test_jpeg_grid_independence(gpu_lib):
    jc.check_grid_independence(gpu_lib, "cuda")


def test_jpeg_overflow_is_flagged(gpu_lib):
    jc.check_overflow(gpu_lib, "cuda")


def test_jpeg_bad_args(gpu_lib):
    jc.check_bad_args(gpu_lib, "cuda")


@pytest.mark.parametrize("kind", ["pix2pix", "cyclegan"])
def test_jpeg_forward_u8(gpu_lib, kind):
    jc.check_forward_jpeg(gpu_lib, "cuda", kind)


def test_jpeg_forward_u8_bf16(gpu_lib):
    jc.check_forward_jpeg(gpu_lib, "cuda", "pix2pix", torch.bfloat16)


def test_jpeg_timing_line(gpu_lib):
    """8 x 512 x 512 x 3 at quality 90, both subsamplings, on output-like content (Lanczos-upscaled noise, as the resize timing uses): the
    encode call as ONE captured graph (torch.cuda.graph around the eager entry; one warm-up, the median of 10 replays, HIP events), printed
    beside Image.save of the same eight arrays on one host thread plus the device-to-host copy of the raw batch.  Print only; asserted: the
    graph's files equal Pillow's (the oracle's where Pillow has no JPEG), and a replay after the pixels changed in place follows them."""
    import ctypes as C
    import time
    from img2img_turbo_amd import image_ops, ops as O
    n, h, w, q = 8, 512, 512, 90
    g = torch.Generator().manual_seed(5)
    small = torch.randint(0, 256, (n, 64, 64, 3), generator=g, dtype=torch.uint8).cuda()
    x = image_ops.lanczos_resize_u8(small, (w, h), gpu_lib).contiguous()
    host = x.cpu().numpy()

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sorted(ms)

    def pillow_all(arrays, s):
        from PIL import Image
        out = []
        for a in arrays:
            f = io.BytesIO()
            Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s)
            out.append(f.getvalue())
        return out

    lines = []
    for sub in ("4:4:4", "4:2:0"):
        code = image_ops.JPEG_SUBSAMPLINGS[sub]
        blocks, cap = image_ops.jpeg_blocks(h, w, sub), image_ops.jpeg_capacity(h, w, sub)
        desc = np.zeros(n, dtype=image_ops.JPEG_IMAGE_DTYPE)
        for b in range(n):
            desc[b] = (b * h * w * 3, b * cap, h, w, 3, q, code, cap, (0, 0))
        desc_dev = torch.from_numpy(desc.view(np.int64).reshape(-1).copy()).cuda()
        pool = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
        state = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        ws = torch.empty(gpu_lib.jpeg_workspace_bytes(n, blocks), dtype=torch.uint8, device="cuda")
        p = O.jpeg_encode_u8(x.view(-1), pool, desc_dev, state, ws, n=n, max_blocks=blocks, bad_mask=state[n:])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            gpu_lib.check(gpu_lib.lib.i2i_jpeg_encode_u8(C.addressof(p), 0, C.c_void_p(side.cuda_stream)))     # warm-up: modules loaded before capture
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                gpu_lib.check(gpu_lib.lib.i2i_jpeg_encode_u8(C.addressof(p), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.current_stream().wait_stream(side)
        tg = events(graph.replay)
        lens = state.cpu().numpy()
        assert lens[n] == 0 and (lens[:n] > 623).all()
        got = [pool[b * cap:b * cap + int(lens[b])].cpu().numpy().tobytes() for b in range(n)]
        if jc.have_pillow_jpeg():
            assert got == pillow_all(host, code)
        else:
            import jpeg_ref
            assert got[0] == jpeg_ref.encode(host[0], q, sub)
        x.copy_(torch.flip(x, dims=[0]))                                          # other pixels in place: the same graph follows them
        graph.replay()
        torch.cuda.synchronize()
        l2 = state.cpu().numpy()
        assert [pool[b * cap:b * cap + int(l2[b])].cpu().numpy().tobytes() for b in range(n)] == got[::-1]
        x.copy_(torch.flip(x, dims=[0]))
        torch.cuda.synchronize()
        line = "[jpeg] 8 x 512x512x3, quality %d, %s: encode as one captured graph median %.4f ms (min %.4f, max %.4f), files %d bytes in all" % (
            q, sub, tg[5], tg[0], tg[-1], int(lens[:n].sum()))
        if jc.have_pillow_jpeg():
            th = []
            for _ in range(5):
                t0 = time.perf_counter()
                raw = x.cpu().numpy()
                t1 = time.perf_counter()
                pillow_all(raw, code)
                th.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
            th.sort()
            line += "; device-to-host copy of the raw batch + Image.save of the eight arrays on one host thread median %.2f ms (min %.2f, max %.2f; the copy %.2f ms of it)" % (
                th[2][0], th[0][0], th[-1][0], th[2][1])
        lines.append(line + "; 10 replays, HIP events; 5 host runs")
    print("\n".join(lines))

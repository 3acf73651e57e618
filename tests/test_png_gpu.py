"""PNG encoding on the device, on an MI355X: the cases of tests/test_png_emu.py (shared through tests/png_cases.py) with valid
descriptors only, both model classes, and one timing line."""
import io

import numpy as np
import pytest
import torch

import png_cases as pc

pytestmark = pytest.mark.gpu
SIZE_IDS = ["%dx%d" % s for s in pc.SIZES]


def test_png_abi_is_additive(gpu_lib):
    pc.check_abi(gpu_lib)


def test_png_bound_host_code(gpu_lib):
    pc.check_bound(gpu_lib)


@pytest.mark.parametrize("size", pc.SIZES, ids=SIZE_IDS)
def test_png_grid(gpu_lib, size):
    pc.check_grid(gpu_lib, "cuda", *size)


def test_png_ragged_batch(gpu_lib):
    pc.check_ragged_batch(gpu_lib, "cuda")


def test_png_invert(gpu_lib):
    pc.check_invert(gpu_lib, "cuda")


def test_png_grid_independence(gpu_lib):
    pc.check_grid_independence(gpu_lib, "cuda")


def test_png_overflow_is_flagged(gpu_lib):
    pc.check_overflow(gpu_lib, "cuda")


def test_png_bad_args(gpu_lib):
    pc.check_bad_args(gpu_lib, "cuda")


@pytest.mark.parametrize("kind", ["pix2pix", "cyclegan"])
def test_png_forward_u8(gpu_lib, kind):
    pc.check_forward_png(gpu_lib, "cuda", kind)


def test_png_timing_line(gpu_lib):
    """8 x 512 x 512 x 3 of the smooth content: the encode call as ONE captured graph (torch.cuda.graph around the eager entry; one warm-up,
    the median of 10 replays, HIP events), printed beside the host path it replaces -- the device-to-host copy of the raw batch plus
    Image.save(f, "PNG") of the eight arrays on one host thread -- and the size ratio device files / Pillow files for the smooth and the
    edge-map content.  Print only; asserted: every file decodes to its array, the first equals the oracle's, and a replay after the pixels
    changed in place follows them."""
    import ctypes as C
    import time
    import png_ref
    from PIL import Image
    from img2img_turbo_amd import image_ops, ops as O
    n, h, w = 8, 512, 512

    def pillow_all(arrays):
        out = []
        for a in arrays:
            f = io.BytesIO()
            Image.fromarray(a).save(f, "PNG")
            out.append(f.getvalue())
        return out

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

    lines, ratio = [], {}
    for content in ("smooth", "binary"):
        host = np.stack([pc.image(content, h, w, 3, seed=s) for s in range(n)])
        x = torch.from_numpy(host.copy()).cuda()
        cap, mb = gpu_lib.png_bound(w, h, 3), image_ops.png_stream_bytes(h, w, 3)
        desc = np.zeros(n, dtype=image_ops.PNG_IMAGE_DTYPE)
        for b in range(n):
            desc[b] = (b * h * w * 3, b * cap, h, w, 3, 0, cap, (0, 0, 0))
        desc_dev = torch.from_numpy(desc.view(np.int64).reshape(-1).copy()).cuda()
        pool = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
        state = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        ws = torch.empty(gpu_lib.png_workspace_bytes(n, mb), dtype=torch.uint8, device="cuda")
        p = O.png_encode_u8(x.view(-1), pool, desc_dev, state, ws, n=n, max_bytes=mb, bad_mask=state[n:])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            gpu_lib.check(gpu_lib.lib.i2i_png_encode_u8(C.addressof(p), 0, C.c_void_p(side.cuda_stream)))     # warm-up: modules loaded before capture
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                gpu_lib.check(gpu_lib.lib.i2i_png_encode_u8(C.addressof(p), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.current_stream().wait_stream(side)
        tg = events(graph.replay)
        lens = state.cpu().numpy()
        assert lens[n] == 0 and (lens[:n] > 63).all()
        got = [pool[b * cap:b * cap + int(lens[b])].cpu().numpy().tobytes() for b in range(n)]
        for f, a in zip(got, host):
            assert (pc.decode(f) == a).all()
        assert got[0] == png_ref.encode(host[0])
        pil = pillow_all(host)
        ratio[content] = sum(len(f) for f in got) / sum(len(f) for f in pil)
        if content != "smooth":
            continue
        x.copy_(torch.flip(x, dims=[0]))                                          # other pixels in place: the same graph follows them
        graph.replay()
        torch.cuda.synchronize()
        l2 = state.cpu().numpy()
        assert [pool[b * cap:b * cap + int(l2[b])].cpu().numpy().tobytes() for b in range(n)] == got[::-1]
        x.copy_(torch.flip(x, dims=[0]))
        torch.cuda.synchronize()
        th = []
        for _ in range(3):
            t0 = time.perf_counter()
            raw = x.cpu().numpy()
            t1 = time.perf_counter()
            pillow_all(raw)
            th.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        th.sort()
        lines.append("[png] 8 x 512x512x3, smooth content: encode as one captured graph median %.4f ms (min %.4f, max %.4f), files %d bytes in all; "
                     "device-to-host copy of the raw batch + Image.save of the eight arrays on one host thread median %.2f ms (min %.2f, max %.2f; the "
                     "copy %.2f ms of it); 10 replays, HIP events; 3 host runs" % (tg[5], tg[0], tg[-1], int(lens[:n].sum()), th[1][0], th[0][0], th[-1][0], th[1][1]))
    lines.append("[png] size ratio, device files / Pillow files: smooth %.3f, edge map %.3f" % (ratio["smooth"], ratio["binary"]))
    print("\n".join(lines))

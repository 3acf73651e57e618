"""Mixed-size images in one batch on an MI355X: the cases of tests/test_ragged_emu.py (shared through tests/ragged_cases.py) with valid
descriptors only, one realistic batch against Pillow, and one timing line."""
import time

import numpy as np
import pytest
import torch

import ragged_cases as rg

pytestmark = pytest.mark.gpu


def test_ragged_abi_is_additive(gpu_lib):
    rg.check_struct_size(gpu_lib)


@pytest.mark.parametrize("pair", rg.TABLE_PAIRS, ids=lambda p: "%dto%d" % p)
def test_lanczos_tables(gpu_lib, pair):
    rg.check_tables(gpu_lib, pair)


def test_ragged_in(gpu_lib):
    rg.check_ragged_in(gpu_lib, "cuda")


def test_ragged_out(gpu_lib):
    rg.check_ragged_out(gpu_lib, "cuda")


@pytest.mark.parametrize("c", [1, 4])
def test_ragged_other_channel_counts(gpu_lib, c):
    rg.check_channels(gpu_lib, "cuda", c)


def test_ragged_empty_slot_and_write_bounds(gpu_lib):
    rg.check_write_bounds(gpu_lib, "cuda")


def test_ragged_grid_independence(gpu_lib):
    rg.check_grid_independence(gpu_lib, "cuda")


def test_ragged_one_graph_two_requests(gpu_lib):
    rg.check_graph(gpu_lib, "cuda")


def test_ragged_bad_args(gpu_lib):
    rg.check_bad_args(gpu_lib, "cuda")


def test_ragged_pix2pix_forward_u8_list(gpu_lib):
    rg.check_pix2pix_list(gpu_lib, "cuda", size=(88, 72))


def test_ragged_cyclegan_forward_u8_list(gpu_lib):
    rg.check_cyclegan_list(gpu_lib, "cuda", size=(88, 72))


def test_ragged_realistic_sizes_against_pillow(gpu_lib):
    """720 x 1280, 561 x 843 and 512 x 512 -> 512 x 512 and back to each request's size: Pillow, bit for bit, in both directions (the
    512 x 512 image is the identity twice)."""
    from img2img_turbo_amd import image_ops
    srcs = rg.images(rg.REAL_HW, 3)
    devs = [rg.to_dev(a, "cuda") for a in srcs]
    there = image_ops.lanczos_resize_u8_ragged(devs, (512, 512), lib=gpu_lib)
    host = there.cpu().numpy()
    for b, a in enumerate(srcs):
        assert np.array_equal(host[b], rg.pillow(a, (512, 512))), b
    assert np.array_equal(host[2], srcs[2])
    back = image_ops.lanczos_resize_u8_ragged(there, [(w, h) for h, w in rg.REAL_HW], lib=gpu_lib)
    for b, (h, w) in enumerate(rg.REAL_HW):
        assert np.array_equal(back[b].cpu().numpy(), rg.pillow(host[b], (w, h))), b


def test_ragged_timing_line(gpu_lib):
    """Eight images of eight different sizes around 1280 x 720 -> 512 x 512, on the device: the ragged path (two launches) beside the only
    option there was before it, eight lanczos_resize_u8 calls (two launches and two allocations each).  Both as the eager Python calls,
    host clock around the call plus a synchronisation (what a request pays), tables and descriptors warm; and the two ragged launches alone
    as a captured graph beside the sixteen launches as a captured graph (HIP events).  One warm-up, then the median of 10 with the spread.
    Print only, no gate."""
    from img2img_turbo_amd import _capi as K, image_ops, ops as O
    hw = [(720, 1280), (712, 1272), (704, 1288), (736, 1264), (728, 1296), (696, 1256), (744, 1248), (688, 1304)]
    devs = [rg.to_dev(a, "cuda") for a in rg.images(hw, 3)]
    size = (512, 512)

    def ragged():
        return image_ops.lanczos_resize_u8_ragged(devs, size, lib=gpu_lib)

    def eight():
        return torch.cat([image_ops.lanczos_resize_u8(t[None], size, lib=gpu_lib) for t in devs])

    def clock(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(10):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return sorted(ms)

    assert torch.equal(ragged(), eight())
    tr, t8 = clock(ragged), clock(eight)
    print("[ragged] 8 images ~1280x720 -> 512x512, eager calls, host clock incl. sync: lanczos_resize_u8_ragged median %.3f ms (min %.3f, max %.3f); "
          "8 x lanczos_resize_u8 median %.3f ms (min %.3f, max %.3f); 10 runs each" % (tr[5], tr[0], tr[-1], t8[5], t8[0], t8[-1]))

    # the launches alone: captured graphs over pre-packed buffers
    layout, desc, tables = image_ops._ragged_pool(gpu_lib, [t.shape[:2] for t in devs], [size] * 8, 3, devs[0].device)
    src = torch.cat([t.reshape(-1) for t in devs])                       # (every image here is a multiple of 4 bytes)
    mid = torch.empty(layout.mid_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(layout.dst_bytes, dtype=torch.uint8, device="cuda")
    two, sixteen = K.Program(), K.Program()
    for i, (opcode, p) in enumerate(image_ops.ragged_ops(layout, src, mid, dst, desc, tables)):
        two.add(opcode, K.F32, p, "ragged %d" % i)
    outs = []
    for b, t in enumerate(devs):
        h, w = hw[b]
        m = torch.empty(h, 512, 3, dtype=torch.uint8, device="cuda")
        o = torch.empty(512, 512, 3, dtype=torch.uint8, device="cuda")
        for axis, s, d, n_in, hin, win in ((1, t, m, w, h, w), (0, m, o, h, h, 512)):
            ksize, bounds, coeffs = image_ops._tables(n_in, 512, t.device)
            p = K.ResizeU8Params()
            p.src, p.dst, p.n, p.hin, p.win, p.c = s.data_ptr(), d.data_ptr(), 1, hin, win, 3
            p.axis, p.nout, p.ksize, p.bounds, p.coeffs = axis, 512, ksize, bounds.data_ptr(), coeffs.data_ptr()
            sixteen.add(K.OP_RESIZE_U8, K.F32, O._keep(p, s, d, bounds, coeffs), "resize %d.%d" % (b, axis))
        outs.append(o)
    two.freeze()
    sixteen.freeze()
    stream = torch.cuda.current_stream().cuda_stream
    g2, g16 = gpu_lib.graph_create(two), gpu_lib.graph_create(sixteen)
    try:
        def events(g):
            gpu_lib.graph_launch(g, stream)
            torch.cuda.synchronize()
            ms = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gpu_lib.graph_launch(g, stream)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            return sorted(ms)
        a, b = events(g2), events(g16)
        assert torch.equal(dst.view(8, 512, 512, 3), torch.stack(outs))
        print("[ragged] the same as captured graphs, HIP events: 2 x i2i_resize_u8_ragged median %.3f ms (min %.3f, max %.3f); "
              "16 x i2i_resize_u8 median %.3f ms (min %.3f, max %.3f); 10 replays each" % (a[5], a[0], a[-1], b[5], b[0], b[-1]))
    finally:
        torch.cuda.synchronize()
        gpu_lib.graph_destroy(g2)
        gpu_lib.graph_destroy(g16)

"""Cases and backend-independent checks shared by tests/test_batch_emu.py (CPU emulator) and tests/test_batch_gpu.py (MI355X): the per-image
request parameters of a batch -- i2i_randn_batch (csrc/elementwise.hip) and i2i_canny_u8_batch (csrc/resize.hip), the "ABI 14 additions" of
include/i2i_turbo.h -- and the planned forwards built on them (ForwardPlan(rng="per_image" / canny="per_image"), forward(seed=[..])).

Every property is stated against the existing single-image op on the same back end or against the integer oracles (tests/randn_ref.py,
tests/canny_ref.py, applied per image), so every comparison is bit-exact; the one tolerance is the existing contract's rad * 2^-21 of the
normal kind against the fp64 oracle (randn_cases.TOL), on the emulator."""
import ctypes as C

import numpy as np
import torch

import canny_cases as cc
import canny_ref
import randn_cases as rc

B = 3
# (seed, step) per image: a plain one, a seed >= 2^32 (the high key word) at the step that wraps, a 64-bit seed at a small step
ROWS = [(42, 0), ((1 << 40) + 7, 0xFFFFFFFF), (0xFEDCBA9876543210, 5)]
SEEDS, STEPS = [r[0] for r in ROWS], [r[1] for r in ROWS]
STREAM = 2
PERM = [2, 0, 1]
# 0: the no-op; 1, 3: a tail only; 4, 5: one counter and one element more; 1023 .. 1025: one workgroup's 256 counters, ragged / whole / one more
# -- with per_image % 4 != 0 the image bases rotate through all four alignments, so the 16-byte store is taken by some images only
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025]
PARENT_SIZEOF_OP = 368          # sizeof(i2i_op) before the additions (the union is sized by i2i_igemm_params: 8 + 360)
RESERVED = 0xDEADBEEF           # what the tests put into the reserved word: it must be ignored


def big_size():
    """The smallest per_image at which the batch kernel's grid-stride loop runs a second time at batch 3: one element (= one Philox counter)
    more than a pass of the capped grid covers (rng.batch_pass_elements mirrors RANDN_BATCH_MAX_BLOCKS of csrc/elementwise.hip;
    test_batch_emu.py checks that the two agree)."""
    from img2img_turbo_amd import rng
    return rng.batch_pass_elements(B) + 1


def states(device, rows=None, reserved=RESERVED):
    """The int32 [B, 4] device table of ROWS (or ``rows``), the reserved word set to garbage."""
    rows = ROWS if rows is None else rows
    words = [[s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF, t & 0xFFFFFFFF, reserved] for s, t in rows]
    return rc.state_tensor([w for row in words for w in row], device).reshape(len(rows), 4)


def call(lib, device, dst_ptr, per_image, batch, states_ptr, *, kind=rc.RAW, stream=STREAM, null_params=False):
    """i2i_randn_batch through the raw C entry; returns the status."""
    from img2img_turbo_amd import _capi as K
    p = K.RandnBatchParams()
    p.dst, p.per_image, p.batch, p.states, p.stream_id, p.kind = dst_ptr, per_image, batch, states_ptr, stream, kind
    hip_stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None
    status = lib.lib.i2i_randn_batch(None if null_params else C.addressof(p), 0, hip_stream)
    rc.sync(device)
    return status


def fill(lib, device, per_image, offset, kind, rows=None):
    """One batch fill through the eager form with ``out=`` on a slice of a guarded buffer that starts ``offset`` elements past a 16-byte
    boundary; returns the [B, per_image] words as uint32 after checking that the guard band on both sides is untouched."""
    from img2img_turbo_amd import rng
    rows = ROWS if rows is None else rows
    n = len(rows) * per_image
    buf, first = rc.guarded(n, offset, device)
    st = states(device, rows)
    if kind == rc.RAW:
        rng.raw_u32_batch(len(rows), per_image, None, stream=STREAM, lib=lib, states=st, out=buf[first:first + n].view(len(rows), per_image))
    else:
        rng.randn_batch((len(rows), per_image), None, stream=STREAM, lib=lib, states=st,
                        out=buf.view(torch.float32)[first:first + n].view(len(rows), per_image))
    rc.sync(device)
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:first] == rc.CANARY).all() and (host[first + n:] == rc.CANARY).all(), ("canary", per_image, offset, kind)
    assert rc.read_state(st.reshape(-1)) == rc.read_state(states(device, rows).reshape(-1))          # a fill leaves the table alone
    return host[first:first + n].reshape(len(rows), per_image)


# ---------------------------------------------------------------------------------------------------------------- randn_batch
def check_raw(lib, device, per_image):
    """RAW: every row is the oracle's words of that row's state and what rng.raw_u32 gives at that row's seed and step; permuting the rows
    of the table permutes the rows of the output."""
    from img2img_turbo_amd import rng
    for offset in rc.OFFSETS:
        got = fill(lib, device, per_image, offset, rc.RAW)
        assert got.shape == (B, per_image)
        if per_image == 0:
            continue
        for b, (seed, step) in enumerate(ROWS):
            assert np.array_equal(got[b], rc.want_raw(per_image, seed, step, STREAM)), (per_image, offset, b)
            single = rng.raw_u32(per_image, seed, step, STREAM, device=device, lib=lib)
            assert np.array_equal(got[b], single.cpu().numpy().view(np.uint32)), (per_image, offset, b)
        perm = fill(lib, device, per_image, offset, rc.RAW, rows=[ROWS[i] for i in PERM])
        assert np.array_equal(perm, got[PERM]), (per_image, offset)


def check_normal(lib, device, per_image, oracle):
    """NORMAL: every row is rng.randn((per_image,), seed_b, step_b, stream) of the same library, bit for bit (compared as words: -0.0 is not
    0.0 here); ``oracle``: also within the contract's rad * 2^-21 of tests/randn_ref.py.  Returns max |err| / rad (0 without the oracle)."""
    from img2img_turbo_amd import rng
    worst = 0.0
    for offset in rc.OFFSETS:
        got = fill(lib, device, per_image, offset, rc.NORMAL)
        if per_image == 0:
            continue
        for b, (seed, step) in enumerate(ROWS):
            single = rng.randn((per_image,), seed, step, STREAM, device=device, lib=lib)
            assert np.array_equal(got[b], single.cpu().numpy().view(np.uint32)), (per_image, offset, b)
            if oracle:
                val = got[b].view(np.float32).astype(np.float64)
                want, rad = rc.want_normal(per_image, seed, step, STREAM)
                assert np.isfinite(val).all() and np.abs(val).max() <= rc.ABS_MAX
                err, zero = np.abs(val - want), rad == 0
                assert (val[zero] == 0).all() and (err <= rad * rc.TOL).all(), (per_image, offset, b)
                if (~zero).any():
                    worst = max(worst, float((err[~zero] / rad[~zero]).max()))
        perm = fill(lib, device, per_image, offset, rc.NORMAL, rows=[ROWS[i] for i in PERM])
        assert np.array_equal(perm, got[PERM]), (per_image, offset)
    return worst


def check_advance(lib, device):
    """ADVANCE: every row's step + 1 (0xffffffff wraps to 0); words 0, 1, 3, the words around the table and dst are untouched.  Then the
    program-op form (capi.hip's dispatch): normal fill, raw fill, advance, raw fill, as a per-image plan records them."""
    from img2img_turbo_amd import _capi as K, ops as O, rng
    table = states(device).reshape(-1)
    before = rc.read_state(table)
    buf = torch.cat([rc.state_tensor([rc.CANARY] * 4, device), table, rc.state_tensor([rc.CANARY] * 4, device)])
    st = buf[4:4 + 4 * B].view(B, 4)
    dst, first = rc.guarded(B * 5, 0, device)
    assert call(lib, device, dst.data_ptr() + 4 * first, 5, B, st.data_ptr(), kind=rc.ADVANCE) == 0
    after = [w if i % 4 != 2 else (w + 1) & 0xFFFFFFFF for i, w in enumerate(before)]
    assert after[6] == 0                                                       # row 1 wrapped
    assert rc.read_state(buf) == [rc.CANARY] * 4 + after + [rc.CANARY] * 4
    assert (dst.cpu().numpy().view(np.uint32) == rc.CANARY).all()
    rng.advance_batch(st, lib=lib)                                             # the eager form, once more
    rc.sync(device)
    assert rc.read_state(buf)[4:-4] == [w if i % 4 != 2 else (w + 2) & 0xFFFFFFFF for i, w in enumerate(before)]
    # one program
    n = 99                                                                     # (n % 4 = 3: images 1 and 2 start off a 16-byte boundary)
    st = states(device)
    a = torch.zeros(B, n, dtype=torch.float32, device=device)
    b = torch.zeros(B, n, dtype=torch.int32, device=device)
    c = torch.zeros(B, n, dtype=torch.int32, device=device)
    prog = K.Program()
    prog.add(*rc._op(O.randn_batch(a, st, batch=B, stream_id=0)), "normal")
    prog.add(*rc._op(O.randn_batch(b, st, batch=B, stream_id=STREAM, kind=K.RANDN_RAW)), "raw")
    prog.add(*rc._op(O.randn_batch(None, st, batch=B, kind=K.RANDN_ADVANCE)), "advance")
    prog.add(*rc._op(O.randn_batch(c, st, batch=B, stream_id=STREAM, kind=K.RANDN_RAW)), "raw after")
    prog.freeze()
    lib.run(prog, torch.cuda.current_stream().cuda_stream if device != "cpu" else 0)
    rc.sync(device)
    for i, (seed, step) in enumerate(ROWS):
        assert torch.equal(a[i].view(torch.int32), rng.randn((n,), seed, step, 0, device=device, lib=lib).view(torch.int32)), i
        assert np.array_equal(b[i].cpu().numpy().view(np.uint32), rc.want_raw(n, seed, step, STREAM)), i
        assert np.array_equal(c[i].cpu().numpy().view(np.uint32), rc.want_raw(n, seed, (step + 1) & 0xFFFFFFFF, STREAM)), i


def check_errors(lib, device):
    """Every error case of the contract returns I2I_ERR_BAD_ARG with a message and writes nothing; the empty fills are successful no-ops."""
    import pytest
    from img2img_turbo_amd import _capi as K
    buf, first = rc.guarded(B * 16, 0, device)
    dst = buf.data_ptr() + 4 * first
    st = states(device)
    sp = st.data_ptr()
    bad = [dict(null_params=True),
           dict(states_ptr=0), dict(states_ptr=0, kind=rc.ADVANCE),            # null states
           dict(states_ptr=sp + 2), dict(states_ptr=sp + 2, kind=rc.ADVANCE),  # states not 4-byte aligned
           dict(batch=-1), dict(per_image=-1), dict(batch=-1, kind=rc.ADVANCE),
           dict(dst_ptr=0), dict(dst_ptr=0, kind=rc.NORMAL),                   # null dst, fill kinds
           dict(dst_ptr=dst + 2), dict(dst_ptr=dst + 2, kind=rc.NORMAL),       # dst not 4-byte aligned
           dict(kind=3), dict(kind=-1)]                                        # unknown kind
    for kw in bad:
        args = dict(dst_ptr=dst, per_image=16, batch=B, states_ptr=sp)
        args.update(kw)
        status = call(lib, device, args.pop("dst_ptr"), args.pop("per_image"), args.pop("batch"), args.pop("states_ptr"), **args)
        assert status == -1, (kw, status)                                      # I2I_ERR_BAD_ARG
        msg = lib.lib.i2i_last_error().decode()
        assert msg.startswith("randn_batch:") and len(msg) > len("randn_batch: "), (kw, msg)
        assert (buf.cpu().numpy().view(np.uint32) == rc.CANARY).all(), kw
        assert rc.read_state(st.reshape(-1)) == rc.read_state(states(device).reshape(-1)), kw
        with pytest.raises(K.I2IError):
            lib.check(status)
    for kind in (rc.NORMAL, rc.RAW):
        assert call(lib, device, dst, 16, 0, sp, kind=kind) == 0 and call(lib, device, dst, 0, B, sp, kind=kind) == 0
        assert call(lib, device, 0, 0, B, sp, kind=kind) == 0                  # (no destination needed for nothing)
    assert call(lib, device, 0, 0, 0, sp, kind=rc.ADVANCE) == 0
    assert (buf.cpu().numpy().view(np.uint32) == rc.CANARY).all()
    assert rc.read_state(st.reshape(-1)) == rc.read_state(states(device).reshape(-1))


def check_struct_size(lib):
    from img2img_turbo_amd import _capi as K
    assert lib.lib.i2i_sizeof_op() == C.sizeof(K.Op) == PARENT_SIZEOF_OP
    assert C.sizeof(K.RandnBatchParams) <= C.sizeof(K.IgemmParams) and C.sizeof(K.CannyU8BatchParams) <= C.sizeof(K.IgemmParams)
    assert lib.lib.i2i_abi_version() == K.ABI_VERSION == 14 and (K.OP_RANDN_BATCH, K.OP_CANNY_U8_BATCH) == (19, 20)


def check_module(lib, device):
    """img2img_turbo_amd.rng: the packing and the eager forms with seeds / steps instead of a table."""
    import pytest
    from img2img_turbo_amd import rng
    assert rng.pack_states([42, (1 << 40) + 7]) == [[42, 0, 0, 0], [7, 1 << 8, 0, 0]]
    assert rng.pack_states([42, -1], [5, -1]) == [[42, 0, 5, 0], [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0]]
    assert rng.pack_states([], 3) == []
    with pytest.raises(ValueError):
        rng.pack_states([1, 2], [0])
    x = rng.randn_batch((B, 4, 9, 11), SEEDS, STEPS, stream=STREAM, device=device, lib=lib)
    assert x.shape == (B, 4, 9, 11) and x.dtype == torch.float32
    for b, (seed, step) in enumerate(ROWS):
        assert torch.equal(x[b].view(torch.int32), rng.randn((4, 9, 11), seed, step, STREAM, device=device, lib=lib).view(torch.int32)), b
    y = rng.randn_batch((B, 396), SEEDS, 1, device=device, lib=lib)                  # one step for every row, stream 0
    w = rng.raw_u32_batch(B, 7, SEEDS, STEPS, stream=STREAM, device=device, lib=lib)
    assert w.dtype == torch.int32 and w.shape == (B, 7)
    for b, (seed, step) in enumerate(ROWS):
        assert torch.equal(y[b].view(torch.int32), rng.randn((396,), seed, 1, 0, device=device, lib=lib).view(torch.int32)), b
        assert np.array_equal(w[b].cpu().numpy().view(np.uint32), rc.want_raw(7, seed, step, STREAM)), b
    with pytest.raises(ValueError):
        rng.randn_batch((B, 8), SEEDS[:2], device=device, lib=lib)


# ---------------------------------------------------------------------------------------------------------------- Canny per image
CANNY_N, CANNY_H, CANNY_W, CANNY_C = 3, 37, 150, 3          # 3 x 3 tiles of 64 x 16 per image, ragged in both directions
CANNY_THR = [(100, 200), (200, 100), (0, 1)]               # plain; low > high (swapped); everything with a gradient is strong


def canny_images():
    return cc.smooth_noise(CANNY_N, CANNY_H, CANNY_W, CANNY_C)


def canny_batch_call(lib, device, src, thr, *, ws=None, out_c=3, null=None):
    """i2i_canny_u8_batch through the raw C entry.  Returns (status, dst, ws)."""
    from img2img_turbo_amd import _capi as K
    n, h, w, c = src.shape
    dst = torch.full((n, h, w, out_c), 7, dtype=torch.uint8, device=device)
    if ws is None:
        ws = torch.empty(lib.canny_ws_bytes(n, h, w), dtype=torch.uint8, device=device)
    p = K.CannyU8BatchParams()
    p.src, p.dst, p.ws, p.thr = src.data_ptr(), dst.data_ptr(), ws.data_ptr(), (thr.data_ptr() if thr is not None else 0)
    p.n, p.h, p.w, p.c, p.out_c = n, h, w, c, out_c
    if null:
        setattr(p, null, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None
    status = lib.lib.i2i_canny_u8_batch(C.addressof(p), 0, stream)
    rc.sync(device)
    return status, dst, ws


def check_canny(lib, device):
    from img2img_turbo_amd import _capi as K, image_ops, ops as O
    img = canny_images()
    src = cc.to_dev(img, device)
    lows, highs = [t[0] for t in CANNY_THR], [t[1] for t in CANNY_THR]
    got = image_ops.canny_u8(src, lows, highs, lib=lib)
    assert got.shape == (CANNY_N, CANNY_H, CANNY_W, 3) and got.dtype == torch.uint8
    want = np.stack([canny_ref.canny(img[b], lows[b], highs[b], 3) for b in range(CANNY_N)])
    for b in range(CANNY_N):
        single = image_ops.canny_u8(src[b:b + 1].clone(), lows[b], highs[b], lib=lib)      # (a copy: the entry wants a 4-byte aligned batch)
        assert torch.equal(got[b:b + 1], single), b
        assert np.array_equal(got[b].cpu().numpy(), want[b]), (b, int((got[b].cpu().numpy() != want[b]).sum()))
    assert np.array_equal(want[0], canny_ref.canny(img[0], 200, 100, 3))                       # (the oracle swaps too)
    # a scalar beside a sequence holds for every image
    mixed = image_ops.canny_u8(src, 100, [200, 120, 300], lib=lib).cpu().numpy()
    assert all(np.array_equal(mixed[b], canny_ref.canny(img[b], 100, hi, 3)) for b, hi in enumerate([200, 120, 300]))
    # the thresholds are really per image: one image in all three slots, three pairs
    same = cc.to_dev(np.stack([img[0]] * 3), device)
    rows = image_ops.canny_u8(same, [100, 60, 0], [200, 120, 1], lib=lib).cpu().numpy()
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
    assert all(np.array_equal(rows[b], canny_ref.canny(img[0], lo, hi, 3)) for b, (lo, hi) in enumerate([(100, 200), (60, 120), (0, 1)]))
    # the scalar entry on the same batch: the oracle, as before
    assert np.array_equal(image_ops.canny_u8(src, 100, 200, lib=lib).cpu().numpy(), canny_ref.canny_batch(img, 100, 200, 3))
    # the raw entry: a dirty workspace changes nothing and nothing is carried from run to run; out_c = 1
    thr = torch.tensor(CANNY_THR, dtype=torch.int32, device=device)
    ws = torch.full((lib.canny_ws_bytes(CANNY_N, CANNY_H, CANNY_W),), 0xFF, dtype=torch.uint8, device=device)
    s1, d1, ws = canny_batch_call(lib, device, src, thr, ws=ws)
    first = d1.cpu().numpy().copy()
    s2, d2, ws = canny_batch_call(lib, device, src, thr, ws=ws)
    assert s1 == 0 and s2 == 0 and np.array_equal(first, want) and np.array_equal(d2.cpu().numpy(), want)
    s3, d3, _ = canny_batch_call(lib, device, src, thr, out_c=1)
    assert s3 == 0 and np.array_equal(d3.cpu().numpy(), want[..., :1])
    # errors: thr is required (and aligned); the rest as i2i_canny_u8
    misaligned = torch.zeros(4 * 2 * CANNY_N + 4, dtype=torch.uint8, device=device)[2:2 + 8 * CANNY_N]
    for kw in (dict(thr=None), dict(thr=misaligned), dict(thr=thr, null="src"), dict(thr=thr, null="dst"), dict(thr=thr, null="ws"), dict(thr=thr, out_c=2)):
        status, dst, _ = canny_batch_call(lib, device, src, kw.pop("thr"), **kw)
        assert status == -1 and lib.lib.i2i_last_error().decode().startswith("canny_u8_batch:"), kw
        assert bool((dst == 7).all()), kw
    assert lib.lib.i2i_canny_u8_batch(None, 0, None) == -1
    # the op through i2i_run (capi.hip's dispatch), as a per-image plan records it
    dst = torch.zeros(CANNY_N, CANNY_H, CANNY_W, 3, dtype=torch.uint8, device=device)
    prog = K.Program()
    opcode, params = O.canny_u8_batch(src, dst, ws, thr, n=CANNY_N, h=CANNY_H, w=CANNY_W, c=CANNY_C, out_c=3)
    prog.add(opcode, K.F32, params, "canny")
    lib.run(prog.freeze(), torch.cuda.current_stream().cuda_stream if device != "cpu" else 0)
    rc.sync(device)
    assert np.array_equal(dst.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- the planned forward
FWD_SEEDS = [7, (1 << 40) + 7, 8]


def state_rows(plan):
    return [rc.read_state(row) for row in plan.rng_state]


def check_forward(lib, device, stochastic, h=rc.H, w=rc.W, replay=None):
    """forward(seed=[s0, s1, s2]) at batch 3.  ``replay(plan)``: how one more run of the plan's program is made (default plan.run(); the GPU
    test passes a captured graph's launch).  Returns (model, plan)."""
    import pytest
    from img2img_turbo_amd import rng
    model = rc.make_model(lib, device, stochastic)
    x, cap = rc.pipeline_inputs(B, device, h, w)
    kw = dict(caption_enc=cap, deterministic=not stochastic, r=0.4 if stochastic else 1.0)
    lat = (4, h // 8, w // 8)

    def draws(step, stream):
        return torch.stack([rng.randn(lat, s, step, stream=stream, device=device, lib=lib) for s in FWD_SEEDS])

    out = model.forward(x, seed=FWD_SEEDS, **kw)
    assert len(model._plans) == 1
    plan = list(model._plans.values())[0]
    assert plan.rng == "per_image" and plan.rng_per_image and plan.rng_state.shape == (B, 4) and plan.rng_state.dtype == torch.int32
    assert state_rows(plan) == [rng.pack_state(s, 1) for s in FWD_SEEDS]              # one run: every row's step moved on
    labels = plan.prog.labels
    assert labels[0] == "rng.eps" and labels[-1] == "rng.advance" and ("rng.noise" in labels) == stochastic
    eps, noise = draws(0, 0), draws(0, 2)
    assert torch.equal(plan.eps.view(torch.int32), eps.view(torch.int32))
    assert (plan.noise is not None) == stochastic and (not stochastic or torch.equal(plan.noise.view(torch.int32), noise.view(torch.int32)))
    with pytest.raises(AssertionError, match="set_seeds"):
        plan.set_seed(3)
    # the explicit twin: exactly those tensors through eps= / noise_map=, on a plan without the op
    out_explicit = model.forward(x, eps=eps, noise_map=noise if stochastic else None, **kw)
    assert len(model._plans) == 2 and torch.equal(out, out_explicit)
    # three replays after set_seeds: steps 0, 1, 2 for every image, without the host
    plan._prepare()
    plan.set_seeds(FWD_SEEDS)
    outs = []
    for k in range(3):
        (replay or (lambda p: p.run()))(plan)
        rc.sync(device)
        assert torch.equal(plan.eps.view(torch.int32), draws(k, 0).view(torch.int32)), k
        if stochastic:
            assert torch.equal(plan.noise.view(torch.int32), draws(k, 2).view(torch.int32)), k
        assert state_rows(plan) == [rng.pack_state(s, k + 1) for s in FWD_SEEDS], k
        outs.append(plan.out.clone())
    assert torch.equal(outs[0], out) and not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    assert state_rows(plan) == [[s & 0xFFFFFFFF, s >> 32, 3, 0] for s in FWD_SEEDS]
    # slot independence: the requests in other slots draw the same noise -- and, on this model, render the same image bit for bit
    out_p = model.forward(x[PERM], seed=[FWD_SEEDS[i] for i in PERM], **kw)
    assert len(model._plans) == 2
    assert torch.equal(plan.eps.view(torch.int32), eps[PERM].view(torch.int32))
    assert not stochastic or torch.equal(plan.noise.view(torch.int32), noise[PERM].view(torch.int32))
    assert torch.equal(out_p, out[PERM])
    # the argument checks
    with pytest.raises(ValueError):
        model.forward(x, seed=[1, 2], **kw)
    with pytest.raises(ValueError):
        model.forward(x, seed=FWD_SEEDS, eps=eps, **kw)
    with pytest.raises(ValueError):
        plan.set_seeds([1, 2])
    # the scalar seed on the same model: the flat index over the whole buffer, on a plan of its own
    model.forward(x, seed=7, **kw)
    assert len(model._plans) == 3
    flat = [p for p in model._plans.values() if p.rng is True][0]
    assert flat.rng_state.shape == (4,) and rc.read_state(flat.rng_state) == [7, 0, 1, 0]
    assert torch.equal(flat.eps, rng.randn((B,) + lat, 7, 0, stream=0, device=device, lib=lib))
    assert not stochastic or torch.equal(flat.noise, rng.randn((B,) + lat, 7, 0, stream=2, device=device, lib=lib))
    return model, plan


def check_forward_canny(lib, device, h=rc.H, w=rc.W):
    """forward_u8(canny=[(low, high)] * B) is the eager per-image Canny followed by forward_u8 of the edge maps; set_canny_thresholds takes
    scalars and sequences."""
    import pytest
    from img2img_turbo_amd import image_ops
    model = rc.make_model(lib, device, False)
    try:
        img, cap, eps = cc.pipeline_inputs(B, h, w)
        imgd, capd, epsd = cc.to_dev(img, device), cap.to(device), eps.to(device)
        out = model.forward_u8(imgd, caption_enc=capd, eps=epsd, canny=CANNY_THR)
        plan = list(model._plans.values())[0]
        assert plan.canny == "per_image" and plan.canny_thr.shape == (B, 2)
        assert plan.canny_thr.cpu().tolist() == [list(t) for t in CANNY_THR]
        edges = image_ops.canny_u8(imgd, [t[0] for t in CANNY_THR], [t[1] for t in CANNY_THR], lib=lib)
        assert torch.equal(plan.canny_edges, edges) and edges.any() and not edges.all()
        assert np.array_equal(edges[1].cpu().numpy(), canny_ref.canny(img[1], 200, 100, 3))
        out_host = model.forward_u8(edges, caption_enc=capd, eps=epsd)
        assert out.shape == (B, h, w, 3) and torch.equal(out, out_host)
        plan.set_canny_thresholds(50, [100, 110, 120])
        assert plan.canny_thr.cpu().tolist() == [[50, 100], [50, 110], [50, 120]]
        with pytest.raises(ValueError):
            plan.set_canny_thresholds([1, 2], 3)
        with pytest.raises(ValueError):
            model.forward_u8(imgd, caption_enc=capd, eps=epsd, canny=CANNY_THR[:2])
        fresh = model.get_plan(B, h + 8, w, u8_io=(1.0, 0.0), canny="per_image")
        assert fresh.canny_thr.cpu().tolist() == [[100, 200]] * B                   # the initial value of every row
    finally:
        model.release_plans()


def check_plan_file(lib, device, tmp_path, model, plan, x, cap, seeds):
    """Export the per-image plan, load it through i2i_plan_load, write a 16 * B byte "seed" and run: "eps" and "out" equal the Python
    replay at those seeds.  Returns (path, eps, out) on the host for further hosts."""
    from img2img_turbo_amd import plan_file, rng
    path = str(tmp_path / "per_image.i2iplan")
    plan.set_seeds([1] * B)
    info = plan_file.export_plan(plan, path)
    assert info["io"]["seed"] == 16 * B
    want = model.forward(x, caption_enc=cap, seed=seeds).cpu()
    eps = plan.eps.cpu()
    table = rc.state_tensor([w for row in rng.pack_states(seeds) for w in row], "cpu")
    h = lib.plan_load(path)
    try:
        assert lib.plan_io(h, "seed")[1] == 16 * B == table.numel() * 4
        assert rc.read_state(lib.plan_read(h, "seed", torch.zeros(4 * B, dtype=torch.int32))) == [1, 0, 0, 0] * B
        lib.plan_write(h, "x", x.cpu())
        lib.plan_write(h, "ctx", cap.cpu())
        lib.plan_write(h, "seed", table)
        lib.plan_run(h, torch.cuda.current_stream().cuda_stream if device != "cpu" else 0)
        assert torch.equal(lib.plan_read(h, "out", torch.zeros_like(want)), want)
        assert torch.equal(lib.plan_read(h, "eps", torch.zeros_like(eps)).view(torch.int32), eps.view(torch.int32))
        assert rc.read_state(lib.plan_read(h, "seed", torch.zeros(4 * B, dtype=torch.int32))) == [w for row in rng.pack_states(seeds, 1) for w in row]
    finally:
        lib.plan_destroy(h)
    return path, eps, want

"""Cases shared by tests/test_variations_emu.py (CPU emulator) and tests/test_variations_gpu.py: the replication op i2i_repeat (the contract is
the comment of i2i_repeat_params in include/i2i_turbo.h) and ForwardPlan / Pix2Pix_Turbo with ``variations=V`` -- V outputs per input image
from one pass of the input ops and the VAE encoder.  Everything runs on the tiny model."""
import ctypes as C

import numpy as np
import torch

import canny_ref
import randn_cases as rc
import randn_ref

PARENT_SIZEOF_OP = 368          # sizeof(i2i_op) before the addition (the union is sized by i2i_igemm_params: 8 + 360)
CHUNK = 1024                    # 16-byte vectors a workgroup of repeat_kernel copies (REPEAT_CHUNK, csrc/elementwise.hip)
GUARD = 64                      # canary bytes on either side of every destination
CANARY = 0xA5
TOL = {torch.float32: 1e-3, torch.bfloat16: 0.15}      # the gate of tests/test_e2e_gpu.py::test_tiny_stochastic_twinconv


def sync(device):
    rc.sync(device)


# ---------------------------------------------------------------------------------------------------------------- i2i_repeat
def _segment(device, batch, variations, n_elems, dtype, seed):
    """(src tensor [batch, n_elems], guarded destination bytes, the view of it the op writes)."""
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        src = torch.randn(batch, n_elems, generator=g).to(dtype)
    else:
        src = torch.randint(0, 200, (batch, n_elems), generator=g).to(dtype)
    nbytes = batch * variations * n_elems * src.element_size()
    raw = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % 16 == 0
    return src.to(device), raw, raw[GUARD:GUARD + nbytes]


def run_repeat(lib, device, batch, variations, shapes, through_program):
    """``shapes``: [(elements per image, dtype)].  Runs the op (as an op of a program, or through the direct entry) and compares every
    destination with torch.repeat_interleave, bit for bit, and every guard byte with the canary."""
    from img2img_turbo_amd import _capi as K
    from img2img_turbo_amd import ops as O
    segs = [_segment(device, batch, variations, n, dt, 100 + i) for i, (n, dt) in enumerate(shapes)]
    op = O.repeat([(s, d) for s, _, d in segs], batch=batch, variations=variations)
    if through_program:
        prog = K.Program()
        prog.add(op[0], K.F32, op[1], "repeat")
        lib.run(prog.freeze())
    else:
        lib.check(lib.lib.i2i_repeat(C.addressof(op[1]), K.U8, C.c_void_p(0)))
    sync(device)
    for (n, dt), (src, raw, dst) in zip(shapes, segs):
        want = src.repeat_interleave(variations, 0)
        got = dst.view(dt).view(batch * variations, n)
        assert torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8)), (batch, variations, n, dt)
        assert (raw[:GUARD] == CANARY).all() and (raw[-GUARD:] == CANARY).all(), (batch, variations, n, dt)


# name -> (batch, variations, [(elements per image, dtype)]); sizes are per image, 16-byte vectors = elements * itemsize / 16
REPEAT_CASES = {
    "one_vector_per_image": (3, 2, [(4, torch.float32)]),
    "one_short_of_a_chunk": (2, 2, [((CHUNK - 1) * 4, torch.float32)]),            # the second image starts inside the first workgroup
    "one_past_a_chunk": (2, 2, [((CHUNK + 1) * 8, torch.bfloat16)]),               # every image spans a workgroup boundary
    "exactly_a_chunk": (3, 2, [(CHUNK * 4, torch.float32)]),
    "identity_b1_v1": (1, 1, [(40, torch.float32)]),
    "b2_v3": (2, 3, [(3 * CHUNK * 8 + 24, torch.float16)]),                        # several workgroups per image, a ragged last one
    "five_segments_mixed": (2, 3, [(8, torch.float32), (264, torch.bfloat16), (48, torch.uint8), (1000, torch.float16), (12, torch.int32)]),
    "five_segments_around_a_chunk": (2, 2, [((CHUNK - 1) * 4, torch.float32), (16, torch.uint8), ((CHUNK // 2 + 1) * 8, torch.bfloat16),
                                            (8, torch.float16), (CHUNK * 4 + 4, torch.int32)]),
    "eight_segments": (2, 2, [(16 * (i + 1), torch.uint8) for i in range(8)]),
}


def check_repeat(lib, device, name):
    batch, variations, shapes = REPEAT_CASES[name]
    for through_program in (True, False):
        run_repeat(lib, device, batch, variations, shapes, through_program)


def check_repeat_errors(lib, device):
    """I2I_ERR_BAD_ARG with a message naming the field, and nothing written."""
    from img2img_turbo_amd import _capi as K
    from img2img_turbo_amd import ops as O
    src = torch.arange(64, dtype=torch.float32, device=device).view(2, 32)
    dst = torch.full((4, 32), -1.0, device=device)

    def call(op):
        rc_ = lib.lib.i2i_repeat(C.addressof(op[1]), K.F32, C.c_void_p(0))
        return rc_, lib.lib.i2i_last_error().decode()

    assert call(O.repeat([(src, dst)], batch=2, variations=2))[0] == 0          # the good call these are variations of
    sync(device)
    assert torch.equal(dst, src.repeat_interleave(2, 0))
    dst.fill_(-1.0)
    cases = [(O.repeat([(src, dst)], batch=2, variations=0), "variations"),
             (O.repeat([(src, dst)] * 9, batch=2, variations=2), "n_segments"),
             (O.repeat([(src, dst)], batch=2, variations=2, bytes_per_image=[120]), "bytes_per_image"),
             (O.repeat([(None, dst)], batch=2, variations=2, bytes_per_image=[128]), "src"),
             (O.repeat([(src, None)], batch=2, variations=2, bytes_per_image=[128]), "dst")]
    for op, field in cases:
        code, msg = call(op)
        assert code == -1 and field in msg, (field, code, msg)
    assert lib.lib.i2i_repeat(None, K.F32, C.c_void_p(0)) == -1
    sync(device)
    assert (dst == -1.0).all()
    # the same refusal through a program: i2i_run names the op
    prog = K.Program()
    op = O.repeat([(src, dst)], batch=2, variations=-3)
    prog.add(op[0], K.F32, op[1], "repeat")
    try:
        lib.run(prog.freeze())
        raise AssertionError("a program with variations = -3 ran")
    except K.I2IError as e:
        assert "variations" in str(e) and "opcode 26" in str(e)


def check_struct_size(lib):
    from img2img_turbo_amd import _capi as K
    assert lib.lib.i2i_sizeof_op() == C.sizeof(K.Op) == PARENT_SIZEOF_OP
    assert C.sizeof(K.RepeatParams) == 16 + 24 * K.REPEAT_MAX_SEGMENTS <= C.sizeof(K.IgemmParams)
    assert K.RepeatParams.src0.offset == 16 and K.RepeatParams.dst0.offset == 24 and K.RepeatParams.bytes0.offset == 32 and K.RepeatParams.src7.offset == 16 + 7 * 24
    assert lib.lib.i2i_abi_version() == K.ABI_VERSION == 14 and K.OP_REPEAT == 26 and K.REPEAT_MAX_SEGMENTS == 8


# ---------------------------------------------------------------------------------------------------------------- the planned forward
def oracle_weights(stochastic):
    from oracle import TINY_UNET, TINY_VAE
    from oracle.synth import make_pix2pix_weights
    return make_pix2pix_weights(TINY_UNET, TINY_VAE, seed=2, sketch=stochastic)


def gw(mw):
    from img2img_turbo_amd.weights import GeneratorWeights
    return GeneratorWeights(mw.unet, mw.vae, mw.unet_arch, mw.vae_arch, mw.unet_scaling, mw.vae_scaling, mw.vae_b2a)


_MODELS = {}


def make_model(lib, device, stochastic=False, dtype=torch.float32, **kw):
    """One model per configuration and session (packing the weights is most of a tiny test's time); every case ends with release_plans(),
    which leaves the model and its packers usable."""
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    key = (lib.path, device, stochastic, dtype, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = Pix2Pix_Turbo(weights=gw(oracle_weights(stochastic)), device=device, dtype=dtype, lib=lib, **kw)
    return _MODELS[key]


def inputs(stochastic, B, V, h, w):
    """x [B], caption [1], eps / noise_map [B * V] (CPU)."""
    from oracle import TINY_UNET
    from oracle.synth import make_inputs
    x, cap, eps, nm = make_inputs("sketch" if stochastic else "canny", B * V, h, w, TINY_UNET.cross_attention_dim)
    return x[:B].contiguous(), cap, eps, nm


def program_of(plan):
    return [(opc, dt, label) for opc, dt, _p, label in plan.prog.ops]


def batch_of(opcode, p):
    """The image count an input / encoder op works on."""
    from img2img_turbo_amd import _capi as K
    return {K.OP_IGEMM: lambda: p.nimg, K.OP_GN_STATS: lambda: p.nimg, K.OP_GN_APPLY: lambda: p.nimg, K.OP_NCHW_TO_NHWC: lambda: p.n,
            K.OP_CANNY_U8: lambda: p.n, K.OP_CANNY_U8_BATCH: lambda: p.n, K.OP_CANNY_AUTO_THR: lambda: p.n,
            K.OP_ATTENTION: lambda: p.batch, K.OP_SOFTMAX: lambda: None}[opcode]()


def check_encoder_once(lib, device, B=2, V=3, h=16, w=24, dtype=torch.float32):
    """Every input.* / encoder.* op of the variations plan has batch B, there are as many as in the plain batch-B plan, there is exactly one
    repeat op, the ops behind it are those of the plain B * V plan; and the digests of the encoder stages and of the moments are bit-equal
    to the plain batch-B plan's on the same input."""
    from img2img_turbo_amd import _capi as K
    model = make_model(lib, device, dtype=dtype, fingerprint="stages")
    try:
        pv = model.get_plan(B, h, w, variations=V)
        pb = model.get_plan(B, h, w)
        pbv = model.get_plan(B * V, h, w)
        assert pv is not pb and pv.V == V and pv.B == B and pv.BV == B * V and pb.V == 1
        front = lambda plan: [(opc, label, p) for opc, _dt, p, label in plan.prog.ops if label.startswith(("input.", "encoder."))]
        fv, fb = front(pv), front(pb)
        assert len(fv) == len(fb) > 10 and [(o, l) for o, l, _ in fv] == [(o, l) for o, l, _ in fb]
        explicit = 0
        for (opc, label, p), (_, _, q) in zip(fv, fb):
            # every shape, stride and count of the op is the plain batch-B plan's (linears carry the batch in their row count M) ...
            for name, ct in p._fields_:
                if ct is not K.vp:
                    assert getattr(p, name) == getattr(q, name), (label, name, getattr(p, name), getattr(q, name))
            # ... and where an op names its image count, it is B
            n = batch_of(opc, p)
            if opc == K.OP_IGEMM and (p.nimg == 1 or p.zcount > 1):      # a linear over B * T rows / a batched matmul: covered above
                n = None
            assert n in (B, None), (label, n)
            explicit += n == B
        assert explicit > 10
        reps = [i for i, (opc, _dt, _l) in enumerate(program_of(pv)) if opc == K.OP_REPEAT]
        assert len(reps) == 1 and program_of(pv)[reps[0]][2] == "variations.repeat"
        rp = pv.prog.ops[reps[0]][2]
        assert (rp.batch, rp.variations, rp.n_segments) == (B, V, 5)
        # behind the repeat op: the plain program at batch B * V, op for op
        tail = lambda plan, start: [(opc, dt, l) for opc, dt, l in program_of(plan)[start:]]
        first_tail = [l for _, _, l in program_of(pbv)].index("posterior_sample")
        assert tail(pv, reps[0] + 1) == tail(pbv, first_tail)
        # the boundary buffers
        assert pv.x_in.shape[0] == B and pv.eps.shape[0] == B * V and pv.out.shape[0] == B * V
        # digests
        x, cap, eps, _ = inputs(False, B, V, h, w)
        model.stage(pv, x.to(device), cap.to(device), eps.to(device))
        pv.run()
        fpv = dict(pv.fingerprint())
        model.stage(pb, x.to(device), cap.to(device), eps[:B].to(device))
        pb.run()
        fpb = dict(pb.fingerprint())
        enc = [l for l in pb.fingerprint_labels if l.startswith("encoder.")] + ["moments"]
        assert len(enc) >= 3
        for l in enc:
            assert fpv[l].shape == (B, 4) and torch.equal(fpv[l].view(torch.int64), fpb[l].view(torch.int64)), l
            assert (fpv[l].view(torch.int64)[:, 2] > 0).all()
        for l in pv.fingerprint_labels:
            if l not in enc:
                assert fpv[l].shape == (B * V, 4) and (fpv[l].view(torch.int64)[:, 2] > 0).all(), l
        # whole-batch health builds and runs on a variations plan
        hm = make_model(lib, device, dtype=dtype, health="stages")
        try:
            ph = hm.get_plan(B, h, w, variations=V)
            hm.stage(ph, x.to(device), cap.to(device), eps.to(device))
            ph.run()
            rep = ph.health_report()
            assert [d["label"] for d in rep] == pv.fingerprint_labels and all(d["runs"] == 1 and d["n_nan"] == 0 for d in rep)
            per_image = {d["label"]: d["elements"] for d in rep}
            assert per_image["latents"] == B * V * 4 * (h // 8) * (w // 8) and per_image["moments"] == B * 8 * (h // 8) * (w // 8)
        finally:
            hm.release_plans()
    finally:
        model.release_plans()


PARITY_SHAPES = [(2, 3, 64, 64), (1, 4, 72, 88)]


def check_parity(lib, device, shape, stochastic, dtype):
    """forward(variations=V) against the oracle on x.repeat_interleave(V, 0) with the same noise; the V outputs of one input differ."""
    from oracle.pipeline import pix2pix_forward
    B, V, h, w = shape
    mw = oracle_weights(stochastic)
    x, cap, eps, nm = inputs(stochastic, B, V, h, w)
    kw = dict(deterministic=False, r=0.4, noise_map=nm) if stochastic else {}
    ref = pix2pix_forward(mw, x.repeat_interleave(V, 0), cap, eps, **kw)
    model = make_model(lib, device, stochastic, dtype)
    try:
        kwd = dict(deterministic=False, r=0.4, noise_map=nm.to(device)) if stochastic else {}
        out = model(x.to(device), caption_enc=cap.to(device), eps=eps.to(device), variations=V, **kwd)
        assert out.shape == (B * V, 3, h, w)
        err = (out.float().cpu() - ref).abs().max().item()
        print("[variations parity] B=%d V=%d %dx%d stochastic=%s %s: max-abs %.3e (gate %.3g)" % (B, V, h, w, stochastic, dtype, err, TOL[dtype]))
        assert err < TOL[dtype], err
        o = out.float().cpu().view(B, V, 3, h, w)
        for b in range(B):
            for v in range(1, V):
                assert not torch.equal(o[b, 0], o[b, v]), (b, v)
        # a caption per input image is expanded to B * V on the device; here every row is the same caption, so the image is too
        if B > 1:
            out_b = model(x.to(device), caption_enc=cap.expand(B, -1, -1).contiguous().to(device), eps=eps.to(device), variations=V, **kwd)
            plan_b = model._last_plan
            assert plan_b.ctx.shape[0] == B * V and plan_b.ctx_in_batch == B
            assert (out_b.float().cpu() - ref).abs().max().item() < TOL[dtype]
        import pytest
        with pytest.raises(ValueError):
            model(x.to(device), caption_enc=cap.to(device), eps=eps[:B].to(device), variations=V, **kwd)
    finally:
        model.release_plans()


def check_v1(lib, device, h=16, w=24, dtype=torch.float32):
    """variations=1 is the forward without the argument: the same plan object from the cache, the same program, the same bits."""
    from img2img_turbo_amd import _capi as K
    model = make_model(lib, device, dtype=dtype)
    try:
        x, cap, eps, _ = inputs(False, 2, 1, h, w)
        a = model(x.to(device), caption_enc=cap.to(device), eps=eps.to(device))
        plan = model._last_plan
        b = model(x.to(device), caption_enc=cap.to(device), eps=eps.to(device), variations=1)
        assert model._last_plan is plan and len(model._plans) == 1 and model.get_plan(2, h, w, variations=1) is model.get_plan(2, h, w) is plan
        assert torch.equal(a, b)
        assert all(opc != K.OP_REPEAT for opc, _, _ in program_of(plan)) and plan.V == 1
        assert model.get_plan(2, h, w, variations=2) is not plan and len(model._plans) == 2
        import pytest
        with pytest.raises(ValueError):
            model(x.to(device), caption_enc=cap.to(device), eps=eps.to(device), variations=0)
    finally:
        model.release_plans()


SEEDS = [[7, (1 << 40) + 7, 8], [9, 7, 0xFEDCBA9876543210]]          # [B][V]; seed 7 twice: the same noise in two slots


def want_noise(per_image, seeds, step, stream):
    """fp32 [len(seeds), per_image] of tests/randn_ref.py and the radii (the error bound of the transform scales with them)."""
    vals, rads = zip(*(rc.want_normal(per_image, s, step, stream) for s in seeds))
    return np.stack(vals), np.stack(rads)


def check_seeds(lib, device, stochastic, graph, h=16, w=24, dtype=torch.float32):
    """Nested [B][V] seeds through rng="per_image": slot b * V + v draws i2i_randn at seed [b][v]; bit-reproducible; a graph captured from
    the program and replayed after set_seeds gives the eager run's bits."""
    from img2img_turbo_amd import rng
    B, V = len(SEEDS), len(SEEDS[0])
    flat = [s for row in SEEDS for s in row]
    model = make_model(lib, device, stochastic, dtype)
    try:
        x, cap, _, _ = inputs(stochastic, B, V, h, w)
        kw = dict(caption_enc=cap.to(device), deterministic=not stochastic, r=0.4 if stochastic else 1.0, variations=V)
        out = model.forward(x.to(device), seed=SEEDS, **kw)
        plan = model._last_plan
        assert plan.rng_per_image and plan.rng_state.shape == (B * V, 4) and plan.eps.shape[0] == B * V
        assert [rc.read_state(r) for r in plan.rng_state] == [rng.pack_state(s, 1) for s in flat]
        lat = 4 * (h // 8) * (w // 8)
        for name, buf, stream in (("eps", plan.eps, 0), ("noise", plan.noise, 2)):
            if buf is None:
                assert not stochastic
                continue
            got = buf.cpu().view(B * V, lat)
            # bit-equal to the library's own i2i_randn at that slot's seed ...
            for i, s in enumerate(flat):
                assert torch.equal(got[i].view(torch.int32), rng.randn((lat,), s, 0, stream=stream, device=device, lib=lib).cpu().view(torch.int32)), (name, i)
            # ... which is within the contract's bound of the fp64 oracle
            want, rad = want_noise(lat, flat, 0, stream)
            assert (np.abs(got.numpy().astype(np.float64) - want) <= rad * rc.TOL + 1e-30).all(), name
        assert torch.equal(plan.eps[0], plan.eps[4]) and not torch.equal(plan.eps[0], plan.eps[1])          # seed 7 in slots 0 and 4
        assert out.shape[0] == B * V and torch.equal(model.forward(x.to(device), seed=flat, **kw), out)         # flat form, and reproducible
        assert not torch.equal(out[0], out[1])
        eps0 = plan.eps.clone()
        # a graph (or, on the emulator, the eager program) replayed after set_seeds
        plan._prepare()
        plan.set_seeds(SEEDS)
        if graph:
            g = lib.graph_create(plan.prog)
            try:
                lib.graph_launch(g, plan.stream())
                sync(device)
                assert torch.equal(plan.out, out) and torch.equal(plan.eps.view(torch.int32), eps0.view(torch.int32))
                lib.graph_launch(g, plan.stream())           # step 1: fresh noise without the host
                sync(device)
                assert not torch.equal(plan.out, out)
                plan.set_seeds(flat)
                lib.graph_launch(g, plan.stream())
                sync(device)
                assert torch.equal(plan.out, out)
            finally:
                sync(device)
                lib.graph_destroy(g)
        else:
            plan.run()
            sync(device)
            assert torch.equal(plan.out, out) and torch.equal(plan.eps.view(torch.int32), eps0.view(torch.int32))
        import pytest
        with pytest.raises(ValueError):
            model.forward(x.to(device), seed=[1, 2, 3], **kw)
        with pytest.raises(ValueError):
            model.forward(x.to(device), seed=[[1, 2], [3, 4]], **kw)
        with pytest.raises(ValueError):
            plan.set_seeds([1] * B)
    finally:
        model.release_plans()


def check_u8_canny(lib, device, B=2, V=2, h=40, w=56, dtype=torch.float32):
    """forward_u8(canny=, variations=): edges once per input, B maps returned, bit-equal to tests/canny_ref.py; B * V uint8 images that are
    what forward_u8 of the repeated edge maps gives."""
    import canny_cases as cc
    model = make_model(lib, device, dtype=dtype)
    try:
        img, cap, _ = cc.pipeline_inputs(B, h, w)
        eps = torch.randn(B * V, 4, h // 8, w // 8, generator=torch.Generator().manual_seed(5))
        imgd, capd, epsd = cc.to_dev(img, device), cap.to(device), eps.to(device)
        thr = [(100, 200), (60, 120)]
        out, edges = model.forward_u8(imgd, caption_enc=capd, eps=epsd, canny=thr, variations=V, return_edges=True)
        plan = model._last_plan
        assert out.shape == (B * V, h, w, 3) and out.dtype == torch.uint8 and edges.shape == (B, h, w, 3)
        assert plan.canny_edges.shape[0] == B and plan.canny_thr.shape == (B, 2) and plan.x_in.shape[0] == B
        for b in range(B):
            assert np.array_equal(edges[b].cpu().numpy(), canny_ref.canny(img[b], thr[b][0], thr[b][1], 3)), b
        assert edges.any() and not edges.all()
        out_host = model.forward_u8(edges.repeat_interleave(V, 0), caption_enc=capd, eps=epsd)
        assert torch.equal(out, out_host)
        assert not torch.equal(out[0], out[1])
        # one pair for every image, and the scalar-threshold plan
        out1, edges1 = model.forward_u8(imgd, caption_enc=capd, eps=epsd, canny=(100, 200), variations=V, return_edges=True)
        assert edges1.shape == (B, h, w, 3) and torch.equal(edges1[0], edges[0]) and torch.equal(out1[:V], out[:V])
    finally:
        model.release_plans()


def check_plan_file(lib, device, tmp_path, B=2, V=3, h=16, w=24, dtype=torch.float32):
    """Export the variations plan (per-image seeds), then plan_load / plan_write ("x" at B, "seed" at B * V) / plan_run / plan_read give the
    bits of the Python replay; i2i_plan_verify passes; the command-line exporter takes --variations."""
    from img2img_turbo_amd import plan_file, rng
    model = make_model(lib, device, dtype=dtype)
    try:
        x, cap, _, _ = inputs(False, B, V, h, w)
        seeds = [[11 + 10 * b + v for v in range(V)] for b in range(B)]
        flat = [s for row in seeds for s in row]
        plan = model.get_plan(B, h, w, rng="per_image", variations=V)
        plan.set_seeds([1] * (B * V))
        path = str(tmp_path / "variations.i2iplan")
        info = plan_file.export_plan(plan, path, digests=True)
        lat = 4 * (h // 8) * (w // 8)
        assert info["io"]["x"] == B * 3 * h * w * 4 and info["io"]["eps"] == B * V * lat * 4 and info["io"]["seed"] == 16 * B * V
        assert info["io"]["out"] == B * V * 3 * h * w * plan.out.element_size() and info["digests"] > 0
        model.forward(x.to(device), caption_enc=cap.to(device), seed=seeds, variations=V)
        assert model._last_plan is plan
        want = plan.out.cpu()                     # (in the plan's output dtype, as the file holds it)
        eps = plan.eps.cpu()
        table = rc.state_tensor([w_ for row in rng.pack_states(flat) for w_ in row], "cpu")
        hd = lib.plan_load(path)
        try:
            assert lib.plan_verify(hd)[0] == 0
            assert lib.plan_io(hd, "x")[1] == x.numel() * 4 and lib.plan_io(hd, "seed")[1] == 16 * B * V == table.numel() * 4
            lib.plan_write(hd, "x", x)
            lib.plan_write(hd, "ctx", cap.to(plan.ctx.dtype))
            lib.plan_write(hd, "seed", table)
            lib.plan_run(hd, torch.cuda.current_stream().cuda_stream if device != "cpu" else 0)
            assert torch.equal(lib.plan_read(hd, "out", torch.zeros_like(want)), want)
            assert torch.equal(lib.plan_read(hd, "eps", torch.zeros_like(eps)).view(torch.int32), eps.view(torch.int32))
            assert rc.read_state(lib.plan_read(hd, "seed", torch.zeros(4 * B * V, dtype=torch.int32))) == [w_ for row in rng.pack_states(flat, 1) for w_ in row]
            assert lib.plan_verify(hd)[0] == 0
        finally:
            lib.plan_destroy(hd)
    finally:
        model.release_plans()


def check_cli(lib, device, tmp_path):
    from img2img_turbo_amd import plan_file
    cli = str(tmp_path / "cli.i2iplan")
    plan_file.main(["--out", cli, "--synthetic", "--arch", "tiny", "--batch", "2", "--variations", "3", "--size", "16", "24", "--dtype", "f32",
                    "--seeds", "1,2,3,4,5,6", "--device", device, "--lib", lib.path])
    hd = lib.plan_load(cli)
    try:
        assert lib.plan_io(hd, "x")[1] == 2 * 3 * 16 * 24 * 4 and lib.plan_io(hd, "out")[1] == 6 * 3 * 16 * 24 * 4
        assert lib.plan_io(hd, "eps")[1] == 6 * 4 * 2 * 3 * 4 and lib.plan_io(hd, "seed")[1] == 16 * 6
    finally:
        lib.plan_destroy(hd)
    import pytest
    for bad in (["--variations", "0"], ["--variations", "3", "--seeds", "1,2"], ["--variations", "2", "--model", "cyclegan"]):
        with pytest.raises(SystemExit):
            plan_file.main(["--out", cli + ".no", "--synthetic", "--arch", "tiny", "--batch", "2", "--size", "16", "24", "--dtype", "f32",
                            "--device", device, "--lib", lib.path] + bad)


def check_health_per_image_raises(lib, device):
    import pytest
    from img2img_turbo_amd.plan import ForwardPlan
    model = make_model(lib, device, health="stages", health_per_image=True)
    try:
        with pytest.raises(ValueError, match="health_per_image.*variations|variations.*health_per_image"):
            model.get_plan(2, 16, 24, variations=2)
        x, cap, eps, _ = inputs(False, 2, 2, 16, 24)
        with pytest.raises(ValueError, match="health_per_image"):
            model(x.to(device), caption_enc=cap.to(device), eps=eps.to(device), variations=2)
        with pytest.raises(ValueError, match="health_per_image"):
            ForwardPlan(lib, model.weights, 2, 16, 24, torch.float32, model.device_, health="stages", health_per_image=True, variations=2)
        assert model.get_plan(2, 16, 24).health_per_image             # without variations the model plans as before
    finally:
        model.release_plans()

"""Shared cases of the device fingerprint (i2i_digest, csrc/elementwise.hip digest_kernel; ForwardPlan(fingerprint=...), plan.py; the digest
section of plan files, csrc/plan_file.hip) for the CPU emulator (tests/test_digest_emu.py) and an MI355X (tests/test_digest_gpu.py).  The oracle
is tests/digest_ref.py, compared bit for bit.

The sizes come from the kernel's constants (csrc/elementwise.hip): SCAN_THREADS = 256 lanes, SCAN_UNROLL = 4 chunks of 16 bytes per lane and
round, so a workgroup strides over WG_CHUNKS = 1024 chunks (16 KiB) per round, and DIGEST_MAX_GRID = 1024 workgroups per launch at most: ONE
image fills the capped grid at 16 MiB, and anything past that runs the grid-stride loop a second time.
"""
import ctypes as C

import numpy as np
import torch

import digest_ref as R
import health_cases as hc

WG_CHUNKS, DIGEST_MAX_GRID = 256 * 4, 1024
GUARD = 0x5A5AA5A5C3C33C3C


def formats():
    from img2img_turbo_amd import _capi as K
    return {"u8": (1, K.U8), "f16": (2, K.F16), "bf16": (2, K.BF16), "f32": (4, K.F32)}


FMTS = ["u8", "f16", "bf16", "f32"]


def words(n, esz, seed):
    """n random bit patterns of esz bytes: every pattern of the format, NaNs, infinities and both zeros included."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 2 ** (8 * esz), size=n, dtype=np.int64).astype(R.WORD[esz])


def on_device(flat, device, offset=0, fill=0xA5):
    """The words in an allocation of their own, `offset` elements past its 16-byte aligned start; 16 elements of `fill` bytes behind them."""
    esz = flat.dtype.itemsize
    host = np.full((offset + flat.size + 16) * esz, fill, dtype=np.uint8).view(flat.dtype)
    host[offset:offset + flat.size] = flat
    buf = torch.from_numpy(host.view(np.uint8)).to(device)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + offset * esz


def records(n, device):
    """n zeroed records with one guard record in front and one behind: (tensor, pointer to record 0)."""
    host = np.zeros((n + 2, 4), dtype=np.uint64)
    host[0], host[-1] = GUARD, GUARD
    t = torch.from_numpy(host.view(np.int64)).to(device)
    return t, t.data_ptr() + 32


def read(t):
    a = t.cpu().numpy().view(np.uint64)
    assert (a[0] == GUARD).all() and (a[-1] == GUARD).all(), "a guard record was written"
    return a[1:-1].copy()


def call(lib, device, x_ptr, code, rec_ptr, *, images=1, rows=1, cols=0, ld=None, img_stride=None, index0=0, kind=0, n_records=0):
    from img2img_turbo_amd import _capi as K
    p = K.DigestParams()
    ld = cols if ld is None else ld
    p.x, p.images, p.rows, p.cols, p.ld, p.rec, p.kind, p.n_records = x_ptr, images, rows, cols, ld, rec_ptr, kind, n_records
    p.img_stride, p.index0 = (rows * ld if img_stride is None else img_stride), index0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None
    rc = lib.lib.i2i_digest(C.addressof(p), code, stream)
    hc.sync(device)
    return rc


def run(lib, device, flat, code, *, offset=0, **kw):
    """One launch over `flat` placed `offset` elements past a 16-byte boundary -> the records (images x 4)."""
    buf, x_ptr = on_device(flat, device, offset)
    rec, rec_ptr = records(kw.get("images", 1), device)
    rc = call(lib, device, x_ptr, code, rec_ptr, **kw)
    assert rc == 0, (rc, lib.lib.i2i_last_error().decode())
    return read(rec)


# ---------------------------------------------------------------------------------------------------------------- op cases
def check_lengths(lib, device, fmt):
    """Contiguous views of 0, 1, 15, 16, 17 and 4097 elements from start addresses 0, 1 and 3 elements past a 16-byte boundary: head only,
    head + chunks, chunks + tail, several chunks per lane."""
    esz, code = formats()[fmt]
    for n in (0, 1, 15, 16, 17, 4097):
        flat = words(n, esz, 100 + n)
        want = R.digest_ref(flat, 1, n)
        for off in (0, 1, 3):
            got = run(lib, device, flat, code, offset=off, cols=n)
            assert np.array_equal(got[0], want), (fmt, n, off, got.tolist(), want.tolist())


def check_pitched(lib, device, fmt):
    """7 x 33 with ld = 40 (rows 16-byte aligned for the 2-byte types: the chunk path of the pitched kernel) and ld = 35 (element loads); the
    pads hold garbage, and other garbage gives the same record."""
    esz, code = formats()[fmt]
    body = words(7 * 33, esz, 7).reshape(7, 33)
    want = R.digest_ref(body.reshape(-1), 7, 33)
    for ld in (40, 35):
        for pad_seed in (1, 2):
            flat = words(6 * ld + 33, esz, 50 + pad_seed)
            for r in range(7):
                flat[r * ld:r * ld + 33] = body[r]
            assert np.array_equal(R.digest_ref(flat, 7, 33, ld), want)
            got = run(lib, device, flat, code, rows=7, cols=33, ld=ld)
            assert np.array_equal(got[0], want), (fmt, ld, pad_seed, got.tolist(), want.tolist())


def check_images(lib, device, fmt):
    """Three images whose starts are 135 elements apart (no multiple of 16 bytes in any format): record b equals the single-image call on
    view b alone, and the oracle."""
    esz, code = formats()[fmt]
    rows, cols, stride = 4, 33, 135
    flat = words(2 * stride + rows * cols, esz, 9)
    got = run(lib, device, flat, code, images=3, rows=rows, cols=cols, img_stride=stride)
    for b in range(3):
        view = flat[b * stride:b * stride + rows * cols]
        alone = run(lib, device, view, code, offset=(b * stride) % (16 // esz), rows=rows, cols=cols)
        assert np.array_equal(got[b], alone[0]) and np.array_equal(got[b], R.digest_ref(view, rows, cols)), (fmt, b)


def check_capped_grid(lib, device):
    """One image of 16 MiB + 65 chunks + 5 bytes: it occupies all DIGEST_MAX_GRID workgroups, and the first of them run the grid-stride loop
    a second time (a whole round, a partial round, and a tail)."""
    esz, code = formats()["u8"]
    n = DIGEST_MAX_GRID * WG_CHUNKS * 16 + 65 * 16 + 5
    flat = words(n, esz, 3)
    got = run(lib, device, flat, code, cols=n)
    assert np.array_equal(got[0], R.digest_ref(flat, 1, n)), got.tolist()


def check_index_carry(lib, device, fmt):
    """index0 = 2^32 - 5 over 64 elements: the carry into the high half of the index; and index0 = 2^64 - 5, which wraps."""
    esz, code = formats()[fmt]
    flat = words(64, esz, 11)
    for index0 in (2 ** 32 - 5, 2 ** 64 - 5):
        got = run(lib, device, flat, code, offset=1, cols=64, index0=index0)
        assert np.array_equal(got[0], R.digest_ref(flat, 1, 64, index0=index0)), (fmt, index0)
    assert not np.array_equal(R.digest_ref(flat, 1, 64, index0=2 ** 32 - 5)[:2], R.digest_ref(flat, 1, 64, index0=2 ** 32 - 6)[:2])


def check_piecewise(lib, device, fmt):
    """digest(1000 elements) = digest(first 333) + digest(the rest, index0 = 333), on the device."""
    esz, code = formats()[fmt]
    flat = words(1000, esz, 13)
    whole = run(lib, device, flat, code, cols=1000)[0]
    a = run(lib, device, flat[:333], code, cols=333)[0]
    b = run(lib, device, flat[333:], code, offset=333 % (16 // esz), cols=667, index0=333)[0]
    assert np.array_equal(whole, R.add(a, b)) and np.array_equal(whole, R.digest_ref(flat, 1, 1000))


def check_accumulate_clear(lib, device):
    """Two launches into one record add up; CLEAR zeroes exactly n_records records and leaves the one behind them alone."""
    esz, code = formats()["bf16"]
    flat = words(300, esz, 17)
    buf, x_ptr = on_device(flat, device)
    rec, rec_ptr = records(3, device)
    one = R.digest_ref(flat, 1, 300)
    for _ in range(2):
        assert call(lib, device, x_ptr, code, rec_ptr, cols=300) == 0
        assert call(lib, device, x_ptr, code, rec_ptr + 64, cols=300) == 0
    got = read(rec)
    assert np.array_equal(got[0], R.add(one, one)) and not got[1].any() and np.array_equal(got[2], got[0])
    assert call(lib, device, 0, code, rec_ptr, kind=1, n_records=2) == 0
    got = read(rec)
    assert not got[:2].any() and np.array_equal(got[2], R.add(one, one))
    assert call(lib, device, 0, code, rec_ptr, kind=1, n_records=0) == 0 and np.array_equal(read(rec), got)


def check_sensitivity(lib, device, every_bit):
    """64 bf16 elements: flipping any single one of the 1024 bits gives a record different from the original and from every other flip
    (``every_bit``; otherwise bit 0 of element 0, the sign of element 63 and a bit in the middle); swapping two unequal elements changes it;
    -0.0 and +0.0 differ."""
    esz, code = formats()["bf16"]
    flat = words(64, esz, 19)
    base = run(lib, device, flat, code, cols=64)[0]
    assert np.array_equal(base, R.digest_ref(flat, 1, 64))
    seen = {tuple(base[:2].tolist())}
    bits = range(1024) if every_bit else (0, 517, 1023)
    for bit in bits:
        f = flat.copy()
        f[bit // 16] ^= np.uint16(1 << (bit % 16))
        got = run(lib, device, f, code, cols=64)[0]
        assert np.array_equal(got, R.digest_ref(f, 1, 64)) and got[2] == 64
        seen.add(tuple(got[:2].tolist()))
    assert len(seen) == len(bits) + 1, "two single-bit changes share a record"
    f = flat.copy()
    assert f[3] != f[40]
    f[3], f[40] = flat[40], flat[3]
    got = run(lib, device, f, code, cols=64)[0]
    assert np.array_equal(got, R.digest_ref(f, 1, 64)) and tuple(got[:2].tolist()) not in seen
    z = np.zeros(8, dtype=np.uint16)
    mz = z.copy()
    mz[5] = 0x8000
    assert not np.array_equal(run(lib, device, z, code, cols=8)[0], run(lib, device, mz, code, cols=8)[0])


def check_refusals(lib, device):
    from img2img_turbo_amd import _capi as K
    esz, code = formats()["f32"]
    flat = words(64, esz, 23)
    buf, x_ptr = on_device(flat, device)
    rec, rec_ptr = records(1, device)
    ok = dict(images=1, rows=2, cols=8, ld=8)
    bad = [dict(ok, cols=9), dict(ok, rows=-1), dict(ok, images=-1), dict(ok, images=2, img_stride=15), dict(ok, kind=7)]
    for kw in bad:
        assert call(lib, device, x_ptr, code, rec_ptr, **kw) == -1, kw
        assert lib.lib.i2i_last_error().decode().startswith("digest:"), kw
    assert call(lib, device, x_ptr + 2, code, rec_ptr, **ok) == -1          # x not aligned to an fp32
    assert call(lib, device, x_ptr, code, rec_ptr + 4, **ok) == -1          # rec not aligned
    assert call(lib, device, 0, code, rec_ptr, **ok) == -1 and call(lib, device, x_ptr, code, 0, **ok) == -1
    assert call(lib, device, x_ptr, 9, rec_ptr, **ok) == -1                 # no such dtype
    assert call(lib, device, 0, code, rec_ptr, kind=1, n_records=-1) == -1
    assert lib.lib.i2i_digest(None, code, None) == -1
    # the no-ops: nothing is written, and nothing is needed
    assert call(lib, device, 0, code, 0, images=0, rows=2, cols=8) == 0 and call(lib, device, 0, code, 0, images=1, rows=0, cols=8) == 0
    assert call(lib, device, 0, code, 0, images=1, rows=3, cols=0) == 0
    assert not read(rec).any()
    assert K.OP_DIGEST == 25


def check_eager(lib, device):
    """digest.digest: contiguous tensors, a [rows, cols] view with a pitch, a batch; and first_diff."""
    from img2img_turbo_amd.digest import digest, first_diff
    g = torch.Generator().manual_seed(5)
    t = torch.randn(3, 7, 40, generator=g).to(torch.bfloat16).to(device)
    bits = R.bits_of(t)
    assert np.array_equal(digest(t, lib=lib).numpy(), R.digest_ref(bits, 1, bits.size)[None])
    assert np.array_equal(digest(t, images=3, lib=lib).numpy(), R.digest_batch_ref(bits, 3, 1, 280))
    v = t[:, :, :33]
    assert np.array_equal(digest(v, images=3, lib=lib).numpy(), R.digest_batch_ref(bits, 3, 7, 33, ld=40, img_stride=280))
    assert np.array_equal(digest(v[1], lib=lib).numpy()[0], R.digest_ref(bits[280:], 7, 33, 40))
    assert np.array_equal(digest(t, images=3, index0=2 ** 40, lib=lib).numpy(), R.digest_batch_ref(bits, 3, 1, 280, index0=2 ** 40))
    u = torch.arange(100, dtype=torch.uint8).to(device)
    assert np.array_equal(digest(u, lib=lib).numpy()[0], R.digest_ref(np.arange(100, dtype=np.uint8), 1, 100))
    a = [("one", digest(t, images=3, lib=lib)), ("two", digest(u, lib=lib))]
    t2 = t.clone()
    t2[2, 0, 0] = -t2[2, 0, 0]
    b = [("one", digest(t2, images=3, lib=lib)), ("two", digest(u, lib=lib))]
    assert first_diff(a, a) is None and first_diff(a, b) == ("one", 2)


# ---------------------------------------------------------------------------------------------------------------- the planned forward
B, H, W, DTYPE = 3, 16, 24, torch.bfloat16


def make_model(lib, device, fingerprint="stages", **kw):
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    if fingerprint != "absent":
        kw["fingerprint"] = fingerprint
    return Pix2Pix_Turbo(weights=hc.tiny_weights(), device=device, dtype=DTYPE, lib=lib, **kw)


def program_of(plan):
    return [(opc, dt, label) for opc, dt, _p, label in plan.prog.ops]


def check_default_unchanged(lib, device):
    """fingerprint=None builds the program a model without the keyword builds, op for op; "stages" adds one CLEAR and one op per tap."""
    a = make_model(lib, device, "absent").get_plan(B, H, W)
    b = make_model(lib, device, None).get_plan(B, H, W)
    assert program_of(a) == program_of(b) and a.prog.n == b.prog.n and b.fingerprint_rec is None and not hasattr(b, "_fp_i64")
    assert len(a.pool.all) == len(b.pool.all)
    c = make_model(lib, device, "stages").get_plan(B, H, W)
    n = len(c.fingerprint_labels)
    assert n > 5 and c.prog.n == a.prog.n + n + 1 and program_of(c)[0][2] == "fingerprint: clear"
    assert [o for o in program_of(c) if not o[2].startswith("fingerprint: ")] == program_of(a)
    # the same taps, in the same places, as health=
    h = make_model(lib, device, None, health="stages", health_per_image=True).get_plan(B, H, W)
    assert h.health_labels == c.fingerprint_labels
    both = make_model(lib, device, "stages", health="stages", health_per_image=True).get_plan(B, H, W)
    assert [l for _, _, l in program_of(both)[:2]] == ["health: clear", "fingerprint: clear"]
    assert [l[len("health: "):] for _, _, l in program_of(both) if l.startswith("health: ")][1:-1] == \
           [l[len("fingerprint: "):] for _, _, l in program_of(both) if l.startswith("fingerprint: ")][1:]


def forward(model, x, cap, eps, replay=False):
    plan = model.get_plan(B, H, W)
    model.stage(plan, x, cap, eps)
    plan.replay() if replay else plan.run()
    model._last_plan = plan
    return model.fingerprint(), plan.out.clone()


def check_repeatable(lib, device, graph):
    """Two runs on the same inputs give equal records (on the GPU also: an eager run and a hipGraph replay); every record counts its
    elements; other inputs give other records."""
    from img2img_turbo_amd.digest import first_diff
    model = make_model(lib, device, "stages")
    x, cap, eps = hc.tiny_inputs(device, B, H, W)
    fa, oa = forward(model, x, cap, eps)
    fb, ob = forward(model, x, cap, eps, replay=graph)
    assert first_diff(fa, fb) is None and torch.equal(oa, ob)
    assert all((r.numpy()[:, 2] > 0).all() and not r.numpy()[:, 3].any() for _, r in fa)
    fc, _ = forward(model, x, cap, eps * 1.5, replay=graph)
    assert first_diff(fa, fc) is not None
    model.release_plans()


def check_images_independent(lib, device):
    """B = 3: one changed input value of image 1 changes image 1's record at the first tap and leaves EVERY record of images 0 and 2 equal."""
    from img2img_turbo_amd.digest import first_diff
    model = make_model(lib, device, "stages")
    x, cap, eps = hc.tiny_inputs(device, B, H, W)
    fa, _ = forward(model, x, cap, eps)
    x2 = x.clone()
    x2[1, 0, 3, 5] += 0.25
    fb, _ = forward(model, x2, cap, eps)
    assert first_diff(fa, fb) == (fa[0][0], 1)
    for (label, ra), (_, rb) in zip(fa, fb):
        assert torch.equal(ra.view(torch.int64)[[0, 2]], rb.view(torch.int64)[[0, 2]]), label
    assert not torch.equal(fa[-1][1].view(torch.int64)[1], fb[-1][1].view(torch.int64)[1])
    model.release_plans()


def check_weights_fingerprint(lib, device):
    """weights_fingerprint() is equal before and after set_lora_scale(0.4) -> 0.8 -> 0.4, and different at 0.8."""
    model = make_model(lib, device, None, live_scale=True)
    plan = model.get_plan(B, H, W, stochastic=True, r=0.4)
    plan._prepare()
    ra, ta = model.weights_fingerprint()
    assert len(ra) > 10 and all(int(r[2]) > 0 for _, r in ra)
    total = torch.stack([r.view(torch.int64) for _, r in ra]).sum(0)
    assert torch.equal(total, ta.view(torch.int64))
    model.set_lora_scale(0.8)
    rb, tb = model.weights_fingerprint()
    model.set_lora_scale(0.4)
    rc, tc = model.weights_fingerprint()
    assert torch.equal(ta.view(torch.int64), tc.view(torch.int64)) and not torch.equal(ta.view(torch.int64)[:2], tb.view(torch.int64)[:2])
    assert all(torch.equal(p.view(torch.int64), q.view(torch.int64)) for (_, p), (_, q) in zip(ra, rc))
    assert [l for l, _ in ra] == [l for l, _ in rb] and torch.equal(ta.view(torch.int64)[2:], tb.view(torch.int64)[2:])
    model.release_plans()


def check_io(lib, device):
    """"io" gives exactly the boundary labels, and the records are the oracle's over the boundary buffers."""
    model = make_model(lib, device, "io")
    x, cap, eps = hc.tiny_inputs(device, B, H, W)
    f, _ = forward(model, x, cap, eps)
    plan = model.get_plan(B, H, W)
    assert [l for l, _ in f] == ["x", "ctx", "eps", "out"]
    for (label, rec), t, images in zip(f, (plan.x_in, plan.ctx, plan.eps, plan.out), (B, 1, B, B)):
        bits = R.bits_of(t)
        want = R.digest_batch_ref(bits, images, 1, bits.size // images)
        assert np.array_equal(rec.numpy()[:images], want), label
        assert not rec.numpy()[images:].any(), label
    model.release_plans()


# ---------------------------------------------------------------------------------------------------------------- plan files
def export(lib, device, path, *flags):
    from img2img_turbo_amd import plan_file
    plan_file.main(["--out", path, "--batch", str(B), "--size", str(H), str(W), "--dtype", "bf16", "--synthetic", "--arch", "tiny",
                    "--device", device, "--lib", lib.path] + list(flags))


def digest_section(path):
    """(offset of the section, [(buf, s0, s1, elements)]) of a file exported with digests."""
    import struct
    raw = open(path, "rb").read()
    at = raw.rfind(b"I2IDIGS1")
    assert at > 0
    n = struct.unpack_from("<I", raw, at + 8)[0]
    assert len(raw) == at + 16 + 32 * n
    return at, [struct.unpack_from("<IIQQQ", raw, at + 16 + 32 * i)[::1] for i in range(n)]


def buffer_table(path):
    """[(bytes, kind, file offset of the contents or None)] of a plan file (csrc/plan_file.hip has the layout)."""
    import struct
    raw = open(path, "rb").read()
    abi, sizeof_op, n_ops, n_bufs, n_relocs, n_io = struct.unpack_from("<6I", raw, 8)
    at = 32
    if raw[:8] == b"I2IPLAN2":
        n_ops += struct.unpack_from("<I", raw, at)[0]
        at += 8
    bufs = [struct.unpack_from("<QII", raw, at + 16 * i)[:2] for i in range(n_bufs)]
    data = at + 16 * n_bufs + 48 * n_io + 24 * n_relocs + sizeof_op * n_ops
    out = []
    for nbytes, kind in bufs:
        out.append((nbytes, kind, data if kind == 1 else None))
        if kind == 1:
            data += nbytes
    return out


def check_plan_verify(lib, device, tmp_path):
    """A file with --digests verifies; one changed byte inside a weight buffer fails and names that buffer (a second file, another buffer:
    the rest is still reported equal); no digests -> UNSUPPORTED; a truncated section / an index out of range are refused at load."""
    from img2img_turbo_amd import _capi as K
    from img2img_turbo_amd import plan_file
    good, plain = str(tmp_path / "good.i2iplan"), str(tmp_path / "plain.i2iplan")
    model = make_model(lib, device, None)
    plan = model.get_plan(B, H, W)               # ONE plan exported twice: the buffer table follows the addresses of its tensors
    info = plan_file.export_plan(plan, good, digests=True)
    assert plan_file.export_plan(plan, plain)["digests"] == 0
    model.release_plans()
    raw = open(good, "rb").read()
    at, recs = digest_section(good)
    assert raw[:at] == open(plain, "rb").read(), "a file with digests is the plain file plus a trailing section"
    table = buffer_table(good)
    assert len(recs) > 10 and all(table[r[0]][1] == 1 and table[r[0]][0] == r[4] for r in recs)
    assert info["digests"] == len(recs) and info["digest_bytes"] == sum(r[4] for r in recs)

    def verify(path):
        h = lib.plan_load(path)
        try:
            return lib.plan_verify(h)
        finally:
            lib.plan_destroy(h)
    assert verify(good)[:2] == (0, -1)
    rc, bad, msg = verify(plain)
    assert rc == K.ERR_UNSUPPORTED and "digests" in msg
    big = sorted(recs, key=lambda r: -r[4])
    for victim in (big[0], big[3]):
        flipped = bytearray(raw)
        flipped[table[victim[0]][2] + victim[4] // 2] ^= 0x10
        path = str(tmp_path / ("flipped%d.i2iplan" % victim[0]))
        open(path, "wb").write(bytes(flipped))
        rc, bad, msg = verify(path)
        assert rc == K.ERR_MISMATCH and bad == victim[0] and ("buffer %d " % victim[0]) in msg, (rc, bad, msg, victim)
    import struct
    for name, blob in (("cut", raw[:-8]), ("cut_magic", raw[:at + 5]), ("cut_count", raw[:at + 12]), ("longer", raw + b"\0"),
                       ("range", raw[:at + 16] + struct.pack("<I", len(table)) + raw[at + 20:]),
                       ("count", raw[:at + 8] + struct.pack("<I", len(table) + 1) + raw[at + 12:]),
                       ("twice", raw[:at + 16 + 32] + raw[at + 16:at + 48] + raw[at + 80:]),
                       ("size", raw[:at + 16 + 24] + struct.pack("<Q", recs[0][4] + 1) + raw[at + 48:])):
        path = str(tmp_path / (name + ".i2iplan"))
        open(path, "wb").write(blob)
        try:
            h = lib.plan_load(path)
        except K.I2IError as e:
            assert "plan_load" in str(e), (name, e)
        else:
            lib.plan_destroy(h)
            raise AssertionError("a plan file with a malformed digest section (%s) loaded" % name)


def check_plan_file_fingerprint(lib, device, tmp_path):
    """--fingerprint stages: "fingerprint" holds taps x B x 32 bytes and "fingerprint_names" the labels; after a run the records equal the
    Python replay's."""
    path = str(tmp_path / "fp.i2iplan")
    export(lib, device, path, "--fingerprint", "stages", "--digests")
    model = make_model(lib, device, "stages")
    x, cap, eps = hc.tiny_inputs(device, B, H, W)
    f, out = forward(model, x, cap, eps)
    names = b"".join(l.encode() + b"\0" for l, _ in f)
    h = lib.plan_load(path)
    try:
        assert lib.plan_io(h, "fingerprint")[1] == len(f) * B * 32 and lib.plan_io(h, "fingerprint_names")[1] == len(names)
        assert bytes(lib.plan_read(h, "fingerprint_names", torch.zeros(len(names), dtype=torch.uint8)).numpy()) == names
        assert lib.plan_verify(h)[0] == 0
        for _ in range(2):
            lib.plan_write(h, "x", x.cpu())
            lib.plan_write(h, "ctx", cap.to(DTYPE).cpu())
            lib.plan_write(h, "eps", eps.cpu())
            lib.plan_run(h)
            got = lib.plan_read(h, "fingerprint", torch.zeros(len(f), B, 4, dtype=torch.int64))
            assert torch.equal(got, torch.stack([r.view(torch.int64) for _, r in f]))
        assert torch.equal(lib.plan_read(h, "out", torch.zeros_like(out).cpu()), out.cpu())
        assert lib.plan_verify(h)[0] == 0          # a run does not touch what the digests cover
    finally:
        lib.plan_destroy(h)
    model.release_plans()
    return path

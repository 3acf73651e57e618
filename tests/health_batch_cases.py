"""Shared cases of the per-image health scan (i2i_scan_batch / i2i_scan_verdict, csrc/elementwise.hip; ForwardPlan(health_per_image=True)) for
the CPU emulator (tests/test_health_batch_emu.py) and an MI355X (tests/test_health_batch_gpu.py).  The oracle is tests/health_ref.py applied to
each image's view alone: the contract says record b equals, bit for bit, what i2i_scan writes for that view.  The verdict is a few lines of
numpy (verdict_ref).

The sizes come from the kernel's constants (csrc/elementwise.hip): SCAN_THREADS, SCAN_UNROLL as in health_cases, and
    SCAN_BATCH_MAX_GRID = 1024   workgroups of one launch at most: grid y = min(images, 1024), and an image gets at most
                                 share(images) = 1024 // grid y slices (workgroups) in x, each striding WG_CHUNKS chunks per round.
"""
import ctypes as C

import numpy as np
import torch

import health_cases as hc
import health_ref as R

SCAN_BATCH_MAX_GRID = 1024
LIMIT = hc.LIMIT
GUARD = 0x5A5AA5A5C3C33C3C


def share(images):
    return SCAN_BATCH_MAX_GRID // min(images, SCAN_BATCH_MAX_GRID)


def extent(rows, cols, ld):
    return (rows - 1) * ld + cols if rows > 0 else 0


def make_batch(images, rows, cols, ld, img_stride, dtype, seed, sprinkle=4, place=()):
    """Raw words of `images` views of rows x cols (pitch ld) that start img_stride elements apart.  Everything that is NOT inside [0, cols) of
    a row of an image -- the padding of the rows, the gaps between the images -- holds NaN / Inf patterns that must not be counted.
    ``sprinkle``: that many of the specials() patterns at random places of every image; ``place``: (image, element index, word) put last."""
    fmt = hc.FMT_OF[dtype]
    f = R.FMT[fmt]
    n = (images - 1) * img_stride + extent(rows, cols, ld)
    flat = np.empty(n, dtype=f["word"])
    flat[0::2] = f["inf"] | 1
    flat[1::2] = f["inf"]
    sp = hc.specials(fmt)
    body = hc.healthy_bits(images * rows * cols, dtype, seed).reshape(images, rows * cols)
    for b in range(images):
        rs = np.random.RandomState(seed * 131 + b)
        k = min(sprinkle, rows * cols)
        if k:
            body[b, rs.choice(rows * cols, size=k, replace=False)] = rs.choice(sp, size=k)
    for b, i, word in place:
        body[b, i] = word
    for b in range(images):
        for r in range(rows):
            at = b * img_stride + r * ld
            flat[at:at + cols] = body[b, r * cols:(r + 1) * cols]
    return flat


def ref_records(flat, images, rows, cols, ld, img_stride, limit, dtype):
    fmt = hc.FMT_OF[dtype]
    return np.stack([R.scan_ref(flat[b * img_stride:b * img_stride + extent(rows, cols, ld)], cols, ld, limit, fmt, rows=rows) for b in range(images)])


def stream_of(device):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None


def call(lib, device, x_ptr, images, rows, cols, ld, img_stride, limit, rec_ptr, rec_stride, dtype_code):
    from img2img_turbo_amd import _capi as K
    p = K.ScanBatchParams()
    p.x, p.images, p.rows, p.cols, p.ld, p.img_stride, p.limit, p.rec, p.rec_stride = x_ptr, images, rows, cols, ld, img_stride, limit, rec_ptr, rec_stride
    rc = lib.lib.i2i_scan_batch(C.addressof(p), dtype_code, stream_of(device))
    hc.sync(device)
    return rc


class Guarded:
    """`words` uint64 words at a 64-byte aligned address with 8 guard words in front and behind (and whatever else the caller leaves as
    guard inside): ``inner(mask)`` checks that every word outside ``mask`` still holds GUARD."""

    def __init__(self, words, device):
        host = np.full(words + 16, GUARD, dtype=np.uint64)
        raw = torch.empty(words + 16 + 8, dtype=torch.int64, device=device)          # (a host allocation need not be 64-byte aligned)
        skip = (-raw.data_ptr() % 64) // 8
        self.buf = raw[skip:skip + words + 16]
        self.buf.copy_(torch.from_numpy(host.view(np.int64)))
        assert self.buf.data_ptr() % 64 == 0
        self.ptr, self.words = self.buf.data_ptr() + 64, words

    def write(self, values, at=0):
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
        self.buf[8 + at:8 + at + v.size] = torch.from_numpy(v.view(np.int64)).to(self.buf.device)

    def read(self):
        return self.buf.cpu().numpy().view(np.uint64).copy()

    def inner(self):
        return self.read()[8:8 + self.words]

    def guards_intact(self, owned):
        """owned: boolean mask over the inner words that the kernel may write"""
        all_words = self.read()
        inner = all_words[8:8 + self.words]
        return (all_words[:8] == GUARD).all() and (all_words[8 + self.words:] == GUARD).all() and (inner[~owned] == GUARD).all()


def new_records(images, rec_stride, device):
    """Zeroed records rec_stride bytes apart inside a guarded buffer: (buffer, mask of the record words)."""
    sw = rec_stride // 8
    g = Guarded(images * sw, device)
    owned = np.zeros(images * sw, dtype=bool)
    for b in range(images):
        owned[b * sw:b * sw + 8] = True
        g.write(np.zeros(8, dtype=np.uint64), at=b * sw)
    return g, owned


def check_batch(lib, device, dtype, images, rows, cols, ld=None, img_stride=None, offset=0, seed=1, sprinkle=4, place=(), limit=LIMIT, launches=1,
                rec_stride=64):
    """One (or several accumulated) launches against the per-image oracle, bit for bit; guard words around the records.  Returns the records."""
    ld = cols if ld is None else ld
    img_stride = rows * ld if img_stride is None else img_stride
    flat = make_batch(images, rows, cols, ld, img_stride, dtype, seed, sprinkle, place)
    buf, x_ptr, code = hc.on_device(flat, dtype, device, offset)
    g, owned = new_records(images, rec_stride, device)
    one = ref_records(flat, images, rows, cols, ld, img_stride, limit, dtype)
    want = np.zeros_like(one)
    for _ in range(launches):
        rc = call(lib, device, x_ptr, images, rows, cols, ld, img_stride, limit, g.ptr, rec_stride, code)
        assert rc == 0, (rc, lib.lib.i2i_last_error().decode())
        want = np.stack([R.accumulate(w, o) for w, o in zip(want, one)])
    got = g.inner().reshape(images, rec_stride // 8)[:, :8]
    what = (str(dtype), images, rows, cols, ld, img_stride, offset, rec_stride)
    assert np.array_equal(got, want), (what, got.tolist(), want.tolist())
    assert g.guards_intact(owned), what
    assert (got[:, 0] == launches).all() and (got[:, 6] == launches * rows * cols).all() and not got[:, 7].any(), what
    return got


# ---------------------------------------------------------------------------------------------------------------- kernel cases
def check_misaligned(lib, device, dtype):
    """Contiguous images of 15 elements: the image starts walk through every misalignment (15 is odd, coprime to 4 and 8); the same one element
    past a 16-byte boundary; images shorter than a chunk; images of no rows at all."""
    for i, images in enumerate((1, 2, 3, 5)):
        for off in (0, 1):
            check_batch(lib, device, dtype, images, 3, 5, offset=off, seed=20 + i)
            check_batch(lib, device, dtype, images, 1, 3, offset=off, seed=30 + i, sprinkle=1)
        got = check_batch(lib, device, dtype, images, 0, 5, seed=40 + i)          # runs = 1, elements = 0, nothing read (all around is NaN)
        assert got.tolist() == [[1, 0, 0, 0, 0, 0, 0, 0]] * images


def check_multi_wg(lib, device, dtype):
    """2 and 3 images of one workgroup's stride + 3 chunks + 5 elements: a second slice with a partial round, per image, from a misaligned
    start for every image but the first."""
    e = hc.epc(dtype)
    n = hc.WG_CHUNKS * e + 3 * e + 5
    check_batch(lib, device, dtype, 2, 1, n, seed=50)
    check_batch(lib, device, dtype, 3, 1, n, offset=1, seed=51)
    check_batch(lib, device, dtype, 3, 7, n // 7, seed=52)                          # the same as rows (contiguous: one long row per image)


def check_grid_pass(lib, device, dtype):
    """One image of one round more than a single pass of its share of the capped grid (+ 5 elements): the second pass of the grid-stride
    loop inside an image.  With one image the share is the whole grid, SCAN_BATCH_MAX_GRID workgroups: 16 MiB and one round."""
    e = hc.epc(dtype)
    n = share(1) * hc.WG_CHUNKS * e + hc.WG_CHUNKS * e + 5
    got = check_batch(lib, device, dtype, 1, 1, n, seed=53, sprinkle=8)
    assert got[0, 6] == n


def check_strided(lib, device, dtype):
    """ld > cols and img_stride > rows * ld, NaN / Inf in every row's padding and in the gaps; pitches that keep rows 16-byte aligned (chunk
    path) and pitches that do not (element path), and gaps that misalign SOME images of an aligned pitch (both paths in one launch)."""
    e = hc.epc(dtype)
    check_batch(lib, device, dtype, 3, 4, 13, ld=16, seed=60)                                   # aligned pitch (16 elements = 32 / 64 bytes), aligned images
    check_batch(lib, device, dtype, 3, 3, 5, ld=9, seed=61)                                     # a pitch that keeps nothing aligned
    check_batch(lib, device, dtype, 3, 4, 13, ld=16, img_stride=4 * 16 + e, seed=62)            # a gap of one chunk: still aligned
    check_batch(lib, device, dtype, 3, 4, 13, ld=16, img_stride=4 * 16 + 3, seed=63)            # a gap of 3 elements: images 1, 2 fall off the chunk path
    check_batch(lib, device, dtype, 3, 3, 5, img_stride=15 + 2, seed=64)                        # contiguous images with a gap
    check_batch(lib, device, dtype, 2, 3, 3 * e, ld=4 * e, offset=1, seed=65)                   # aligned pitch from a misaligned base
    check_batch(lib, device, dtype, 2, 40, 33 * e + 3, ld=40 * e, seed=66)                      # 1320 chunks per image: two slices, the row division, tails
    check_batch(lib, device, dtype, 2, 300, 7, ld=9, img_stride=300 * 9 + 1, seed=67)           # 2100 element loads per image


def check_boundaries(lib, device, dtype):
    """One class of special value per image, at its first AND its last element: the last element of image b and the first of image b + 1
    are neighbours in memory and belong to different records.  The last image has none."""
    fmt = hc.FMT_OF[dtype]
    sp = hc.specials(fmt)
    images, n = len(sp) + 1, 15
    place = [(b, i, sp[b]) for b in range(len(sp)) for i in (0, n - 1)]
    got = check_batch(lib, device, dtype, images, 3, 5, seed=70, sprinkle=0, place=place)
    # +Inf, -Inf, two NaNs, -0, the smallest denormal, +-max finite, the limit, the next value above it: [n_nan, n_pos_inf, n_neg_inf, n_over]
    want = [[0, 2, 0, 0], [0, 0, 2, 0], [2, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 2], [0, 0, 0, 2], [0, 0, 0, 0], [0, 0, 0, 2],
            [0, 0, 0, 0]]
    assert got[:, 1:5].tolist() == want, got[:, 1:5].tolist()


def check_accumulate(lib, device, dtype):
    """Two launches accumulate (runs = 2, counts doubled, the max idempotent); records 128 bytes apart leave the 64 bytes between them alone
    (check_batch looks at the guard words between and around the records in every case)."""
    got = check_batch(lib, device, dtype, 3, 3, 5, seed=80, launches=2)
    assert (got[:, 0] == 2).all() and (got[:, 6] == 30).all()
    check_batch(lib, device, dtype, 3, 3, 5, seed=81, rec_stride=128)
    check_batch(lib, device, dtype, 2, 1, hc.WG_CHUNKS * hc.epc(dtype) + 5, seed=82, rec_stride=128, launches=2)


def check_refusals(lib, device):
    import pytest
    from img2img_turbo_amd import _capi as K
    rows, cols, ld, images = 4, 16, 16, 3
    flat = make_batch(images, rows, cols, ld, rows * ld, torch.float32, 1)
    buf, x, code = hc.on_device(flat, torch.float32, device)
    g, owned = new_records(images, 64, device)
    r = g.ptr
    bad = [dict(x=0), dict(rec=0),                                                    # null pointers
           dict(images=0), dict(images=-2),                                           # images < 1
           dict(rows=-1), dict(cols=-1), dict(ld=15),                                 # negative sizes, ld < cols
           dict(img_stride=(rows - 1) * ld + cols - 1), dict(img_stride=-64),         # img_stride smaller than an image's extent
           dict(limit=0.0), dict(limit=-1.0), dict(limit=float("nan")),               # limit must be > 0
           dict(rec=r + 8), dict(rec=r + 32),                                         # rec not 64-byte aligned
           dict(rec_stride=0), dict(rec_stride=32), dict(rec_stride=96), dict(rec_stride=-64),      # rec_stride not a multiple of 64, >= 64
           dict(x=x + 2),                                                             # x not aligned to its element
           dict(code=K.U8), dict(code=7)]                                             # not a float dtype
    for kw in bad:
        a = dict(x=x, images=images, rows=rows, cols=cols, ld=ld, img_stride=rows * ld, limit=1.0, rec=r, rec_stride=64, code=code)
        a.update(kw)
        rc = call(lib, device, a["x"], a["images"], a["rows"], a["cols"], a["ld"], a["img_stride"], a["limit"], a["rec"], a["rec_stride"], a["code"])
        assert rc == -1, (kw, rc)
        assert lib.lib.i2i_last_error().decode().startswith("scan_batch:"), kw
        with pytest.raises(K.I2IError):
            lib.check(rc)
    assert lib.lib.i2i_scan_batch(None, code, None) == -1
    assert not g.inner().any() and g.guards_intact(owned)                            # nothing was written by a refused call
    # the smallest stride that is allowed: the images touch
    assert call(lib, device, x, images, rows, cols - 1, ld, (rows - 1) * ld + cols - 1, 1.0, r, 64, code) == 0
    assert g.inner().reshape(images, 8)[:, 0].tolist() == [1] * images


# ---------------------------------------------------------------------------------------------------------------- the verdict
def verdict_ref(rec, verdict):
    """rec uint64 [taps][images][8], verdict uint32 [images][4] -> the rows after one JUDGE."""
    out = verdict.copy()
    for b in range(rec.shape[1]):
        bad = np.flatnonzero((rec[:, b, 1] | rec[:, b, 2] | rec[:, b, 3]) != 0)
        over = np.flatnonzero(rec[:, b, 4] != 0)
        out[b, 0] = bad[0] + 1 if bad.size else 0
        out[b, 1] = over[0] + 1 if over.size else 0
        out[b, 2] += 1
        out[b, 3] += 1 if bad.size else 0
    return out


def call_verdict(lib, device, rec_ptr, taps, images, verdict_ptr, mode):
    from img2img_turbo_amd import _capi as K
    p = K.ScanVerdictParams()
    p.rec, p.taps, p.images, p.verdict, p.mode = rec_ptr, taps, images, verdict_ptr, mode
    rc = lib.lib.i2i_scan_verdict(C.addressof(p), 0, stream_of(device))
    hc.sync(device)
    return rc


def check_verdict(lib, device):
    from img2img_turbo_amd import _capi as K
    taps, images = 4, 3
    # table A: image 0 bad at tap 0 (and again later), image 1 over at tap 1 and bad at the last tap, image 2 over only (tap 2)
    a = np.zeros((taps, images, 8), dtype=np.uint64)
    a[:, :, 0], a[:, :, 6], a[:, :, 5] = 1, 77, 0x3F800000
    a[0, 0, 1], a[2, 0, 2] = 5, 1
    a[1, 1, 4], a[3, 1, 3] = 2, 1 << 40           # (a count whose low 32 bits are zero is a count all the same)
    a[2, 2, 4] = 9
    # table B: image 0 clean, image 1 bad at taps 2 and 3 (+Inf), image 2 clean
    b = np.zeros_like(a)
    b[:, :, 0], b[:, :, 6] = 1, 77
    b[2, 1, 2], b[3, 1, 1] = 3, 4
    rec = Guarded(taps * images * 8, device)
    ver = Guarded(images * 2, device)            # images x 4 uint32 = images x 2 words
    all_rec, all_ver = np.ones(taps * images * 8, dtype=bool), np.ones(images * 2, dtype=bool)
    start = np.array([[9, 9, 10, 3], [9, 9, 10, 3], [9, 9, 0, 0]], dtype=np.uint32)      # stale first_bad / first_over, totals of earlier runs
    ver.write(start.view(np.uint64))
    rows = lambda: ver.inner().view(np.uint32).reshape(images, 4)
    want = start
    for table, first in ((a, [[1, 0], [4, 2], [0, 3]]), (b, [[0, 0], [3, 0], [0, 0]])):
        rec.write(table)
        assert call_verdict(lib, device, rec.ptr, taps, images, ver.ptr, K.VERDICT_JUDGE) == 0, lib.lib.i2i_last_error().decode()
        want = verdict_ref(table, want)
        assert want[:, :2].tolist() == first                                          # (the oracle itself, against the table as written above)
        assert np.array_equal(rows(), want), (rows().tolist(), want.tolist())
        assert np.array_equal(rec.inner().reshape(taps, images, 8), table)            # JUDGE only reads the records
    assert want[:, 2].tolist() == [12, 12, 2] and want[:, 3].tolist() == [4, 5, 0]
    # CLEAR zeroes the records and leaves the verdict alone (also when it is not given at all)
    for vptr in (ver.ptr, 0):
        rec.write(a)
        assert call_verdict(lib, device, rec.ptr, taps, images, vptr, K.VERDICT_CLEAR) == 0
        assert not rec.inner().any() and np.array_equal(rows(), want)
    # a JUDGE over cleared records: a clean run
    assert call_verdict(lib, device, rec.ptr, taps, images, ver.ptr, K.VERDICT_JUDGE) == 0
    want = verdict_ref(np.zeros_like(a), want)
    assert np.array_equal(rows(), want) and not want[:, :2].any()
    # fewer taps / images than the buffers hold: the rest is not touched (tap-major with the GIVEN image count)
    rec.write(np.full(taps * images * 8, GUARD, dtype=np.uint64))
    assert call_verdict(lib, device, rec.ptr, 2, 2, ver.ptr, K.VERDICT_CLEAR) == 0
    got = rec.inner()
    assert not got[:32].any() and (got[32:] == GUARD).all()
    assert call_verdict(lib, device, rec.ptr, 0, 2, ver.ptr, K.VERDICT_JUDGE) == 0      # no taps: the run is counted, nothing else
    want[:2, 2] += 1
    assert np.array_equal(rows(), want)
    assert rec.guards_intact(all_rec) and ver.guards_intact(all_ver)
    # refusals: nothing written
    before_r, before_v = rec.read(), ver.read()
    for kw in (dict(rec=0), dict(rec=rec.ptr + 4), dict(taps=-1), dict(images=0), dict(mode=2), dict(mode=-1), dict(verdict=0), dict(verdict=ver.ptr + 2)):
        args = dict(rec=rec.ptr, taps=taps, images=images, verdict=ver.ptr, mode=K.VERDICT_JUDGE)
        args.update(kw)
        assert call_verdict(lib, device, args["rec"], args["taps"], args["images"], args["verdict"], args["mode"]) == -1, kw
        assert lib.lib.i2i_last_error().decode().startswith("scan_verdict:"), kw
    assert lib.lib.i2i_scan_verdict(None, 0, None) == -1
    assert np.array_equal(rec.read(), before_r) and np.array_equal(ver.read(), before_v)


# ---------------------------------------------------------------------------------------------------------------- the planned forward
B, H, W = 3, 16, 24
DTYPE = torch.bfloat16


def make_model(lib, device, health="stages", per_image=True, weights=None, **plan_options):
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    return Pix2Pix_Turbo(weights=weights or hc.tiny_weights(), device=device, dtype=DTYPE, lib=lib, health=health, health_per_image=per_image,
                         plan_options=plan_options)


def again(plan, device):
    """One more execution of the staged plan: a graph replay on the GPU, a run on the emulator (which has no graphs)."""
    if device == "cpu":
        plan.run()
    else:
        plan.replay()


def records(plan):
    """uint64 [taps][B][8] of a per-image plan"""
    hc.sync(str(plan.device))
    n = len(plan.health_labels)
    return plan._health_i64.cpu().numpy().view(np.uint64)[:n * plan.B].reshape(n, plan.B, 8).copy()


def verdict_rows(plan):
    hc.sync(str(plan.device))
    return plan._verdict_i32.cpu().numpy().view(np.uint32).copy()


def check_forward_clean(lib, device):
    """Eager + two more executions of a clean batch: the image of a model without scans, verdict rows {0, 0, 3, 0}, and an aggregated report
    that equals, field by field, what a whole-batch health= plan reports after ONE run (the records are zeroed by every run)."""
    x, cap, eps = hc.tiny_inputs(device, B, H, W)
    plain = hc.make_model(lib, device, DTYPE, None)
    want = plain(x, caption_enc=cap, eps=eps)
    model = make_model(lib, device)
    plan = model.get_plan(B, H, W)
    model.stage(plan, x, cap, eps)
    plan.run()
    eager = plan.out.clone()
    again(plan, device)
    again(plan, device)
    model._last_plan = plan
    assert torch.equal(eager, want) and torch.equal(plan.out, want)
    assert verdict_rows(plan).tolist() == [[0, 0, 3, 0]] * B
    assert model.health_verdict() == [dict(image=b, first_bad=None, first_over=None, runs=3, bad_runs=0) for b in range(B)]
    whole = hc.make_model(lib, device, DTYPE, "stages")
    assert torch.equal(whole(x, caption_enc=cap, eps=eps), want)
    rep, rep_whole = model.health_report(), whole.health_report()
    assert [d["label"] for d in rep] == hc.stage_names(model.weights) == plan.health_labels
    assert rep == rep_whole, [(a, b) for a, b in zip(rep, rep_whole) if a != b]
    assert model.health_first_bad() is None
    # per image: the views of the tap tensors add up
    rec = records(plan)
    for i, (t, rows, cols, ld) in enumerate(plan.health_taps):
        assert (rec[i, :, 0] == 1).all() and (rec[i, :, 6] == rows // B * cols).all() and not rec[i, :, 1:4].any(), plan.health_labels[i]
    per = [model.health_report(image=b) for b in range(B)]
    for i, d in enumerate(rep):
        assert d["elements"] == sum(p[i]["elements"] for p in per) and d["max_abs"] == max(p[i]["max_abs"] for p in per) and d["runs"] == per[0][i]["runs"] == 1
        assert model.health_report(image=-1)[i] == per[B - 1][i]
    model.health_reset()
    assert not records(plan).any() and not verdict_rows(plan).any()
    for m in (plain, model, whole):
        m.release_plans()
    return want


def check_forward_one_bad(lib, device):
    """A NaN in eps[1] alone: the verdict names image 1 at "latents" (the posterior sample, the first stage downstream of eps); images 0 and
    2 are clean, in the verdict and in the pixels; a clean execution afterwards leaves first_bad = 0 everywhere and bad_runs = 1 for image 1."""
    x, cap, eps = hc.tiny_inputs(device, B, H, W)
    bad_eps = eps.clone()
    bad_eps[1, 0, 0, 0] = float("nan")
    model = make_model(lib, device)
    plan = model.get_plan(B, H, W)
    model.stage(plan, x, cap, eps)
    plan.run()
    clean = plan.out.clone()
    model._last_plan = plan
    model.health_reset()
    model.stage(plan, x, cap, bad_eps)
    again(plan, device)
    out = plan.out.clone()
    v = model.health_verdict()
    assert v[1] == dict(image=1, first_bad="latents", first_over=None, runs=1, bad_runs=1), v
    assert v[0] == dict(image=0, first_bad=None, first_over=None, runs=1, bad_runs=0) and v[2] == dict(image=2, first_bad=None, first_over=None, runs=1, bad_runs=0), v
    at = plan.health_labels.index("latents")
    rec = records(plan)
    assert not rec[:at, :, 1:4].any() and rec[at, 1, 1] == 1 and not rec[:, [0, 2], 1:4].any()
    assert model.health_first_bad()["label"] == "latents"                               # the aggregate sees it too
    assert model.health_report(image=0)[at]["n_nan"] == 0 and model.health_report(image=1)[at]["n_nan"] == 1
    # no kernel reduces across images: the neighbours of the bad request are bit-equal to the clean run
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
    model.stage(plan, x, cap, eps)
    again(plan, device)
    assert torch.equal(plan.out, clean)
    assert verdict_rows(plan).tolist() == [[0, 0, 2, 0], [0, 0, 2, 1], [0, 0, 2, 0]]
    assert not records(plan)[:, :, 1:4].any()                                         # the records describe THAT run
    model.release_plans()


def check_default_unchanged(lib, device):
    """health_per_image=False plans the program of before: no new opcode; and the per-image program is that program with every scan in its
    batch form, the CLEAR op in front and the JUDGE op behind -- same labels, same order, same activation memory."""
    from img2img_turbo_amd import _capi as K
    from img2img_turbo_amd.plan import ForwardPlan
    m = hc.make_model(lib, device, DTYPE, "stages")
    mk = lambda **kw: ForwardPlan(m.lib, m.weights, B, H, W, DTYPE, device, packers=m._get_packers("a2b"), **kw)
    none, whole, default, per = mk(), mk(health="stages"), mk(health="stages", health_per_image=False), mk(health="stages", health_per_image=True)
    ops = lambda p: [(o, l) for (o, _, _, l) in p.prog.ops]
    new = (K.OP_SCAN_BATCH, K.OP_SCAN_VERDICT)
    assert ops(default) == ops(whole) and all(o not in new for o, _ in ops(whole) + ops(none))
    assert [(o, l) for o, l in ops(whole) if o != K.OP_SCAN] == ops(none)
    assert whole.health_rec.shape == (len(whole.health_labels), 8) and whole.health_verdict_rows is None and not whole.health_per_image
    po = ops(per)
    assert po[0] == (K.OP_SCAN_VERDICT, "health: clear") and po[-1] == (K.OP_SCAN_VERDICT, "health: verdict")
    assert [(K.OP_SCAN if o == K.OP_SCAN_BATCH else o, l) for o, l in po[1:-1]] == ops(whole)
    assert per.prog.ops[0][2].mode == K.VERDICT_CLEAR and per.prog.ops[-1][2].mode == K.VERDICT_JUDGE
    assert per.health_labels == whole.health_labels and per.health_rec.shape == (len(per.health_labels), B, 8) and per.pool.bytes == whole.pool.bytes == none.pool.bytes
    for i, ((_, _, p, _), (t, rows, cols, ld)) in enumerate(zip([o for o in per.prog.ops if o[0] == K.OP_SCAN_BATCH], per.health_taps)):
        assert (p.images, p.rows, p.cols, p.ld, p.img_stride, p.rec_stride) == (B, rows // B, cols, ld, rows // B * ld, 64)
        assert p.rec == per._health_i64.data_ptr() + 64 * B * i and p.x == t.data_ptr()
    for p in (none, whole, default, per):
        p.release()
    m.release_plans()

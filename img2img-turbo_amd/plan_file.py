"""Plan files: save a planned forward so that a C / C++ host can run it without Python (include/i2i_turbo.h ``i2i_plan_*``,
csrc/plan_file.hip has the file layout).

    model = Pix2Pix_Turbo(weights=..., device="cuda", dtype=torch.bfloat16)
    plan = model.get_plan(8, 512, 512)
    export_plan(plan, "pix2pix_bs8_512.i2iplan")          # once, where Python and the checkpoints are

    /* C host */  i2i_plan_load(path, &p); i2i_plan_write(p, "x", ...); "ctx"; "eps"; i2i_plan_run(p, stream); i2i_plan_read(p, "out", ...);

What is saved: the op program (``plan.prog``: every launch with its tile / route decisions already taken), one buffer record per
torch storage an op pointer refers to, and a relocation table (op, pointer field) -> (buffer, offset).  Buffers of the plan's
recycling pool and its boundary buffers are *scratch* (size only, zero-filled at load); everything else -- packed weights with the LoRA
merged at the current scale, norm parameters, device scalars, ticket counters -- is saved with its contents.  The boundary buffers get
names: "x", "ctx", "eps", "noise" (stochastic plans), "out", and "canny_thr" (plans with the Canny op in front: two int32 {low, high},
saved with the values of the export, which a host overwrites with i2i_plan_write to move the thresholds), and "seed" (plans that draw
their own noise, --seed N: the 16-byte state {seed_lo, seed_hi, step, reserved} of i2i_randn_params, saved with the exported seed at step 0;
the program overwrites "eps" / "noise", which a host may read back, and advances the step after every run), and "health" / "health_names"
(plans built with health=: the n_taps x 8 uint64 records of the scans, saved zeroed and accumulated by every run, and the n_taps labels as
NUL-terminated bytes -- io names are 24 bytes, so the labels travel as data; examples/health_host.c prints them).  Per-image plans
(--seeds S0,S1,.. / --canny-per-image LOW HIGH; ForwardPlan(rng="per_image" / canny="per_image")) have "seed" as 16 * B bytes -- one state row
per image, i2i_randn_batch_params.states, examples/batch_host.c -- and "canny_thr" as 8 * B bytes, one {low, high} pair per image.
Edge plans also expose "canny_edges" (uint8 [B][H][W][3], the edge map the generator saw).  Automatic-threshold plans (--canny-auto SIGMA;
ForwardPlan(canny="auto"): the program computes "canny_thr" from the photos, i2i_canny_auto_thr_params) have "canny_sigma" (int32 [B],
sigma * 65536, saved as given; a negative entry makes that image keep the pair the host wrote to "canny_thr") and "canny_median2" (uint32
[B], the doubled medians of the last run): examples/auto_canny_host.c.
Plans with per-image health (--health-per-image with --health; ForwardPlan(health_per_image=True)) have "health" as n_taps x B x 8 uint64
(tap-major, one record per tap and image: i2i_scan_batch_params; the program zeroes them at the start of every run, so they describe the
most recent run), "health_names" unchanged, and "verdict" (16 * B bytes: one row of four uint32 {first_bad, first_over, runs, bad_runs} per
image, written by the program's last op, i2i_scan_verdict_params; totals over the runs).  Export zeroes both; examples/batch_health_host.c
prints one line per request.
Plans built with fingerprint= (--fingerprint io|stages|all; ForwardPlan(fingerprint=...)) have "fingerprint" (n_taps x B x 4 uint64, tap-major,
one i2i_digest_params record {s0, s1, elements, 0} per tap and image; the program zeroes them at the start of every run) and
"fingerprint_names" (the tap labels, NUL-terminated like "health_names"): examples/fingerprint_host.c.
Self-verifying files (--digests; export_plan(digests=True)): behind the data the file stores one i2i_digest_params record -- the buffer as
bytes, index0 = 0, computed on the exporting device -- for every buffer that is saved with contents, that no op of the forward writes and
that no io name exposes: the weights, constants and tables.  i2i_plan_verify() digests them again where they were loaded and names the first
buffer that differs.  The section is optional and trailing: a file exported without the flag is byte for byte what it always was.

This replaces the reference's ``model(...)`` call (src/pix2pix_turbo.py:186-219, src/cyclegan_turbo.py:241-254) for hosts that are not
Python; the planner itself (route queries, tile choices, buffer recycling) stays in plan.py and runs once, at export.
"""
import bisect
import ctypes as C
import struct

import torch

from . import _capi as K

MAGIC = b"I2IPLAN1"
MAGIC_LIVE = b"I2IPLAN2"      # exported with live_scale: the header also counts the scale program's ops, stored after the forward's
MAGIC_DIGESTS = b"I2IDIGS1"   # the optional trailing section of a self-verifying file (csrc/plan_file.hip has the layout)

# pointer fields an op WRITES through (everything else it only reads): a buffer the forward writes is state of a run, not a constant, and
# gets no digest
_WRITES = {K.OP_IGEMM: ("c", "c2", "ws", "gn_part"), K.OP_GN_STATS: ("partial", "ss", "counters"), K.OP_GN_APPLY: ("y",), K.OP_LAYERNORM: ("y",),
           K.OP_SOFTMAX: ("p",), K.OP_ATTENTION: ("o", "ws"), K.OP_NCHW_TO_NHWC: ("y",), K.OP_NHWC_TO_NCHW: ("y",), K.OP_POSTERIOR: ("u", "u_f32"),
           K.OP_DDPM_POSTQUANT: ("y",), K.OP_EMBED: ("y",), K.OP_LORA_MERGE: ("dst", "colsum", "bias_out"), K.OP_RESIZE_U8: ("dst",), K.OP_NOP: (),
           K.OP_CANNY_U8: ("dst", "ws"), K.OP_RANDN: ("dst", "state"), K.OP_TWIN_FOLD: ("dst", "bias"), K.OP_SCAN: ("rec",),
           K.OP_RANDN_BATCH: ("dst", "states"), K.OP_CANNY_U8_BATCH: ("dst", "ws"), K.OP_RESIZE_U8_RAGGED: ("dst", "bad_mask"),
           K.OP_SCAN_BATCH: ("rec",), K.OP_SCAN_VERDICT: ("rec", "verdict"), K.OP_CANNY_AUTO_THR: ("thr", "median2", "ws"), K.OP_DIGEST: ("rec",),
           K.OP_REPEAT: tuple("dst%d" % s for s in range(K.REPEAT_MAX_SEGMENTS)), K.OP_TILE_CUT: ("dst", "bad_mask"),
           K.OP_TILE_BLEND_U8: ("dst", "bad_mask")}


def _pointer_fields():
    """{opcode: [(byte offset inside i2i_op, field name)]} for every pointer-typed member of that opcode's parameter struct."""
    out = {}
    u_off = K.Op.u.offset
    for opcode, member in K._FIELD_OF.items():
        st = dict(K._OpUnion._fields_)[member]
        out[opcode] = [(u_off + getattr(st, name).offset, name) for name, ct in st._fields_ if ct is K.vp]
    return out


def _storage_key(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.nbytes()


def scale_program_of(plan):
    """The scale programs of the plan's packers as ONE flat per-layer program (Packer.scale_program().all_ops of the UNet's, then the VAE's):
    what a live_scale plan file stores after the forward."""
    prog = K.Program()
    for which, pk in (("unet", plan.pu), ("vae", plan.pv)):
        if pk._refolds:
            raise K.I2IError("export_plan(live_scale=True): the %s packer folds its TwinConv on the host -- construct the model with "
                             "live_scale=True, so that the fold is an op a C host can run" % which)
        sp = pk.scale_program()
        for opcode, dtype, params, label in sp.all_ops.ops:
            prog.add(opcode, dtype, params, "%s.%s" % (which, label))
        prog.keep.append(sp)
    return prog.freeze()


def export_plan(plan, path, extra_tensors=(), live_scale=False, digests=False):
    """Write ``plan`` (a ForwardPlan) to ``path``.  Returns a small summary dict.  The plan must not be replaying while this runs
    (the buffers' contents are read back through torch).

    ``live_scale=True``: the file (magic "I2IPLAN2") also carries the scale program -- every per-layer merge op and the TwinConv fold, with
    the fp32 masters, A, B and the device (r, gamma) pairs they read -- so that a C host moves the LoRA scale with i2i_plan_set_scale().
    Without it the file is an "I2IPLAN1" one whose weights stay merged at the export scale.

    The packed weights are SHARED by every plan of a model and hold whatever LoRA / skip scale ``r`` was merged last (another plan's
    ``r``, or 1.0 after a deterministic plan ran): ``plan._prepare()`` re-merges them at THIS plan's ``r`` before anything is read
    back, and refuses a plan whose buffers were released (plan-cache eviction).  A plan with health scans is exported with zeroed records:
    ``plan.health_reset()`` runs first, so read ``health_report()`` before exporting if the counts matter.

    ``digests=True``: the file ends with the digest section (see the module text) and i2i_plan_verify() works on it; on a live_scale file the
    records describe the weights as merged at the export scale."""
    plan._prepare()
    named = {"x": plan.x_in, "ctx": plan.ctx, "eps": plan.eps, "out": plan.out}
    if getattr(plan, "noise", None) is not None:
        named["noise"] = plan.noise
    # (the GroupNorm scratch -- partial sums, (scale, shift) tables, ticket counters -- is patched into the ops after they were recorded:
    # plan._finish_gn_scratch; produced inside the program, zero at rest)
    if getattr(plan, "canny", False):
        named["canny_thr"] = plan.canny_thr
        named["canny_edges"] = plan.canny_edges
    if getattr(plan, "canny_auto", False):
        named["canny_sigma"], named["canny_median2"] = plan.canny_sigma, plan.canny_median2
    if getattr(plan, "rng", False):
        named["seed"] = plan.rng_state
    if getattr(plan, "health", None):       # the records (zeroed in the file: a loaded plan starts counting at 0) and their labels, NUL-separated
        plan.health_reset()
        named["health"], named["health_names"] = plan._health_i64, plan.health_names
        if getattr(plan, "health_per_image", False):       # (health_reset zeroed the rows too)
            named["verdict"] = plan._verdict_i32
    if getattr(plan, "fingerprint_mode", None):   # the records (scratch: the program zeroes them itself) and their labels
        named["fingerprint"], named["fingerprint_names"] = plan._fp_i64, plan.fingerprint_names
    gn_scratch = [t for t in (getattr(plan, n, None) for n in ("gn_partial", "gn_ss", "gn_counters")) if t is not None]
    if getattr(plan, "canny", False):
        gn_scratch += [plan.canny_edges, plan.canny_ws] + ([plan.canny_auto_ws] if getattr(plan, "canny_auto", False) else [])
    return export_program(plan.prog, path, named, scratch=list(plan.pool.all) + gn_scratch, keep_contents=("canny_thr", "canny_sigma", "seed", "health", "health_names", "verdict", "fingerprint_names"), holders=[plan] + list(extra_tensors), device=plan.device,
                          scale_prog=scale_program_of(plan) if live_scale else None, digests=digests, lib=plan.lib)


def export_text_plan(encoder, batch, path):
    """The native CLIP text tower (text_encoder.ClipTextEncoder) for ``batch`` prompts as a plan file: "ids" (int64
    [batch * 77] token ids, padded / truncated as the reference's tokenizer call does, src/pix2pix_turbo.py:190-193) -> "ctx" ([batch * 77]
    [hidden] last hidden states in the encoder's dtype: what the generator plans take as their "ctx")."""
    from .text_encoder import _Plan
    tp = encoder._plans.get(batch)
    if tp is None:
        tp = encoder._plans[batch] = _Plan(encoder, batch)
    return export_program(tp.prog, path, {"ids": tp.ids, "ctx": tp.out}, scratch=list(tp._keep), holders=[tp, encoder.w], device=encoder.device)


def _digest_storage(t, lib):
    """The i2i_digest record of t's whole storage as bytes (index0 = 0), computed on its device, in pieces of 2^30 bytes."""
    from .digest import digest
    s = t.untyped_storage()
    flat = torch.empty(0, dtype=torch.uint8, device=t.device).set_(s, 0, (s.nbytes(),), (1,))
    tot = torch.zeros(4, dtype=torch.int64)
    for at in range(0, s.nbytes(), 1 << 30):
        tot += digest(flat[at:at + (1 << 30)], index0=at, lib=lib)[0].view(torch.int64)      # (int64 adds wrap like uint64 ones)
    return [int(v) & (2 ** 64 - 1) for v in tot.tolist()]


def export_program(prog, path, named, scratch=(), holders=(), device="cpu", keep_contents=(), scale_prog=None, digests=False, lib=None):
    """The file writer behind both: ``prog`` (a frozen _capi.Program), ``named`` boundary tensors, ``scratch`` tensors whose contents need
    not be saved (zero-filled at load, like the boundary buffers), ``holders``: objects / tensors that own anything else the ops point at,
    ``keep_contents``: names of boundary tensors that are saved WITH their contents (parameters with a meaningful default).
    ``scale_prog``: a second frozen program stored after ``prog`` (the live_scale form, see export_plan).  ``digests``: append the digest
    section, computed with ``lib`` (default: the product library)."""
    assert prog.array is not None, "the program is not frozen"
    progs = [prog] + ([scale_prog] if scale_prog is not None else [])
    all_ops = [(pg, i) for pg in progs for i in range(pg.n)]      # the concatenated op array relocations index
    named = dict(named)
    scratch_keys = {_storage_key(t) for t in list(scratch) + [t for n, t in named.items() if n not in keep_contents]}
    tensors = list(named.values()) + list(scratch)

    def harvest(obj, depth):                     # any other tensor the plan (or its packers) holds -- device scalars such as the LoRA /
        if isinstance(obj, torch.Tensor):        # skip scale r: saved with contents; only storages an op points into end up in the file
            tensors.append(obj)
        elif isinstance(obj, (list, tuple)):
            for t in obj:
                harvest(t, depth)
        elif isinstance(obj, dict):
            for t in obj.values():
                harvest(t, depth)
        elif depth > 0 and hasattr(obj, "__dict__") and type(obj).__module__.startswith(__package__):
            for t in vars(obj).values():
                harvest(t, depth - 1)
    for hld in holders:
        harvest(hld, 2)
    for _, _, params, _ in [o for pg in progs for o in pg.ops]:
        tensors += [t for t in getattr(params, "_keep", ()) if isinstance(t, torch.Tensor)]
    storages = {}                                # (ptr, nbytes) -> a tensor that owns it
    for t in tensors:
        storages.setdefault(_storage_key(t), t)
    keys = sorted(storages)                      # by address
    starts = [k[0] for k in keys]

    def locate(addr, what):
        i = bisect.bisect_right(starts, addr) - 1
        if i < 0 or addr >= keys[i][0] + max(keys[i][1], 1):
            raise K.I2IError("export_plan: %s points at 0x%x, which no tensor pinned to the program owns" % (what, addr))
        return i, addr - keys[i][0]

    # ---- relocations
    fields = _pointer_fields()
    relocs, used, volatile = [], set(), set()    # volatile: buffers the forward writes or an io name exposes (no digest)
    for oi, (pg, li) in enumerate(all_ops):
        op = pg.array[li]
        base = C.addressof(op)
        for off, fname in fields[op.opcode]:
            v = C.c_void_p.from_address(base + off).value
            if not v:
                continue
            b, o = locate(v, "op %d (%s) field %s" % (oi, pg.labels[li], fname))
            relocs.append((oi, off, b, o))
            used.add(b)
            if pg is prog and fname in _WRITES[op.opcode]:
                volatile.add(b)
    io = []
    for name, t in named.items():
        b, o = locate(t.data_ptr(), "boundary buffer " + name)
        io.append((name, b, o, t.numel() * t.element_size()))
        used.add(b)
        volatile.add(b)
    # ---- compact the buffer table to the storages that are referenced
    remap, bufs = {}, []
    for b in sorted(used):
        remap[b] = len(bufs)
        k = keys[b]
        bufs.append((k[1], 0 if k in scratch_keys else 1, storages[k]))
    if str(device) != "cpu":
        torch.cuda.synchronize()
    with open(path, "wb") as f:
        f.write((MAGIC if scale_prog is None else MAGIC_LIVE) + struct.pack("<6I", K.ABI_VERSION, C.sizeof(K.Op), prog.n, len(bufs), len(relocs), len(io)))
        if scale_prog is not None:
            f.write(struct.pack("<2I", scale_prog.n, 0))
        for nbytes, kind, _ in bufs:
            f.write(struct.pack("<QII", nbytes, kind, 0))
        for name, b, o, n in io:
            f.write(struct.pack("<24sIIQQ", name.encode(), remap[b], 0, o, n))
        for oi, off, b, o in relocs:
            f.write(struct.pack("<IIIIQ", oi, off, remap[b], 0, o))
        raw = bytearray(b"".join(C.string_at(C.addressof(pg.array), pg.n * C.sizeof(K.Op)) for pg in progs))
        for oi, off, _, _ in relocs:             # pointer fields carry no meaning in the file
            p0 = oi * C.sizeof(K.Op) + off
            raw[p0:p0 + 8] = b"\0" * 8
        f.write(bytes(raw))
        data_bytes = 0
        for nbytes, kind, t in bufs:
            if kind != 1:
                continue
            s = t.untyped_storage()
            flat = torch.empty(0, dtype=torch.uint8, device=t.device).set_(s, 0, (s.nbytes(),), (1,))
            host = flat.cpu().numpy()
            f.write(host.tobytes())
            data_bytes += nbytes
        digest_recs = []
        if digests:
            for b in sorted(used):
                nbytes, kind, t = bufs[remap[b]]
                if kind == 1 and b not in volatile:
                    s0, s1, n, _ = _digest_storage(t, lib)
                    assert n == nbytes, (n, nbytes)
                    digest_recs.append((remap[b], s0, s1, n))
            f.write(MAGIC_DIGESTS + struct.pack("<2I", len(digest_recs), 0))
            for b, s0, s1, n in digest_recs:
                f.write(struct.pack("<IIQQQ", b, 0, s0, s1, n))
    return {"digests": len(digest_recs), "digest_bytes": sum(r[3] for r in digest_recs),
            "ops": prog.n, "scale_ops": scale_prog.n if scale_prog is not None else 0, "buffers": len(bufs), "relocations": len(relocs), "data_bytes": data_bytes,
            "scratch_bytes": sum(b[0] for b in bufs if b[1] == 0), "io": {n: sz for n, _, _, sz in io}}


def main(argv=None):
    """python -m img2img_turbo_amd.plan_file --out pix2pix_bs8_512.i2iplan [--model pix2pix|cyclegan] [--batch 8 --size 512 --dtype bf16]
    [--stochastic --gamma 0.4] [--live-scale] [--direction a2b] [--u8 [--canny LOW HIGH | --canny-per-image LOW HIGH | --canny-auto SIGMA]] [--seed N | --seeds S0,S1,..] [--variations V] [--health stages|all [--health-per-image]] [--fingerprint io|stages|all] [--digests] (--base-dir <sd-turbo snapshot> --pretrained-path <lora .pkl> | --synthetic)"""
    import argparse
    ap = argparse.ArgumentParser(description="export a planned forward to a plan file for C / C++ hosts (include/i2i_turbo.h i2i_plan_*)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--model", default="pix2pix", choices=["pix2pix", "cyclegan"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, nargs="+", default=[512], help="H [W]")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--stochastic", action="store_true")
    ap.add_argument("--gamma", type=float, default=None, help="LoRA / skip scale r the weights are merged at (stochastic plans; default 0.4, "
                    "the reference's default: src/inference_paired.py:22)")
    ap.add_argument("--sketch", action="store_true", help="with --u8: 'x' holds raw uint8 sketches, binarised in the boundary kernel as the sketch "
                    "script does (F.to_tensor(img) < 0.5, src/inference_paired.py:56-58); implied by --stochastic --u8")
    ap.add_argument("--direction", default="a2b", choices=["a2b", "b2a"])
    ap.add_argument("--u8", action="store_true", help="uint8 NHWC boundary (to_tensor / Normalize / ToPILImage inside the boundary kernels)")
    ap.add_argument("--canny", type=float, nargs=2, default=None, metavar=("LOW", "HIGH"), help="with --u8 (pix2pix): 'x' holds photos; the program "
                    "starts with Canny edge detection (canny_from_pil, src/inference_paired.py:47-50).  LOW HIGH are the thresholds saved in the file; "
                    "a host moves them by writing two int32 to the buffer named 'canny_thr'")
    ap.add_argument("--seed", type=int, default=None, help="the program draws 'eps' (and 'noise') itself: seeded noise under the contract of "
                    "i2i_randn_params (include/i2i_turbo.h).  N is the seed saved in the file (step 0); a host sets another by writing four "
                    "uint32 {seed_lo, seed_hi, step, 0} to the buffer named 'seed'")
    ap.add_argument("--seeds", default=None, metavar="S0,S1,..", help="--batch comma-separated seeds: as --seed with ONE noise state per image "
                    "(i2i_randn_batch_params: image b's noise does not depend on its slot); 'seed' is then 16 bytes per image, row b = {seed_lo, "
                    "seed_hi, step, 0} of image b")
    ap.add_argument("--variations", type=int, default=1, metavar="V", help="pix2pix: V outputs per input image from one pass of the input ops and the "
                    "VAE encoder (ForwardPlan(variations=V), i2i_repeat_params): 'x' holds --batch images, 'eps' / 'noise' / 'out' and the rows of "
                    "'seed' (--seeds then takes batch * V values) batch * V, output slot b * V + v")
    ap.add_argument("--canny-per-image", type=float, nargs=2, default=None, metavar=("LOW", "HIGH"), help="as --canny with one {low, high} pair per "
                    "image: 'canny_thr' is 8 bytes per image, every row saved as LOW HIGH")
    ap.add_argument("--canny-auto", type=float, default=None, metavar="SIGMA", help="as --canny-per-image, with the thresholds computed by the program "
                    "from each photo (the median rule: low = (1 - SIGMA) * median, high = (1 + SIGMA) * median; 0.33 is customary): 'canny_sigma' "
                    "holds int32 SIGMA * 65536 per image, 'canny_thr' is written by every run")
    ap.add_argument("--health", default=None, choices=["stages", "all"], help="numerical health scans in the program (ForwardPlan(health=...)): the file "
                    "gets the buffers 'health' (8 uint64 per scanned tensor, accumulated by every run) and 'health_names' (their labels)")
    ap.add_argument("--health-per-image", action="store_true", help="with --health: one record per scanned tensor AND image ('health' holds "
                    "taps x batch x 8 uint64, zeroed by the program at the start of every run) and the buffer 'verdict' (16 bytes per image: "
                    "uint32 {first_bad, first_over, runs, bad_runs}; first_bad = 1 + the index of the first tap at which that image held a NaN / Inf)")
    ap.add_argument("--fingerprint", default=None, choices=["io", "stages", "all"], help="device fingerprints in the program (ForwardPlan(fingerprint=...)): "
                    "the file gets the buffers 'fingerprint' (4 uint64 {s0, s1, elements, 0} per tap and image, tap-major, zeroed by the program at the "
                    "start of every run) and 'fingerprint_names' (the tap labels)")
    ap.add_argument("--digests", action="store_true", help="self-verifying file: store one digest per weight / constant buffer behind the data; "
                    "i2i_plan_verify() recomputes them on the device that loaded the file")
    ap.add_argument("--live-scale", action="store_true", help="also store the scale program (per-layer merges, TwinConv fold, their fp32 masters and "
                    "LoRA factors): a host then moves the LoRA scale / skip gamma with i2i_plan_set_scale() instead of exporting one file per scale")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--base-dir", default=None, help="local stabilityai/sd-turbo snapshot directory")
    ap.add_argument("--pretrained-path", default=None, help="the reference's LoRA checkpoint (.pkl)")
    ap.add_argument("--synthetic", action="store_true", help="random-init weights of the SD-Turbo architecture (benchmarks, tests)")
    ap.add_argument("--arch", default="sd-turbo", choices=["sd-turbo", "tiny"], help="with --synthetic: the test architecture instead of SD-Turbo's")
    ap.add_argument("--lib", default=None, help="another build of the kernel library (tests: the CPU emulator)")
    a = ap.parse_args(argv)
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    if a.canny is not None and a.canny_per_image is not None:
        ap.error("--canny and --canny-per-image are exclusive")
    if a.canny_auto is not None and (a.canny is not None or a.canny_per_image is not None):
        ap.error("--canny-auto and --canny / --canny-per-image are exclusive")
    if a.canny_auto is not None and not 0.0 <= a.canny_auto <= 1.0:
        ap.error("--canny-auto takes a sigma in 0 .. 1")
    canny_mode = "auto" if a.canny_auto is not None else ("per_image" if a.canny_per_image is not None else (a.canny is not None))
    if a.canny_per_image is not None:
        a.canny = a.canny_per_image
    if a.seed is not None and a.seeds is not None:
        ap.error("--seed and --seeds are exclusive")
    if a.variations < 1:
        ap.error("--variations takes an integer >= 1")
    if a.variations > 1 and (a.model != "pix2pix" or a.health_per_image):
        ap.error("--variations is a pix2pix option, and not available with --health-per-image")
    seeds = None
    if a.seeds is not None:
        try:
            seeds = [int(s, 0) for s in a.seeds.split(",")]
        except ValueError:
            ap.error("--seeds takes comma-separated integers")
        if len(seeds) != a.batch * max(a.variations, 1):
            ap.error("--seeds holds %d values for --batch %d" % (len(seeds), a.batch) + (" x --variations %d" % a.variations if a.variations > 1 else ""))
    rng_mode = "per_image" if seeds is not None else (a.seed is not None)
    if (a.canny is not None or a.canny_auto is not None) and (not a.u8 or a.model != "pix2pix" or a.sketch or a.stochastic):
        ap.error("--canny requires --u8 on a deterministic pix2pix plan (the edge_to_image branch; not with --sketch / --stochastic)")
    H, W = a.size[0], a.size[-1]
    if a.health_per_image and not a.health:
        ap.error("--health-per-image needs --health stages|all")
    kw = dict(device=a.device, dtype=dt, live_scale=a.live_scale, health=a.health, health_per_image=a.health_per_image, fingerprint=a.fingerprint)
    if a.lib:
        kw["lib"] = K.Library(a.lib)
    if a.synthetic:
        from . import arch
        from .synth import make_cyclegan_weights, make_pix2pix_weights
        ua, va = (arch.TINY_UNET, arch.TINY_VAE) if a.arch == "tiny" else (arch.SD_TURBO_UNET, arch.SD_TURBO_VAE)
        kw["weights"] = make_cyclegan_weights(ua, va) if a.model == "cyclegan" else make_pix2pix_weights(ua, va, seed=1234, sketch=a.stochastic)
    else:
        if not (a.base_dir and a.pretrained_path):
            ap.error("give --base-dir and --pretrained-path (or --synthetic)")
        kw.update(base_dir=a.base_dir, pretrained_path=a.pretrained_path)
    if a.model == "cyclegan":
        from .cyclegan_turbo import CycleGAN_Turbo
        model = CycleGAN_Turbo(**kw)
        u8 = (2.0, -1.0) if a.u8 else None          # CycleGAN callers normalise to [-1, 1] (src/inference_unpaired.py:42-44)
        plan = model.get_plan(a.batch, H, W, direction=a.direction, u8_io=u8, rng=rng_mode)
    else:
        from .pix2pix_turbo import Pix2Pix_Turbo
        model = Pix2Pix_Turbo(**kw)
        # uint8 boundary: edge maps go through to_tensor (x / 255); the sketch model's input is the binarised sketch (threshold 128 =
        # `F.to_tensor(img) < 0.5`), which is what Pix2Pix_Turbo.forward_u8(..., sketch=True) feeds -- a stochastic plan is the sketch model
        u8 = ((1.0, 0.0, 128) if (a.sketch or a.stochastic) else (1.0, 0.0)) if a.u8 else None
        gamma = a.gamma if a.gamma is not None else (0.4 if a.stochastic else 1.0)
        plan = model.get_plan(a.batch, H, W, stochastic=a.stochastic, r=gamma, u8_io=u8, canny=canny_mode, rng=rng_mode, variations=a.variations)
        if a.canny is not None:
            plan.set_canny_thresholds(*a.canny)
        if a.canny_auto is not None:
            plan.set_canny_sigma(a.canny_auto)
    if seeds is not None:
        plan.set_seeds(seeds, 0)
    elif a.seed is not None:
        plan.set_seed(a.seed, 0)
    info = export_plan(plan, a.out, live_scale=a.live_scale, digests=a.digests)                 # (re-merges the weights at this plan's r first: plan._prepare)
    print("wrote %s: %d ops%s, %d buffers, %.2f GB of weights, %.2f GB of scratch at load; boundary buffers %s"
          % (a.out, info["ops"], " + %d scale ops" % info["scale_ops"] if a.live_scale else "", info["buffers"], info["data_bytes"] / 1e9, info["scratch_bytes"] / 1e9, info["io"]))


if __name__ == "__main__":
    main()

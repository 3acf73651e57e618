"""Pix2Pix_Turbo with the reference's API surface (src/pix2pix_turbo.py:29-229), MI355X-native inside.

``forward(c_t, prompt=None, prompt_tokens=None, deterministic=True, r=1.0, noise_map=None)`` keeps the
reference signature and semantics (:186-219).  Differences, all explicit:
  * weights come from local files / in-memory state dicts (no HTTP download, :48-64);
  * the LoRA scale / skip gamma / TwinConv blend ``r`` are per-call arguments of the planned program, so a
    stochastic call does not leave state behind (reference quirk: :206-207,217 persist);
  * a single prompt is broadcast over the batch (reference: shape error for B>1);
  * the two RNG draws (posterior eps :198, scheduler noise :200) are drawn with torch on the device in the
    same order; ``eps`` may also be injected for parity tests;
  * text conditioning: pass ``caption_enc`` ([1|B,77,1024]) or give the model a ``text_encoder`` /
    ``tokenizer`` pair (CLIP weights are not available offline).
All arithmetic runs in the HIP kernels behind include/i2i_turbo.h; there is no torch/diffusers fallback.
"""
import collections
import numbers
from typing import Optional

import torch

from . import _capi
from .model import make_1step_sched
from .plan import ForwardPlan
from .packer import Packer
from .weights import GeneratorWeights, from_pix2pix_checkpoint, load_checkpoint_file, load_sd_turbo_base


class _NetHandle:
    """What callers reach through ``model.unet`` / ``model.vae`` / ``model.vae_enc`` / ``model.vae_dec``
    (src/pix2pix_turbo.py:161, src/cyclegan_turbo.py:186-190): the canonical state dict of that network plus the no-op
    switches the reference scripts call on it (``enable_xformers_memory_efficient_attention`` src/inference_unpaired.py:36,
    ``eval`` / ``requires_grad_`` / ``to``).  The arithmetic itself lives in the planned program, not in these objects."""

    def __init__(self, name, sd, sd_b2a=None):
        self.name, self._sd, self._sd_b2a = name, sd, sd_b2a

    def state_dict(self):
        if self._sd_b2a is None:
            return dict(self._sd)
        out = {"vae." + k: v for k, v in self._sd.items()}         # VAE_encode / VAE_decode wrap both VAEs (:15-45)
        out.update({"vae_b2a." + k: v for k, v in self._sd_b2a.items()})
        return out

    def enable_xformers_memory_efficient_attention(self):
        return None            # the fused flash-style attention kernel is always on

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("training (autograd through the generator) is out of scope of the MI355X forward path")
        return self

    def requires_grad_(self, flag=False):
        return self

    def to(self, *a, **k):
        return self


class TurboGeneratorBase(torch.nn.Module):
    """Shared plumbing: plan cache (LRU, graphs released on eviction), packers (one per network and dtype; the LoRA scale r is
    re-merged on the device), boundary staging, text conditioning."""

    MAX_PLANS = 8          # distinct (batch, size, mode) programs kept alive; each owns an activation pool + a hipGraph

    def __init__(self, weights: GeneratorWeights, device="cuda", dtype=torch.float32, lib=None,
                 tokenizer=None, text_encoder=None, use_graph=True, fuse_gn=True, flash=True, plan_options=None, unet_dtype=None, live_scale=False,
                 health=None, health_limit=None, health_per_image=False, fingerprint=None):
        """``dtype``: element type of activations and packed weights (fp32 = the exact-MFMA parity mode).  ``unet_dtype``: another 16-bit
        type for the UNet alone -- ``dtype=torch.bfloat16, unet_dtype=torch.float16`` keeps the VAE (whose real activations overflow fp16)
        in bf16 and gives the UNet, whose error the 1-step scheduler multiplies by 14.6, fp16's three extra mantissa bits.
        ``live_scale=True``: ``set_lora_scale(r)`` writes the device pair (r, gamma) and runs each packer's scale program
        (Packer.scale_program: one grouped merge launch, the LayerNorm-fold layers, the TwinConv fold as a kernel) -- asynchronous on the
        stream with no host tensor math.  Off (the default), the per-layer loop and the host TwinConv fold run as before; the device fold
        rounds differently from torch's host fold, so a TwinConv checkpoint's outputs differ in the last bits between the two settings.
        ``health="stages"`` / ``"all"``: every plan carries numerical health scans (ForwardPlan(health=...), the contract of i2i_scan_params) --
        per-stage NaN / Inf / near-saturation counts accumulated on the device; read them with ``health_report()`` /
        ``health_first_bad()``, zero them with ``health_reset()``.  ``forward`` itself never synchronises for it; off (None) nothing changes.
        ``health_limit``: the near-saturation threshold (default: half the largest finite value of each scanned tensor's dtype).
        ``health_per_image=True`` (with ``health=``): one record per tap AND IMAGE and a per-image verdict computed by the program itself
        (ForwardPlan(health_per_image=True), the contracts of i2i_scan_batch_params / i2i_scan_verdict_params): ``health_verdict()`` says which
        request of the batch went non-finite and at which tap; the records then describe the most recent run alone.
        ``fingerprint="io"`` / ``"stages"`` / ``"all"``: every plan carries device fingerprints (ForwardPlan(fingerprint=...), the contract of
        i2i_digest_params) -- one 128-bit digest per tap and image of the most recent run, read with ``fingerprint()``; two runs, two GPUs or
        two hosts that computed the same bits have equal lists, and ``digest.first_diff`` names the first tap and request that differ."""
        super().__init__()
        assert fingerprint in (None, "io", "stages", "all"), fingerprint
        self.fingerprint_mode = fingerprint
        assert health in (None, "stages", "all"), health
        assert health or not health_per_image, "health_per_image needs health=\"stages\" or \"all\""
        self.health, self.health_limit, self.health_per_image = health, health_limit, bool(health_per_image)
        self._last_plan = None
        self.live_scale = bool(live_scale)
        self.unet_dtype_ = unet_dtype
        self.weights = weights
        self.device_ = torch.device(device)
        if self.device_.type == "cuda" and self.device_.index is None:
            self.device_ = torch.device("cuda", torch.cuda.current_device())
        self.dtype_ = dtype
        self.lib = lib or _capi.default_library()     # raises if the HIP build is missing: no fallback
        if self.lib.backend == "gfx950" and self.device_.type != "cuda":
            raise _capi.I2IError("the gfx950 kernel library needs a CUDA/HIP device, got %s" % device)
        self.tokenizer, self.text_encoder = tokenizer, text_encoder
        self.sched = make_1step_sched()
        self.timesteps = self.sched.timesteps
        self.use_graph = use_graph and self.lib.backend == "gfx950"
        self.fuse_gn, self.flash = fuse_gn, flash
        self.plan_options = dict(plan_options or {})   # extra ForwardPlan switches (tests / ablations): halo_min_tiles, subpix, ...
        self._plans = collections.OrderedDict()
        self._packers = {}
        self._caption_cache = {}
        self._r = 1.0
        self.unet = _NetHandle("unet", weights.unet)

    # ---- reference-compatible no-ops / switches ----
    def set_eval(self):
        return self.eval()

    def set_train(self):
        raise NotImplementedError("training (autograd through the generator) is out of scope of the MI355X forward path")

    def half(self):
        return self.to_dtype(torch.float16)

    def bfloat16(self):
        return self.to_dtype(torch.bfloat16)

    def float(self):
        return self.to_dtype(torch.float32)

    def to_dtype(self, dtype):
        if dtype != self.dtype_ or self.unet_dtype_ is not None:
            self.dtype_, self.unet_dtype_ = dtype, None
            self.release_plans()
            self._packers.clear()
        return self

    def release_plans(self):
        for plan in self._plans.values():
            plan.release()
        self._plans.clear()
        self._last_plan = None

    # ---- numerical health (of the plan that ran most recently) ----
    def _health_plan(self):
        if not self.health:
            raise _capi.I2IError("health scans are off: construct the model with health=\"stages\" or \"all\"")
        if self._last_plan is None or self._last_plan.released:
            raise _capi.I2IError("no forward has run yet (or its plan was released)")
        return self._last_plan

    def health_report(self, image=None):
        """One dict per scanned tensor of the most recently run plan, in program order (ForwardPlan.health_report; synchronises).  With
        ``health_per_image``: of image ``image``, or (the default) aggregated over the images."""
        return self._health_plan().health_report(image=image)

    def health_verdict(self):
        """``health_per_image`` models: one dict per image of the most recently run plan -- image, first_bad, first_over (tap labels or None,
        of the most recent run), runs, bad_runs (totals since the last reset); ForwardPlan.health_verdict, synchronises."""
        if not self.health_per_image:
            raise _capi.I2IError("per-image health is off: construct the model with health=... and health_per_image=True")
        return self._health_plan().health_verdict()

    def health_first_bad(self):
        """The first tensor, in program order, that held a NaN or an Inf since the last reset, or None (synchronises)."""
        return self._health_plan().health_first_bad()

    def health_reset(self):
        """Zero the records (and the per-image verdict rows) of the most recently run plan (asynchronous on the current stream)."""
        self._health_plan().health_reset()

    # ---- device fingerprints ----
    def fingerprint(self):
        """[(label, uint64 [B, 4])] of the most recently run plan, in program order (ForwardPlan.fingerprint; synchronises)."""
        if not self.fingerprint_mode:
            raise _capi.I2IError("fingerprints are off: construct the model with fingerprint=\"io\", \"stages\" or \"all\"")
        if self._last_plan is None or self._last_plan.released:
            raise _capi.I2IError("no forward has run yet (or its plan was released)")
        return self._last_plan.fingerprint()

    def weights_fingerprint(self):
        """(records, total): one (label, uint64 [4]) per packed weight buffer of every packer built so far -- the buffers the kernels read,
        with the LoRA merged at the current scale -- in packing order, and their field-wise sum mod 2^64.  Computed on the device that holds
        them (digest.digest, on the current stream: ordered behind a set_lora_scale); reads back 32 bytes per buffer."""
        from .digest import digest
        records, total = [], torch.zeros(4, dtype=torch.int64)
        with self._on_device():
            for (dt, which), pk in self._packers.items():
                for key, ent in pk.cache.items():
                    if isinstance(ent, dict) and isinstance(ent.get("w"), torch.Tensor):
                        rec = digest(ent["w"], lib=self.lib)[0]
                        records.append(("%s[%s]:%s" % (which, str(dt).replace("torch.", ""), "/".join(str(k) for k in (key if isinstance(key, tuple) else (key,)))), rec))
                        total += rec.view(torch.int64)          # (int64 adds wrap like uint64 ones)
        return records, total.view(torch.uint64)

    # ---- plumbing ----
    def _on_device(self):
        import contextlib
        return torch.cuda.device(self.device_) if self.device_.type == "cuda" else contextlib.nullcontext()

    def _packer(self, which):
        """One packer per network ('unet', 'vae', 'vae_b2a') and dtype: base weights are packed and uploaded once, the LoRA
        merge at the current r runs on the device (Packer.set_scale)."""
        dt = (self.unet_dtype_ or self.dtype_) if which == "unet" else self.dtype_
        key = (dt, which)
        if key not in self._packers:
            w = self.weights
            sd, sc = {"unet": (w.unet, w.unet_scaling), "vae": (w.vae, w.vae_scaling), "vae_b2a": (w.vae_b2a, w.vae_scaling)}[which]
            with self._on_device():
                self._packers[key] = Packer(sd, sc, dt, self.device_, self.lib, self._r, self._r, live_scale=self.live_scale)
        return self._packers[key]

    def _get_packers(self, direction):
        vae = "vae" if (direction == "a2b" or self.weights.vae_b2a is None) else "vae_b2a"
        return self._packer("unet"), self._packer(vae)

    def set_lora_scale(self, r: float):
        """The reference's per-call ``unet.set_adapters(["default"], weights=[r])`` +
        ``set_weights_and_activate_adapters(vae, ["vae_skip"], [r])`` + ``decoder.gamma = r`` + ``conv_in.r = r``
        (src/pix2pix_turbo.py:206-217) as ONE device-side re-merge of the packed weights (csrc/lora_merge.hip): no re-pack,
        no re-upload, plans and captured graphs stay valid.  Asynchronous on the current stream."""
        r = float(r)
        if r != self._r:
            self._r = r
            with self._on_device():
                for pk in self._packers.values():
                    pk.set_scale(r, r)

    def get_plan(self, B, H, W, stochastic=False, r=1.0, direction="a2b", ctx_batch=1, u8_io=None, canny=False, rng=False, _variations=1) -> ForwardPlan:
        """The cached plan for this shape.  `r` is not part of the key (device addresses do not depend on it): ONE plan object
        per key, which records the r of the most recent get_plan() for that key and re-applies it whenever it runs
        (ForwardPlan.before_run).  Plans of DIFFERENT keys (a stochastic and a deterministic one, two sizes) can be held and
        interleaved safely; two r values for the SAME key are the same object -- the last get_plan() wins, so ask again
        (it is a dictionary lookup) before running with another r.  ``canny=True`` (uint8 boundary only): the program starts with Canny
        edge detection of "x"; only the boolean is part of the key -- the thresholds are device state of the plan
        (ForwardPlan.set_canny_thresholds), so every (low, high) shares one plan and one captured graph.  ``rng=True``: the program draws
        "eps" (and "noise") itself from the plan's device state (ForwardPlan.set_seed; the contract of i2i_randn_params) and advances the step
        after every run; again only the boolean is part of the key, every seed shares the plan.  ``rng="per_image"`` / ``canny="per_image"``:
        one noise state / one threshold pair per image of the batch (ForwardPlan.set_seeds, set_canny_thresholds with sequences; the
        contracts of i2i_randn_batch_params / i2i_canny_u8_batch_params).  ``canny="auto"``: the per-image form whose thresholds the program
        computes from the photos (ForwardPlan.set_canny_sigma; the contract of i2i_canny_auto_thr_params).  The mode is part of the key, so
        the plans of scalar callers stay theirs."""
        r_plan = float(r) if stochastic else 1.0
        self.set_lora_scale(r_plan)
        key = ((B, H, W, self.dtype_, self.unet_dtype_, stochastic, direction, ctx_batch, u8_io)
               + ((("canny_per_image",) if canny == "per_image" else (("canny_auto",) if canny == "auto" else (True,))) if canny else ())
               + ((("rng_per_image",) if rng == "per_image" else ("rng",)) if rng else ())
               + (("health", self.health, self.health_limit) if self.health else ()) + (("health_per_image",) if self.health_per_image else ())
               + (("fingerprint", self.fingerprint_mode) if self.fingerprint_mode else ())
               + (("variations", int(_variations)) if int(_variations) != 1 else ()))      # (1 = the key, and the plan, of a call without it)
        if int(_variations) > 1 and self.health_per_image:
            raise ValueError("variations=%d on a model with health_per_image=True: per-image health of a variations plan is not supported "
                             "(use whole-batch health)" % int(_variations))
        if key in self._plans:
            self._plans.move_to_end(key)
        else:
            opts = dict(self.plan_options)
            if u8_io is not None:
                opts["u8_io"] = u8_io
            if canny:
                opts["canny"] = canny if canny in ("per_image", "auto") else True
            if rng:
                opts["rng"] = rng if rng == "per_image" else True
            if self.health:
                opts["health"], opts["health_limit"] = self.health, self.health_limit
                if self.health_per_image:
                    opts["health_per_image"] = True
            if self.fingerprint_mode:
                opts["fingerprint"] = self.fingerprint_mode
            if int(_variations) != 1:
                opts["variations"] = int(_variations)
            with self._on_device():
                self._plans[key] = ForwardPlan(self.lib, self.weights, B, H, W, self.dtype_, self.device_, stochastic=stochastic,
                                               r=self._r, direction=direction, ctx_batch=ctx_batch, fuse_gn=self.fuse_gn,
                                               flash=self.flash, packers=self._get_packers(direction), unet_dtype=self.unet_dtype_, **opts)
            while len(self._plans) > self.MAX_PLANS:      # LRU: the evicted plan's graph and activation pool are released
                _, old = self._plans.popitem(last=False)
                old.release()
        plan = self._plans[key]
        plan.r = r_plan
        plan.before_run = self._apply_plan_r
        return plan

    def _apply_plan_r(self, plan):
        self.set_lora_scale(plan.r)

    def encode_prompt(self, prompt=None, prompt_tokens=None):
        """tokenizer(prompt, max_length=77, padding="max_length", truncation=True) -> text_encoder(ids)[0]
        (src/pix2pix_turbo.py:190-196).  Cached per prompt string."""
        if self.text_encoder is None:
            raise _capi.I2IError("no text encoder attached: pass caption_enc=[1|B,77,%d] or construct the model with "
                                 "tokenizer= and text_encoder=" % self.weights.unet_arch.cross_attention_dim)
        if prompt is not None:
            key = prompt if isinstance(prompt, str) else tuple(prompt)
            if key not in self._caption_cache:
                ids = self.tokenizer(prompt, max_length=self.tokenizer.model_max_length, padding="max_length",
                                     truncation=True, return_tensors="pt").input_ids
                self._caption_cache[key] = self.text_encoder(ids.to(self.device_))[0].detach()
            return self._caption_cache[key]
        ids = prompt_tokens.reshape(-1, prompt_tokens.shape[-1])   # [B,1,77] from the training dataset (A.5)
        return self.text_encoder(ids.to(self.device_))[0].detach()

    def stage(self, plan: ForwardPlan, x, caption_enc, eps, noise_map=None):
        """Copy one batch into the plan's static boundary buffers (device-to-device when the inputs are already resident).  ``eps=None``:
        the plan draws its own noise (rng plans)."""
        plan.x_in.copy_(x)
        V = getattr(plan, "V", 1)
        if V > 1 and plan.ctx_batch > 1 and caption_enc.numel() * V == plan.ctx.numel():      # one caption per INPUT image: image-major rows
            caption_enc = caption_enc.reshape((plan.B,) + tuple(plan.ctx.shape[1:])).to(plan.ctx.device).repeat_interleave(V, 0)
        plan.ctx.copy_(caption_enc.reshape(plan.ctx.shape))
        if eps is not None:
            plan.eps.copy_(eps)
        if noise_map is not None:
            plan.noise.copy_(noise_map.expand_as(plan.noise))

    def _execute(self, plan: ForwardPlan, x, caption_enc, eps, noise_map=None, canny=None, seed=None):
        with self._on_device():
            self.stage(plan, x, caption_enc, eps, noise_map)
            if isinstance(seed, list):
                plan.set_seeds(seed, 0)
            elif seed is not None:
                plan.set_seed(seed, 0)
            if canny is not None and canny[0] == "auto":
                _, sigmas, lows, highs = canny
                plan.set_canny_sigma(sigmas)
                if any(v is not None for v in lows):
                    plan.set_canny_thresholds(lows, highs)
            elif canny is not None:
                plan.set_canny_thresholds(*canny)
            if self.use_graph:
                plan.replay()
            else:
                plan.run()
            self._last_plan = plan
            return plan.out.clone()

    # ---- tiled forward at native resolution (include/i2i_turbo.h, the note above i2i_tile_request; DESIGN.md "Tiled forward") ----
    def _tile_refusals(self, tile, tile_batch, *, eps=None, noise_map=None, variations=1, resize_back=False):
        """The argument combinations a tiled forward_u8 refuses (ValueError with the reason)."""
        if not (isinstance(tile, (tuple, list)) and len(tile) == 2 and all(isinstance(v, numbers.Integral) for v in tile)):
            raise ValueError("tile=%r (a pair (tile width, tile height) of multiples of 8)" % (tile,))
        if int(tile_batch) < 1:
            raise ValueError("tile_batch=%r (an integer >= 1)" % (tile_batch,))
        if eps is not None or noise_map is not None:
            raise ValueError("tile= draws one noise field per request and crops it per tile (seed= or torch.randn): do not pass eps= / noise_map= with it")
        if int(variations) > 1:
            raise ValueError("tile= together with variations=%d is not supported" % int(variations))
        if resize_back:
            raise ValueError("tile= keeps the request's size: resize_back=True has nothing to undo")
        if self.health_per_image:
            raise ValueError("tile= on a model with health_per_image=True: the images of a tile batch are tiles, not requests")
        if self.fingerprint_mode:
            raise ValueError("tile= on a model with fingerprint=%r: the images of a tile batch are tiles, not requests" % (self.fingerprint_mode,))

    def _forward_tiles(self, items, stacked, chunk_forward, *, tile, tile_overlap, tile_batch, seed, stochastic, caption_enc):
        """Cut -> the ordinary forward over the tile batch in chunks of ``tile_batch`` -> blend.  ``items``: the requests AFTER the input ops
        (uint8 [H_b, W_b, 3] each); ``chunk_forward(tiles, caption, eps, noise)`` runs one chunk and returns its uint8 outputs.  Noise: every
        request draws ONE field [lat][ceil(H / 8)][ceil(W / 8)] at (its seed, step 0, stream 0) -- and, stochastic, a second one at stream 2
        -- and a tile gets the crop at its latent origin (image_ops.tile_cut_planes), so a request's noise depends on neither its slot nor
        the chunking; without a seed the fields come from torch.randn.  Returns (images, layout)."""
        from . import image_ops, rng
        B = len(items)
        layout = image_ops.tile_layout([t.shape[:2] for t in items], tile, tile_overlap)      # ValueError: the layout rule's refusals
        seed = seed_argument(seed, B)
        lat = self.weights.vae_arch.latent_channels
        with self._on_device():
            tiles, layout = image_ops.tile_cut_u8(items, tile, tile_overlap, self.lib)
            crops = []
            for stream in ((rng.STREAM_EPS, rng.STREAM_NOISE) if stochastic else (rng.STREAM_EPS,)):
                fields = []
                for b, (h, w) in enumerate(layout.sizes):
                    shape = (lat, -(-h // 8), -(-w // 8))
                    if seed is None:
                        fields.append(torch.randn(shape, device=self.device_, dtype=torch.float32))
                    else:
                        fields.append(rng.randn(shape, seed[b] if isinstance(seed, list) else seed, 0, stream, device=self.device_, lib=self.lib))
                crops.append(image_ops.tile_cut_planes(fields, layout, self.lib))
            per_tile = None
            if caption_enc.dim() == 3 and caption_enc.shape[0] == B and B > 1:               # one caption per request: expanded per tile
                per_tile = caption_enc.to(self.device_)[torch.tensor(layout.request_of_tile, device=self.device_)]
            outs = []
            for k in range(0, layout.T, int(tile_batch)):
                sl = slice(k, min(k + int(tile_batch), layout.T))
                outs.append(chunk_forward(tiles[sl], caption_enc if per_tile is None else per_tile[sl], crops[0][sl], crops[1][sl] if stochastic else None))
            return image_ops.tile_blend_u8(torch.cat(outs) if len(outs) > 1 else outs[0], layout, self.lib, stack=stacked), layout


def _bind(names, args, kw):
    """forward's positional arguments by name, merged with its keywords."""
    if len(args) > len(names):
        raise TypeError("forward_u8: %d positional arguments behind the images (at most %d: %s)" % (len(args), len(names), ", ".join(names)))
    bound = dict(zip(names, args))
    for k in kw:
        if k in bound:
            raise TypeError("forward_u8: %s given twice" % k)
    bound.update(kw)
    return bound


def seed_argument(seed, B, V=1):
    """``seed=`` of the forwards: None, one int (one noise state for the batch), or a sequence of B ints (one per image) -> None | int | list.
    With ``variations=V`` the sequence is nested [B][V] or flat with B * V entries; the list returned is flat, in output order (b * V + v)."""
    if seed is None or isinstance(seed, numbers.Integral):
        return seed
    seed = list(seed)
    if V > 1 and len(seed) == B and all(isinstance(s, (list, tuple)) for s in seed):
        if any(len(s) != V for s in seed):
            raise ValueError("seed= holds %s seeds per image for variations=%d" % ([len(s) for s in seed], V))
        seed = [v for s in seed for v in s]
    seed = [int(s) for s in seed]
    if len(seed) != B * V:
        raise ValueError("seed= holds %d seeds for a batch of %d (one int, or one per image)" % (len(seed), B * V)
                         + (" = %d images x %d variations (nested [B][V], or flat in output order)" % (B, V) if V > 1 else ""))
    return seed


def per_image_mode(canny):
    """get_plan's canny mode of forward_u8's normalised ``canny``: None -> False, (low, high) -> True, (lows, highs) -> "per_image",
    ("auto", sigmas, lows, highs) -> "auto"."""
    if canny is None:
        return False
    if canny[0] == "auto":
        return "auto"
    return "per_image" if isinstance(canny[0], list) else True


def _is_auto(entry):
    """"auto" or ("auto", sigma): one automatic request of forward_u8's ``canny=``."""
    return entry == "auto" if isinstance(entry, str) else (isinstance(entry, (tuple, list)) and len(entry) == 2 and entry[0] == "auto"
                                                            and isinstance(entry[1], (int, float)))


def canny_argument(canny, B, default_sigma=0.33):
    """forward_u8's ``canny=`` in the form _execute takes: None | (low, high) | (lows, highs) | ("auto", sigmas, lows, highs) -- the last
    with B entries each, sigmas[b] None for a request with its own sliders and lows[b] / highs[b] None for an automatic one."""
    if canny is None or canny is False:
        return None
    if canny is True:
        return (100, 200)
    if _is_auto(canny):
        sigma = default_sigma if isinstance(canny, str) else float(canny[1])
        return ("auto", [sigma] * B, [None] * B, [None] * B)
    if isinstance(canny, str):
        raise ValueError("canny=%r (True, (low, high), \"auto\", (\"auto\", sigma) or a list of B such entries)" % (canny,))
    if isinstance(canny[0], (int, float)):
        return (canny[0], canny[1])
    if len(canny) != B:                                                      # a sequence of B entries
        raise ValueError("canny= holds %d entries for a batch of %d" % (len(canny), B))
    if not any(_is_auto(e) for e in canny):
        return ([p[0] for p in canny], [p[1] for p in canny])
    sigmas = [(default_sigma if isinstance(e, str) else float(e[1])) if _is_auto(e) else None for e in canny]
    return ("auto", sigmas, [None if _is_auto(e) else e[0] for e in canny], [None if _is_auto(e) else e[1] for e in canny])


class Pix2Pix_Turbo(TurboGeneratorBase):
    def __init__(self, pretrained_name=None, pretrained_path=None, ckpt_folder="checkpoints", lora_rank_unet=8, lora_rank_vae=4,
                 *, weights: Optional[GeneratorWeights] = None, base_dir=None, **kw):
        if weights is None:
            # local-file counterpart of src/pix2pix_turbo.py:47-130: base SD-Turbo snapshot + LoRA .pkl
            import os
            base_dir = base_dir or os.environ.get("I2I_SD_TURBO_DIR")      # so Pix2Pix_Turbo(pretrained_name=...) works as written
            if base_dir is None:                                            # in src/inference_paired.py:31
                raise ValueError("give weights=GeneratorWeights(...), base_dir=<local sd-turbo snapshot> or set I2I_SD_TURBO_DIR "
                                 "(the reference downloads stabilityai/sd-turbo from the hub; there is no network here)")
            names = {"edge_to_image": "edge_to_image_loras.pkl", "sketch_to_image_stochastic": "sketch_to_image_stochastic_lora.pkl"}
            if pretrained_name in names:
                pretrained_path = os.path.join(ckpt_folder, names[pretrained_name])
            if pretrained_path is None:
                raise ValueError("pretrained_name or pretrained_path required (random-init training models are out of scope)")
            unet, vae = load_sd_turbo_base(base_dir)
            weights = from_pix2pix_checkpoint(unet, vae, load_checkpoint_file(pretrained_path))
        super().__init__(weights, **kw)
        self.lora_rank_unet, self.lora_rank_vae = lora_rank_unet, lora_rank_vae
        self.vae = _NetHandle("vae", weights.vae)
        self.target_modules_unet = weights.meta.get("unet_lora_target_modules")
        self.target_modules_vae = weights.meta.get("vae_lora_target_modules")
        if weights.meta.get("rank_unet"):
            self.lora_rank_unet, self.lora_rank_vae = weights.meta["rank_unet"], weights.meta["rank_vae"]

    def get_plan(self, B, H, W, *args, variations=1, **kw) -> ForwardPlan:
        """TurboGeneratorBase.get_plan with ``variations=V`` (part of the LRU key; 1 = the key and the plan of a call without it): V outputs per
        input image from one pass of the input ops and the VAE encoder (ForwardPlan(variations=V)) -- "x" holds B images, "eps" / "noise" /
        the seed rows / "out" B * V, output slot b * V + v."""
        if int(variations) < 1:
            raise ValueError("variations=%r (an integer >= 1)" % (variations,))
        return super().get_plan(B, H, W, *args, _variations=int(variations), **kw)

    @torch.no_grad()
    def forward_u8(self, images_u8, *args, resize=None, sketch=False, canny=None, return_edges=False, resample="lanczos",
                   tile=None, tile_overlap=64, tile_batch=8, jpeg=None, png=None, **kw):
        """uint8 HWC in, uint8 HWC out ([B, H, W, 3] on the device): the callers' ``F.to_tensor`` (src/inference_paired.py:50)
        and ``ToPILImage()(out*0.5+0.5)`` (:72) run inside the boundary kernels; everything else as ``forward``.
        ``resize="multiple_of_8"`` first applies the script's ``input_image.resize((w - w % 8, h - h % 8), Image.LANCZOS)``
        (:38-41) on the device, bit-identical to Pillow (image_ops.lanczos_resize_u8); ``resize=(width, height)`` any size.
        ``sketch=True``: the sketch branch's binarisation ``F.to_tensor(input_image) < 0.5`` (:57-58) instead of ``to_tensor``
        (bytes below 128 become 1.0, the others 0.0), as the stochastic sketch model expects.
        ``canny=(low, high)`` or ``canny=True`` (100, 200): the edge_to_image branch, ``canny_from_pil(input_image, low, high)`` (:47-50 =
        cv2.Canny replicated to 3 channels, src/image_prep.py:6-12), after the optional resize and in front of ``to_tensor`` -- the first op
        of the planned program (csrc/resize.hip), so photo -> resize -> Canny -> generator -> uint8 image is one asynchronous sequence.
        Every (low, high) runs the same plan / captured graph (the thresholds are device state).  OpenCV parity is unpinned where cv2 is
        absent: tests/canny_ref.py is the oracle of the contract in include/i2i_turbo.h.  ``canny=[(low, high)] * B``: one pair per image (the
        requests of a batch keep their own sliders; image b is what a call on image b alone gives, i2i_canny_u8_batch_params).
        ``canny="auto"`` / ``canny=("auto", sigma)``: the thresholds are computed on the device from each photo by the median rule, low =
        (1 - sigma) * median, high = (1 + sigma) * median in the integer form of i2i_canny_auto_thr_params (include/i2i_turbo.h) -- the first
        op of the program, in front of Canny.  The rule is NOT part of the reference; sigma = 0.33 is its customary default, not a tuned one.
        Per image, ``canny=[(100, 200), "auto", ("auto", 0.25), ..]`` mixes requests with their own sliders and automatic ones on one plan.
        ``return_edges=True`` (with ``canny``): returns ``(out, edges)``, edges a uint8 [B, H, W, 3] clone of the edge map the generator saw
        (255 on edges; the reference saves and shows ``255 - edges``, src/inference_paired.py:48-49) -- and on an automatic plan ``(out,
        edges, thr)``, thr int32 [B, 2] the {low, high} pairs that were used.
        ``resample="bicubic"``: the resize uses Pillow's BICUBIC tables, bit-identical to ``Image.resize(size)`` with no filter argument
        (gradio_canny2image.py:16); the default is the scripts' LANCZOS.
        ``seed=`` / ``variations=``: as in ``forward``; with ``canny=`` the edges are computed once per input and ``return_edges=True`` returns
        the B maps (not B * V).
        ``images_u8`` may also be a LIST of uint8 [H_b, W_b, 3] tensors of different sizes with ``resize=(width, height)``: the requests of a
        batch are brought to the model size in two launches (image_ops.lanczos_resize_u8_ragged) and image b of the result is what the
        stacked, pre-resized batch gives.  A list needs an explicit size: ``resize=None`` / ``"multiple_of_8"`` would leave the images at
        different sizes in front of the generator (ValueError).
        ``tile=(tile width, tile height)`` (multiples of 8; NOT part of the reference): a request larger than the model size keeps its size --
        it is cut into tiles that overlap by ``tile_overlap`` pixels (a multiple of 8, at most half the tile; the layout rule is stated at
        i2i_tile_request, include/i2i_turbo.h), the tiles run through the ordinary forward in chunks of ``tile_batch`` and the outputs are
        blended back with an integer feather, cut and blend each one launch on the device.  ``images_u8`` may be a tensor or a list of
        requests of different sizes (the result is then a list); ``resize=`` applies first.  ``canny=`` runs over the WHOLE request before
        the cut (hysteresis is not local; ``return_edges=True`` returns ``(out, edges)`` with the requests' shapes), ``sketch=True`` as
        without tiles.  Noise: with ``seed=`` (one int or one per request) every request draws one field [lat][ceil(H / 8)][ceil(W / 8)] at
        (seed, step 0) and a tile's eps (and noise map) is the crop at its latent origin, so overlapping tiles see the same noise and a
        request's noise depends on neither its slot nor the chunking; without ``seed=`` the fields come from torch.randn.  ValueError:
        ``eps=`` / ``noise_map=``, ``variations`` > 1, per-image health or fingerprints, a request smaller than the tile, a tile that is no
        multiple of 8, a bad ``tile_overlap``.  Picture quality of tiled output on trained weights is unassessed.
        ``jpeg=True`` / a quality / ``(quality, "4:4:4" | "4:2:0")`` / a list of one such entry per input image: the script's
        ``output_pil.save(...)`` (src/inference_paired.py:75) on the device -- the images come back as a list of ``bytes``, each the complete
        baseline JPEG file Pillow writes for that image at that quality and subsampling, byte for byte (image_ops.jpeg_encode_u8; ``True`` is
        Pillow's default, quality 75 at 4:2:0), in the order the tensor would have had (``variations=V``: image-major, B * V files; ``tile=``
        or a list: every request at its own size, one ragged call).  ``return_edges=True`` keeps returning the edges beside them.
        ``png=True``: the same line when the name ends in .png, what the scripts' ``bname`` usually asks for -- a list of ``bytes``, each a
        PNG file with Pillow's container and filtered scanlines and this project's deflate stream (image_ops.png_encode_u8; lossless: the
        files decode to the uint8 output); composes as ``jpeg=`` does; ``png=`` beside ``jpeg=`` is a ValueError.  ``return_edges="png"``
        (with ``canny=``): the second result is the list of PNG files of ``255 - edges``, the script's ``_canny.png`` (:48-49)."""
        if png is not None or (isinstance(return_edges, str) and return_edges == "png"):
            from . import image_ops
            want = image_ops.png_argument(png, jpeg)
            edges_png = isinstance(return_edges, str)
            res = self.forward_u8(images_u8, *args, resize=resize, sketch=sketch, canny=canny, return_edges=bool(return_edges), resample=resample,
                                  tile=tile, tile_overlap=tile_overlap, tile_batch=tile_batch, jpeg=jpeg, **kw)
            if not want and not edges_png:
                return res
            with self._on_device():
                return image_ops.png_files(res, self.lib, images=want, edges=edges_png)
        if jpeg is not None:
            from . import image_ops
            n = images_u8.shape[0] if torch.is_tensor(images_u8) else len(images_u8)
            spec = image_ops.jpeg_argument(jpeg, n, int(kw.get("variations", 1)))
            res = self.forward_u8(images_u8, *args, resize=resize, sketch=sketch, canny=canny, return_edges=return_edges, resample=resample, tile=tile,
                                  tile_overlap=tile_overlap, tile_batch=tile_batch, **kw)
            with self._on_device():
                return image_ops.jpeg_files(res, spec, self.lib)
        if tile is not None:
            return self._forward_u8_tiled(images_u8, _bind(("prompt", "prompt_tokens", "deterministic", "r", "noise_map"), args, kw), resize=resize,
                                          sketch=sketch, canny=canny, return_edges=return_edges, resample=resample, tile=tile,
                                          tile_overlap=tile_overlap, tile_batch=tile_batch)
        if isinstance(images_u8, (list, tuple)):
            if resize is None or isinstance(resize, str):
                raise ValueError("a list of images of different sizes needs resize=(width, height): resize=%r leaves them at different sizes" % (resize,))
            from .image_ops import lanczos_resize_u8_ragged
            with self._on_device():
                images_u8 = lanczos_resize_u8_ragged(list(images_u8), (int(resize[0]), int(resize[1])), self.lib, resample=resample)
            resize = None
        assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3
        canny = canny_argument(canny, images_u8.shape[0])
        if canny is not None and sketch:
            raise ValueError("canny and sketch=True are the two exclusive branches of the script (src/inference_paired.py:47-58)")
        if return_edges and canny is None:
            raise ValueError("return_edges=True needs canny=: without it the input IS the edge map")
        if resize is not None:
            from .image_ops import lanczos_resize_u8, resize_to_multiple_of_8
            with self._on_device():
                images_u8 = (resize_to_multiple_of_8(images_u8, self.lib, resample=resample) if resize == "multiple_of_8"
                             else lanczos_resize_u8(images_u8, resize, self.lib, resample=resample))
        out = self.forward(images_u8, *args, _u8_io=(1.0, 0.0, 128) if sketch else (1.0, 0.0), _canny=canny, **kw)
        if not return_edges:
            return out
        plan = self._last_plan                   # (the plan that just ran; same stream, so the clones see this run's edge map)
        with self._on_device():
            return (out, plan.canny_edges.clone()) + ((plan.canny_thr.clone(),) if plan.canny_auto else ())

    def _forward_u8_tiled(self, images, opts, *, resize, sketch, canny, return_edges, resample, tile, tile_overlap, tile_batch):
        """forward_u8 with ``tile=`` (see there): input ops over the whole request, cut, forward over the tile batch, blend."""
        from . import image_ops
        unknown = set(opts) - {"prompt", "prompt_tokens", "deterministic", "r", "noise_map", "caption_enc", "eps", "seed", "variations"}
        if unknown:
            raise TypeError("forward_u8: unexpected arguments %s" % sorted(unknown))
        self._tile_refusals(tile, tile_batch, eps=opts.get("eps"), noise_map=opts.get("noise_map"), variations=opts.get("variations", 1))
        stacked = torch.is_tensor(images)
        with self._on_device():
            if resize is not None and not stacked:
                if isinstance(resize, str):
                    raise ValueError("a list of images of different sizes takes resize=(width, height), not %r" % (resize,))
                images, stacked = image_ops.lanczos_resize_u8_ragged(list(images), (int(resize[0]), int(resize[1])), self.lib, resample=resample), True
            elif resize is not None:
                images = (image_ops.resize_to_multiple_of_8(images, self.lib, resample=resample) if resize == "multiple_of_8"
                          else image_ops.lanczos_resize_u8(images, resize, self.lib, resample=resample))
        items = list(images.unbind(0)) if stacked else list(images)
        if not items or any(not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3 for t in items):
            raise ValueError("forward_u8(tile=...): uint8 [B, H, W, 3], or a list of uint8 [H, W, 3] requests")
        image_ops.tile_layout([t.shape[:2] for t in items], tile, tile_overlap)        # the layout rule's refusals, before any device work
        canny = canny_argument(canny, len(items))
        if canny is not None and sketch:
            raise ValueError("canny and sketch=True are the two exclusive branches of the script (src/inference_paired.py:47-58)")
        if return_edges and canny is None:
            raise ValueError("return_edges=True needs canny=: without it the input IS the edge map")
        deterministic = bool(opts.get("deterministic", True))
        caption_enc = opts.get("caption_enc")
        if caption_enc is None:
            assert (opts.get("prompt") is None) != (opts.get("prompt_tokens") is None), "Either prompt or prompt_tokens should be provided"
            caption_enc = self.encode_prompt(opts.get("prompt"), opts.get("prompt_tokens"))
        edges = None
        if canny is not None:                    # Canny over the WHOLE request: hysteresis follows edges across tile borders
            with self._on_device():
                edges = []
                for b, t in enumerate(items):
                    if canny[0] == "auto" and canny[1][b] is not None:
                        edges.append(image_ops.canny_u8(t[None], "auto", out_channels=3, lib=self.lib, sigma=canny[1][b])[0])
                    else:
                        lows, highs = canny[-2:]
                        lo, hi = (lows[b], highs[b]) if isinstance(lows, list) else (lows, highs)
                        edges.append(image_ops.canny_u8(t[None], lo, hi, out_channels=3, lib=self.lib)[0])
            items = edges
        u8_io = (1.0, 0.0, 128) if sketch else (1.0, 0.0)

        def chunk(tiles, cap, eps, noise):
            return self.forward(tiles, deterministic=deterministic, r=opts.get("r", 1.0), noise_map=noise, caption_enc=cap, eps=eps, _u8_io=u8_io)

        out, _ = self._forward_tiles(items, stacked, chunk, tile=tile, tile_overlap=tile_overlap, tile_batch=tile_batch, seed=opts.get("seed"),
                                     stochastic=not deterministic, caption_enc=caption_enc)
        if not return_edges:
            return out
        return out, (torch.stack(edges) if stacked else edges)

    @torch.no_grad()
    def forward(self, c_t, prompt=None, prompt_tokens=None, deterministic=True, r=1.0, noise_map=None,
                *, caption_enc=None, eps=None, seed=None, variations=1, _u8_io=None, _canny=None):
        """``seed=s``: the scripts' ``torch.manual_seed(s)`` + ``torch.randn`` (src/inference_paired.py:58-60) on the device -- the planned
        program draws "eps" (and, stochastic, the noise map) itself at (seed s, step 0) under the contract of i2i_randn_params
        (include/i2i_turbo.h; img2img_turbo_amd.rng): nothing is staged by the host, the same seed gives the same image on every call, and
        ``noise_map`` is not needed.  Not together with ``eps=`` / ``noise_map=``.  ``seed=None``: as before.
        ``seed=[s0, .., sB-1]``: one seed per image, every image at step 0 (the contract of i2i_randn_batch_params): image b's noise is what
        a batch-1 call with ``seed=sb`` draws, whatever its slot -- the noise, not necessarily every bit of the image (the kernels choose
        their routes by batch size).
        ``variations=V``: V outputs per input image -- the seed gallery of gradio_sketch2image.py ("try different seeds to generate
        different results") in one call.  Returns B * V images, image-major (slot b * V + v); the input ops and the VAE encoder run once per
        INPUT (nothing in front of the posterior sample depends on the seed).  ``seed``: one int, a nested [B][V] list or a flat list of
        B * V; explicit ``eps`` / ``noise_map`` have leading dimension B * V; ``caption_enc`` [1 | B | B * V, 77, D]."""
        V = int(variations)
        if V < 1:
            raise ValueError("variations=%r (an integer >= 1)" % (variations,))
        if seed is not None and (eps is not None or noise_map is not None):
            raise ValueError("seed= draws eps and the noise map on the device: do not pass eps= / noise_map= with it")
        seed = seed_argument(seed, c_t.shape[0], V)
        if caption_enc is None:
            # either the prompt or the prompt_tokens should be provided (src/pix2pix_turbo.py:188)
            assert (prompt is None) != (prompt_tokens is None), "Either prompt or prompt_tokens should be provided"
            caption_enc = self.encode_prompt(prompt, prompt_tokens)
        if _u8_io is not None:
            B, H, W, _ = c_t.shape
        else:
            B, _, H, W = c_t.shape
        if not deterministic:
            if noise_map is None and seed is None:
                raise ValueError("stochastic forward needs noise_map (src/pix2pix_turbo.py:210) or seed=")
        elif self.weights.is_twin_conv:
            raise ValueError("this checkpoint wraps conv_in in a TwinConv, which the reference can only run with "
                             "deterministic=False (TwinConv.r is None otherwise, src/pix2pix_turbo.py:21-26)")
        lat = self.weights.vae_arch.latent_channels
        if eps is None and seed is None:   # latent_dist.sample() draw, then the (numerically dead) scheduler draw: same order as the reference
            eps = torch.randn(B * V, lat, H // 8, W // 8, device=self.device_, dtype=torch.float32)
            torch.randn(B * V, lat, H // 8, W // 8, device=self.device_, dtype=torch.float32)
        ctx_batch = caption_enc.shape[0] if caption_enc.dim() == 3 else 1
        assert ctx_batch in (1, B, B * V)
        if V > 1:
            for name, t in (("eps", eps), ("noise_map", noise_map)):
                if t is not None and t.shape[0] != B * V:
                    raise ValueError("%s holds %d images for %d images x %d variations (leading dimension B * V)" % (name, t.shape[0], B, V))
        plan = self.get_plan(B, H, W, stochastic=not deterministic, r=r, ctx_batch=ctx_batch, u8_io=_u8_io, canny=per_image_mode(_canny),
                             rng=("per_image" if isinstance(seed, list) else seed is not None), variations=V)
        out = self._execute(plan, c_t, caption_enc, eps, None if deterministic else noise_map, canny=_canny, seed=seed)
        if _u8_io is not None:
            return out
        return out.to(c_t.dtype) if c_t.dtype in (torch.float16, torch.bfloat16, torch.float32) else out

    def save_model(self, outf):
        """Same dict layout as the reference (src/pix2pix_turbo.py:221-229): keys as ``unet.state_dict()`` /
        ``vae.state_dict()`` name them after adapter injection (``X.base_layer.weight``, ``X.lora_A.<adapter>.weight``),
        filtered with the reference's substring tests, so the file loads back through from_pix2pix_checkpoint (and into the
        reference itself)."""
        sd = {"unet_lora_target_modules": self.target_modules_unet, "vae_lora_target_modules": self.target_modules_vae,
              "rank_unet": self.lora_rank_unet, "rank_vae": self.lora_rank_vae,
              "state_dict_unet": {k: v for k, v in self.weights.unet.items() if "lora" in k or "conv_in" in k},
              "state_dict_vae": {k: v for k, v in self.weights.vae.items() if "lora" in k or "skip" in k}}
        torch.save(sd, outf)

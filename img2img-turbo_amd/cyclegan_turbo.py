"""CycleGAN_Turbo with the reference's API surface (src/cyclegan_turbo.py:109-254), MI355X-native inside.

``forward(x_t, direction=None, caption=None, caption_emb=None)`` follows :241-254; the generator itself is
``forward_with_networks`` (:199-207): VAE (``vae`` for a2b, ``vae_b2a`` for b2a, :21-27/:36-45) -> one shared
UNet -> per-sample scheduler step (same closed form for every sample; the reference's ``timesteps[i]``
indexing only works at B=1, here a length-1 ``timesteps`` broadcasts) -> VAE decode with skips -> clamp.
"""
from typing import Optional

import torch

from .pix2pix_turbo import TurboGeneratorBase, _NetHandle, _bind, seed_argument
from .weights import GeneratorWeights, from_cyclegan_checkpoint, load_checkpoint_file, load_sd_turbo_base

PRETRAINED = {  # src/cyclegan_turbo.py:126-149: name -> (checkpoint file, caption, direction)
    "day_to_night": ("day2night.pkl", "driving in the night", "a2b"),
    "night_to_day": ("night2day.pkl", "driving in the day", "b2a"),
    "clear_to_rainy": ("clear2rainy.pkl", "driving in heavy rain", "a2b"),
    "rainy_to_clear": ("rainy2clear.pkl", "driving in the day", "b2a"),
}


class CycleGAN_Turbo(TurboGeneratorBase):
    def __init__(self, pretrained_name=None, pretrained_path=None, ckpt_folder="checkpoints", lora_rank_unet=8, lora_rank_vae=4,
                 *, weights: Optional[GeneratorWeights] = None, base_dir=None, caption=None, direction=None, **kw):
        self.caption, self.direction = caption, direction
        if weights is None:
            import os
            base_dir = base_dir or os.environ.get("I2I_SD_TURBO_DIR")
            if base_dir is None:
                raise ValueError("give weights=GeneratorWeights(...), base_dir=<local sd-turbo snapshot> or set I2I_SD_TURBO_DIR "
                                 "(no network here)")
            if pretrained_name in PRETRAINED:
                fn, cap, dr = PRETRAINED[pretrained_name]
                pretrained_path = os.path.join(ckpt_folder, fn)
                caption, direction = cap, dr
            if pretrained_path is None:
                raise ValueError("pretrained_name or pretrained_path required")
            unet, _ = load_sd_turbo_base(base_dir)
            weights = from_cyclegan_checkpoint(unet, load_checkpoint_file(pretrained_path))
        super().__init__(weights, **kw)
        self.caption, self.direction = caption, direction
        # the wrappers the reference builds at src/cyclegan_turbo.py:115-116 (each holds both VAEs, picks one per direction)
        self.vae_enc = _NetHandle("vae_enc", weights.vae, weights.vae_b2a if weights.vae_b2a is not None else weights.vae)
        self.vae_dec = _NetHandle("vae_dec", weights.vae, weights.vae_b2a if weights.vae_b2a is not None else weights.vae)
        self.vae_enc._model = self.vae_dec._model = self.unet._model = self

    @torch.no_grad()
    def forward_u8(self, images_u8, *args, resize=None, resize_back=False, image_prep=None, tile=None, tile_overlap=64, tile_batch=8, jpeg=None,
                   png=None, **kw):
        """uint8 HWC in/out on the device: ``Normalize([0.5],[0.5])(to_tensor(img))`` (src/inference_unpaired.py:47) and
        ``ToPILImage()(out*0.5+0.5)`` (:53) run inside the boundary kernels.  ``resize=(width, height)`` applies the script's
        ``transforms.Resize(..., LANCZOS)`` (:40-47, e.g. (512, 512) for "resize_512x512") before the generator and
        ``resize_back=True`` its ``output_pil.resize((input width, input height), Image.LANCZOS)`` (:53) after it, both on the
        device and bit-identical to Pillow (image_ops.lanczos_resize_u8).  ``seed=``: as in ``forward``.
        ``images_u8`` may also be a LIST of uint8 [H_b, W_b, 3] tensors of different sizes -- one request each, as the script handles one
        file each -- with ``resize=(width, height)`` or ``image_prep="resize_512x512"`` / ``"resize_256x256"`` (and their short forms): two
        launches bring the batch to the model size and, with ``resize_back=True``, two more take every output back to its request's own size
        (image_ops.lanczos_resize_u8_ragged); the result is then a list, element b bit-identical to the per-image resize.  A list without a
        common size in front of the generator (no ``resize``, ``image_prep="resized_crop_512"`` / ``"no_resize"``) is a ValueError.
        ``tile=(tile width, tile height)`` with ``tile_overlap`` / ``tile_batch``: the request keeps its size and runs as overlapping tiles
        of the model size, cut and feather-blended on the device, as Pix2Pix_Turbo.forward_u8 describes (noise rule, refusals and the
        caveat on picture quality included); ``resize=`` / ``image_prep=`` apply first, ``resize_back=True`` is refused, and a list of
        requests of different sizes needs no common size.
        ``jpeg=True`` / a quality / ``(quality, "4:4:4" | "4:2:0")`` / a list of one such entry per image: the script's
        ``output_pil.save(...)`` (src/inference_unpaired.py:58) on the device, as Pix2Pix_Turbo.forward_u8 describes -- a list of ``bytes``,
        byte-identical to Pillow's files; with ``resize_back=True`` or ``tile=`` on a list every request is encoded at its own size.
        ``png=True``: the same line when the name ends in .png -- a list of ``bytes``, PNG files with Pillow's container and filtered
        scanlines and this project's deflate stream (image_ops.png_encode_u8), lossless; composes as ``jpeg=`` does and is refused beside it."""
        if png is not None:
            from . import image_ops
            want = image_ops.png_argument(png, jpeg)
            res = self.forward_u8(images_u8, *args, resize=resize, resize_back=resize_back, image_prep=image_prep, tile=tile, tile_overlap=tile_overlap,
                                  tile_batch=tile_batch, jpeg=jpeg, **kw)
            if not want:
                return res
            with self._on_device():
                return image_ops.png_files(res, self.lib)
        if jpeg is not None:
            from . import image_ops
            n = images_u8.shape[0] if torch.is_tensor(images_u8) else len(images_u8)
            spec = image_ops.jpeg_argument(jpeg, n)
            res = self.forward_u8(images_u8, *args, resize=resize, resize_back=resize_back, image_prep=image_prep, tile=tile, tile_overlap=tile_overlap,
                                  tile_batch=tile_batch, **kw)
            with self._on_device():
                return image_ops.jpeg_files(res, spec, self.lib)
        if tile is not None:
            return self._forward_u8_tiled(images_u8, _bind(("direction", "caption", "caption_emb"), args, kw), resize=resize, resize_back=resize_back,
                                          image_prep=image_prep, tile=tile, tile_overlap=tile_overlap, tile_batch=tile_batch)
        if isinstance(images_u8, (list, tuple)):
            return self._forward_u8_list(list(images_u8), *args, resize=resize, resize_back=resize_back, image_prep=image_prep, **kw)
        assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3
        in_hw = images_u8.shape[1:3]
        if image_prep is not None:          # the script's build_transform(args.image_prep) (src/inference_unpaired.py:40, default "resize_512x512")
            from .image_ops import apply_image_prep
            with self._on_device():
                images_u8 = apply_image_prep(images_u8, image_prep, self.lib)
        if resize is not None:
            from .image_ops import lanczos_resize_u8
            with self._on_device():
                images_u8 = lanczos_resize_u8(images_u8, resize, self.lib)
        out = self.forward(images_u8, *args, _u8_io=(2.0, -1.0), **kw)
        if resize_back and tuple(out.shape[1:3]) != tuple(in_hw):
            from .image_ops import lanczos_resize_u8
            with self._on_device():
                out = lanczos_resize_u8(out, (in_hw[1], in_hw[0]), self.lib)
        return out

    def _forward_u8_tiled(self, images, opts, *, resize, resize_back, image_prep, tile, tile_overlap, tile_batch):
        """forward_u8 with ``tile=`` (see there)."""
        from . import image_ops
        unknown = set(opts) - {"direction", "caption", "caption_emb", "eps", "seed"}
        if unknown:
            raise TypeError("forward_u8: unexpected arguments %s" % sorted(unknown))
        self._tile_refusals(tile, tile_batch, eps=opts.get("eps"), resize_back=resize_back)
        stacked = torch.is_tensor(images)
        sizes = {"resize_256": (256, 256), "resize_256x256": (256, 256), "resize_512": (512, 512), "resize_512x512": (512, 512)}
        with self._on_device():
            if stacked:
                if image_prep is not None:
                    images = image_ops.apply_image_prep(images, image_prep, self.lib)
                if resize is not None:
                    images = image_ops.lanczos_resize_u8(images, resize, self.lib)
            elif image_prep is not None and image_prep != "no_resize" and image_prep not in sizes:
                raise ValueError("image_prep %r does not apply to a list of images of different sizes" % (image_prep,))
            elif resize is not None or image_prep in sizes:
                size = (int(resize[0]), int(resize[1])) if resize is not None else sizes[image_prep]
                images, stacked = image_ops.lanczos_resize_u8_ragged(list(images), size, self.lib), True
        items = list(images.unbind(0)) if stacked else list(images)
        if not items or any(not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3 for t in items):
            raise ValueError("forward_u8(tile=...): uint8 [B, H, W, 3], or a list of uint8 [H, W, 3] requests")
        direction = opts.get("direction") or self.direction
        assert direction in ("a2b", "b2a")
        caption_enc = opts.get("caption_emb")
        if caption_enc is None:
            caption = opts.get("caption") or self.caption
            assert caption is not None
            caption_enc = self.encode_prompt(caption)

        def chunk(tiles, cap, eps, noise):
            return self.forward(tiles, direction=direction, caption_emb=cap, eps=eps, _u8_io=(2.0, -1.0))

        return self._forward_tiles(items, stacked, chunk, tile=tile, tile_overlap=tile_overlap, tile_batch=tile_batch, seed=opts.get("seed"),
                                   stochastic=False, caption_enc=caption_enc)[0]

    def _forward_u8_list(self, images, *args, resize, resize_back, image_prep, **kw):
        """forward_u8 for a list of images of different sizes (see there)."""
        from .image_ops import lanczos_resize_u8_ragged
        sizes = {"resize_256": (256, 256), "resize_256x256": (256, 256), "resize_512": (512, 512), "resize_512x512": (512, 512)}
        if image_prep is not None and image_prep not in sizes:
            raise ValueError("image_prep %r does not bring a list of images of different sizes to one size (use resize_256[x256] / "
                             "resize_512[x512] or resize=(width, height))" % (image_prep,))
        if image_prep is None and (resize is None or isinstance(resize, str)):
            raise ValueError("a list of images of different sizes needs resize=(width, height) or a resizing image_prep")
        size = (int(resize[0]), int(resize[1])) if resize is not None else sizes[image_prep]      # (resize after image_prep wins, as for tensors)
        with self._on_device():
            batch = lanczos_resize_u8_ragged(images, size, self.lib)
        out = self.forward(batch, *args, _u8_io=(2.0, -1.0), **kw)
        if not resize_back:
            return out
        with self._on_device():
            return lanczos_resize_u8_ragged(out, [(int(t.shape[1]), int(t.shape[0])) for t in images], self.lib)

    @staticmethod
    @torch.no_grad()
    def forward_with_networks(x, direction, vae_enc, unet, vae_dec, sched, timesteps, text_emb, *, eps=None):
        """Static generator entry of the reference (src/cyclegan_turbo.py:199-207), called as
        ``CycleGAN_Turbo.forward_with_networks(x, "a2b", model.vae_enc, model.unet, model.vae_dec, model.sched,
        model.timesteps, text_emb)`` (src/train_cyclegan_turbo.py:181).  The three network arguments must be the handles of
        ONE model of this package (they name its planned program: vae_enc(x, direction) -> unet -> per-sample sched.step ->
        vae_dec(x, direction)); ``sched`` / ``timesteps`` are the fixed one-step schedule and are checked, not used."""
        model = getattr(unet, "_model", None)
        if model is None or getattr(vae_enc, "_model", None) is not model or getattr(vae_dec, "_model", None) is not model:
            raise ValueError("forward_with_networks: pass model.vae_enc, model.unet, model.vae_dec of one CycleGAN_Turbo")
        assert direction in ("a2b", "b2a")
        ts = [int(t) for t in (timesteps.tolist() if hasattr(timesteps, "tolist") else list(timesteps))]
        if any(t != model.weights.unet_arch.timestep for t in ts):
            raise ValueError("the planned forward is specialised for the reference's fixed timestep %d" % model.weights.unet_arch.timestep)
        return model.forward(x, direction=direction, caption_emb=text_emb, eps=eps)

    @torch.no_grad()
    def forward(self, x_t, direction=None, caption=None, caption_emb=None, *, eps=None, seed=None, _u8_io=None):
        """``seed=s``: the posterior draw comes from the device at (seed s, step 0) under the contract of i2i_randn_params
        (include/i2i_turbo.h; img2img_turbo_amd.rng) instead of a host-side ``torch.randn``; not together with ``eps=``.
        ``seed=[s0, .., sB-1]``: one seed per image, slot-independent noise (i2i_randn_batch_params), as Pix2Pix_Turbo.forward."""
        if seed is not None and eps is not None:
            raise ValueError("seed= draws eps on the device: do not pass eps= with it")
        seed = seed_argument(seed, x_t.shape[0])
        if direction is None:
            assert self.direction is not None
            direction = self.direction
        assert direction in ("a2b", "b2a")
        if caption is None and caption_emb is None:
            assert self.caption is not None
            caption = self.caption
        caption_enc = caption_emb if caption_emb is not None else self.encode_prompt(caption)
        if _u8_io is not None:
            B, H, W, _ = x_t.shape
        else:
            B, _, H, W = x_t.shape
        lat = self.weights.vae_arch.latent_channels
        if eps is None and seed is None:
            eps = torch.randn(B, lat, H // 8, W // 8, device=self.device_, dtype=torch.float32)
            torch.randn(B, lat, H // 8, W // 8, device=self.device_, dtype=torch.float32)
        ctx_batch = caption_enc.shape[0] if caption_enc.dim() == 3 else 1
        plan = self.get_plan(B, H, W, direction=direction, ctx_batch=ctx_batch, u8_io=_u8_io,
                             rng=("per_image" if isinstance(seed, list) else seed is not None))
        out = self._execute(plan, x_t, caption_enc, eps, seed=seed)
        return out if _u8_io is not None else out.to(x_t.dtype)

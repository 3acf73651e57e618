/*
 * i2i_turbo.h -- C ABI of the MI355X (gfx950) kernels behind Pix2Pix_Turbo / CycleGAN_Turbo .forward().
 *
 * The reference (GaParmar/img2img-turbo) has no FFI/plugin interface: its hot path
 * (src/pix2pix_turbo.py:186-219, src/cyclegan_turbo.py:199-207, src/model.py:14-54) reaches its
 * kernels through torch.nn.functional inside diffusers/peft.  Each entry point below names the
 * library call(s) it replaces on that path.  All functions are `extern "C"`, take plain pointers and
 * sizes (no torch types), never allocate device memory, never synchronise, and launch asynchronously
 * on the caller's hipStream_t (graph-capturable).  Return value: 0 = ok, negative = error; the message
 * is available from i2i_last_error().
 *
 * Activations are NHWC ("tokens" [B, H*W, C] are the same memory), element type = `dtype`.
 * Channel counts of every activation tensor are multiples of 8 (inputs are padded once at the boundary).
 * Weights are packed [Cout][KH][KW][Cin] (k contiguous) in `dtype`; biases and norm affine parameters
 * are fp32.
 */
#ifndef I2I_TURBO_H
#define I2I_TURBO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I2I_ABI_VERSION 14

typedef enum { I2I_F32 = 0, I2I_BF16 = 1, I2I_F16 = 2,
               I2I_U8 = 3   /* only as src_dtype / dst_dtype of the boundary layout ops: uint8 images, HWC interleaved */
} i2i_dtype;

typedef enum {
    I2I_OK = 0,
    I2I_ERR_BAD_ARG = -1,      /* unsupported shape / alignment / null pointer */
    I2I_ERR_LAUNCH = -2,       /* HIP reported an error at launch */
    I2I_ERR_UNSUPPORTED = -3,
    I2I_ERR_RUNTIME = -4,      /* other HIP runtime failure (graph capture, events) */
    I2I_ERR_MISMATCH = -5      /* i2i_plan_verify: a buffer's digest differs from the one stored in the plan file */
} i2i_status;

typedef enum {
    I2I_OP_IGEMM = 1,
    I2I_OP_GN_STATS = 2,
    I2I_OP_LAYERNORM = 3,
    I2I_OP_SOFTMAX = 4,
    I2I_OP_NCHW_TO_NHWC = 5,
    I2I_OP_NHWC_TO_NCHW = 6,
    I2I_OP_POSTERIOR = 7,
    I2I_OP_DDPM_POSTQUANT = 8,
    I2I_OP_ATTENTION = 9,
    I2I_OP_GN_APPLY = 10,
    I2I_OP_EMBED = 11,
    I2I_OP_LORA_MERGE = 12,
    I2I_OP_RESIZE_U8 = 13,
    I2I_OP_NOP = 14,           /* one empty kernel launch (bench.py's calibration: microseconds per hipGraph node) */
    I2I_OP_CANNY_U8 = 15,
    I2I_OP_RANDN = 16,
    I2I_OP_TWIN_FOLD = 17,
    I2I_OP_SCAN = 18,
    I2I_OP_RANDN_BATCH = 19,   /* ABI 14 additions (see the note above i2i_randn_batch_params) */
    I2I_OP_CANNY_U8_BATCH = 20,
    I2I_OP_RESIZE_U8_RAGGED = 21,  /* ABI 14 addition (see the note above i2i_resize_u8_ragged_params) */
    I2I_OP_SCAN_BATCH = 22,        /* ABI 14 additions (see the note above i2i_scan_batch_params) */
    I2I_OP_SCAN_VERDICT = 23,
    I2I_OP_CANNY_AUTO_THR = 24,    /* ABI 14 addition (see the note above i2i_canny_auto_thr_params) */
    I2I_OP_DIGEST = 25,            /* ABI 14 addition (see the note above i2i_digest_params) */
    I2I_OP_REPEAT = 26,            /* ABI 14 addition (see the note above i2i_repeat_params) */
    I2I_OP_TILE_CUT = 27,          /* ABI 14 additions (see the note above i2i_tile_request) */
    I2I_OP_TILE_BLEND_U8 = 28
} i2i_opcode;

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear / batched matmul on MFMA.
 *   C[m][n] = epilogue( alpha * sum_k A[m][k] * B[n][k] )
 * Replaces F.conv2d (3x3 s1/s2, 1x1), F.linear and the q.k^T / p.v matmuls of
 * F.scaled_dot_product_attention, with the surrounding F.group_norm+F.silu (as an A-operand
 * prologue), F.interpolate(nearest 2x) and torch.cat (as A-operand gathers), F.pad(0,1,0,1), bias,
 * residual add, skip add (src/model.py:41-43) and GEGLU fused in.  LoRA (peft) is merged into B at
 * load (W' = W + s.B.A), so one launch covers base + adapter.
 *
 * A operand: virtual concat of up to two NHWC sources [nimg][hin][win][c0 | c1]; m -> (img, oy, ox),
 *            k -> (ky, kx, ci); input coord = up_map(o*stride + k - pad) (>> ups, or the explicit up_h/up_w map), zero outside.
 *            z (grid z) adds zb*a_bs_b + zh*a_bs_h with zb = z / zh_count, zh = z % zh_count.
 * B operand: [N][ldb] k-contiguous (weights, or K of q.k^T, or V^T of p.v).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const void* a0; const void* a1;
    int32_t c0, c1;            /* channels per source (c1 = 0: single source); multiples of 8 */
    int32_t lda0, lda1;        /* pixel stride in elements (>= c0 / c1, multiple of 8) */
    int64_t a_bs_b, a_bs_h;    /* batch strides (elements) applied to BOTH sources */
    int32_t nimg, hin, win;    /* source geometry (before the optional 2x upsample) */
    int32_t ho, wo;            /* output geometry; M = nimg*ho*wo */
    int32_t ks, stride, pad, ups;
    const void* b; int32_t ldb; int64_t b_bs_b, b_bs_h;
    int32_t M, N, K;           /* K = ks*ks*(c0+c1) */
    const float* gn_ss;        /* optional [nimg][c0+c1][2] = (scale, shift) from I2I_OP_GN_STATS */
    int32_t act;               /* 0 none, 1 SiLU (after the affine) */
    const float* bias; int32_t bias_mode;   /* 0 none, 1 per column n, 2 per row m */
    float alpha;
    const void* res; int32_t ldr; int64_t r_bs_b, r_bs_h;   /* optional residual, same dtype */
    void* c; int32_t ldc; int64_t c_bs_b, c_bs_h;
    int32_t zcount, zh_count;  /* grid z = zcount batches; zh_count heads per batch (>= 1) */
    int32_t geglu;             /* 1: B rows interleaved [a16|g16]; out[:, n/2] = a * gelu(g); ldc for N/2 */
    int32_t out_f32;           /* 1: store fp32 regardless of dtype (attention scores) */
    int32_t tile;              /* 0 = auto; else forces a kernel / tile config id (tests / tuning):
                                  1-5 register-staged igemm, 10-19 / 30-39 halo conv3x3, 20-26 LDS-DMA igemm (26: 64x32 tiles),
                                  40-49 wide-tile conv3x3 (32x32x16 MFMA, conv3x3_w32.hip; 40 = its own auto; with `subpix` its
                                  sub-pixel upsampler form), 50-56 wide GEMM (32x32x16 MFMA, gemm_w32.hip; 50 = its own auto,
                                  51 256x160, 52 128x160, 53 256x128, 54 128x128 workgroup tiles; 55 / 56 = 52 / 54 with a 2-deep
                                  ring, two workgroups per CU); 60-69 the narrow-input 3x3 conv (8 padded input channels into a multiple
                                  of 128 output channels: the VAE's conv_in; conv_narrow.hip).
                                  `bias` (bias_mode 1) must be 4-byte aligned; the 3x3 conv routes need it 16-byte aligned */
    int32_t splitk;            /* > 1: split the K loop over grid z; needs `ws`; no GEGLU, zcount == 1 */
    void* ws;                  /* fp32 workspace, >= splitk * M * N floats (split-K partial slabs) */
    float* gn_part;            /* optional: GroupNorm partial sums of the OUTPUT tensor (as stored), written by the
                                  epilogue as [nimg][parts][gn_part_groups][2] = (sum, sum of squares) with
                                  parts = i2i_igemm_gn_parts(); finished by I2I_OP_GN_STATS with finalize_only */
    int32_t gn_part_groups;
    int32_t subpix;            /* 1 (with ups = 1, ks = 3, stride 1, pad 1): `b` holds the SUB-PIXEL form of the
                                  upsample+conv, [4 parities (a,b)][N][2*2*cin] with ldb = 4*cin, tap weights
                                  pre-summed per output parity (packer.subpixel_weights); K stays 9*cin */
    int32_t act_out;           /* epilogue activation after alpha/bias, before the residual: 0 none, 1 GELU (erf form,
                                  CLIP ViT-H MLP), 2 quick_gelu x*sigmoid(1.702x) (CLIP ViT-L).  LDS-DMA igemm only */
    int32_t up_h, up_w;        /* ups = 1 only: explicit size of the nearest-upsampled plane (F.interpolate(size=...), the
                                  UNet's forward_upsample_size path for latent sizes that are not multiples of 8);
                                  0,0 = (2*hin, 2*win).  Source index = min(floor(i * in/up), in-1) as ATen computes it */
    /* Optional SECOND contraction accumulated into the same output before the epilogue:
     *     acc += k2_a[m][0..k2_c) . k2_b[n][0..k2_c)^T        (so `alpha` scales it like the first contraction),
     * a 1x1 convolution over another NHWC tensor at OUTPUT resolution ([nimg][ho][wo][k2_lda], same dtype; k2_b is [N][k2_ldb]).
     * It is the decoder's `sample = sample + skip_conv_i(skip * gamma)` (src/model.py:41-43) folded into the Upsample2D conv
     * that produces `sample` (no read-modify-write pass over the stream), and a ResnetBlock2D's conv_shortcut(input) folded
     * into its conv2.  k2_c a multiple of 64; taken by the wide-tile conv only (i2i_igemm_route() == "conv3x3_w32_kernel" or
     * "conv3x3_w32_kernel<SUBPIX>"), anything else returns I2I_ERR_UNSUPPORTED. */
    const void* k2_a; const void* k2_b;
    int32_t k2_c, k2_lda, k2_ldb;
    /* LayerNorm folded into this GEMM (ABI v9; the wide GEMM only, ks = 1, one source, no split-K): `a0` holds the UN-normalised rows x and
     * the launch computes  C = LN(x) . W^T + b  (F.layer_norm over the K channels, eps = ln_eps, followed by F.linear: the norm1 -> to_q / to_k /
     * to_v, norm2 -> to_q and norm3 -> ff.net.0.proj pairs of diffusers' BasicTransformerBlock under src/pix2pix_turbo.py:199) as
     *     C[m][n] = rstd_m * (x_m . W'_n) - rstd_m * mu_m * ln_cs[n] + bias[n],
     * with W'[n][k] = W[n][k] * gamma[k] in `b` (folded by i2i_lora_merge: kscale), ln_cs[n] = sum_k W'[n][k] over the STORED (rounded)
     * weights and bias[n] = b[n] + sum_k W[n][k] * beta[k] (both written by i2i_lora_merge).  mu_m / rstd_m are accumulated from the row
     * fragments in the K loop (no extra pass over x, no normalised copy of x in HBM).  NULL = off.
     * Supported DC offset of a row: |mu| <= 100 sigma (mu^2 / var <= 1e4).  Up to there the result is no worse than the unfused
     * i2i_layernorm + i2i_igemm pair (asserted: RMS <= 1.25 x, max-abs <= 1.5 x that pair's error, tests/opcheck.py check_ln_gemm); fp16
     * takes its sums of x - p for that, p = the median of the row's first, middle and last element (one outlier channel or one 0 among
     * them does not matter; a pivot r sigma from the mean leaves the sums as exposed as plain ones at an offset of r sigma, r <= sqrt(K)
     * for any row element -- fp16 at K = 1280 with two of the three overwritten measures up to 2.3 x the pair's error), bf16 the plain one-pass sums (its own
     * rounding step is the larger term).  fp16 rows spanning more than 65504 overflow x - p: not supported.  Beyond 100 sigma is measured
     * only: bf16 rows of |mu| >= 300 sigma can have var clamped to 0 -- route such tensors through i2i_layernorm. */
    const float* ln_cs; float ln_eps;
    /* Transposed column range (with ln_cs only): output columns n >= n_trans are written TRANSPOSED to c2[(n - n_trans) * ldc2 + m]
     * (the self-attention V^T [C][B*T] the flash kernel reads), columns below it to `c` as usual: to_q | to_k | to_v in ONE launch.
     * n_trans a multiple of the tile width (160 / 128), M a multiple of 8; 0 = off. */
    int32_t n_trans; void* c2; int32_t ldc2;
} i2i_igemm_params;

/* GroupNorm statistics -> per (image, channel) (scale, shift) so that GN(x)[c] = x*scale + shift.
 * Replaces the reduction half of F.group_norm; the affine+SiLU half runs in the consumer's prologue.
 * Two-stage and atomics-free (deterministic).  One-pass sums (sum, sum of squares) in fp32 with a second, shifted pass over
 * exactly the groups where |mean| > 16 sigma (F.group_norm is two-pass; DESIGN.md "Numerics").  `partial` needs nimg*nparts*groups*2 floats. */
typedef struct {
    const void* x0; const void* x1; int32_t c0, c1, ld0, ld1;
    int32_t nimg, hw, groups; float eps;
    const float* gamma; const float* beta;    /* [c0+c1] fp32 */
    float* partial; int32_t nparts;
    float* ss;                                /* out [nimg][c0+c1][2] */
    int32_t finalize_only;                    /* 1: `partial` was produced by a conv epilogue (gn_part).  x0 (+ ld0) may still be
                                                 given: groups whose one-pass variance is below mean^2 / 256 (cancellation) are
                                                 then re-read against the first-pass mean; with x0 = NULL the one-pass numbers stand */
    int32_t* counters;                        /* optional (ABI v7), >= nimg*groups ints, ZERO before the first launch (the kernel leaves
                                                 them zero): lets the single-launch path for small tensors cut every image's pixels
                                                 into up to `nparts` slices, one workgroup each; the workgroup that arrives last at
                                                 its (image, group set) ticket sums the slices in a fixed order and writes `ss`.
                                                 CONCURRENCY: `counters` / `partial` are state of the launch in flight -- an op (and therefore
                                                 a program, a captured graph or a loaded plan file that contains it) must not run on two
                                                 streams at once; consecutive launches on one stream are fine (the kernel leaves the
                                                 counters at zero).  The same holds for every scratch slab an op names (gn_part, ws). */
} i2i_gn_stats_params;

/* Standalone GN apply (+SiLU): y = act(x*scale+shift).  Used where the consumer cannot apply it in its
 * operand staging (LDS-DMA igemm on the small UNet planes, unfused VAE attention), and when fusion is disabled. */
typedef struct {
    const void* x; void* y; const float* ss; int32_t nimg, hw, c, act;
    int32_t ldx, ldy;          /* pixel strides in elements (0 = c): y may be a channel slice of a concat buffer */
    int32_t ss_ld, ss_off;     /* ss is [nimg][ss_ld][2]; this tensor's channels start at ss_off (0,0 = c,0) */
    const void* x1;            /* ABI v10: optional SECOND source [nimg*hw][ldx1] of c1 channels (torch.cat([x, x1], 1) in front of the norm:
                                  the resnets of the UNet's up blocks): its channels follow x's in y and in ss -- one launch normalises the
                                  concatenated input (it was one launch per source) */
    int32_t c1, ldx1;          /* c1 multiple of 8; ldx1 = 0 means c1 */
} i2i_gn_apply_params;

/* LayerNorm over the last dim (F.layer_norm, eps 1e-5, affine). rows x c, c multiple of 8. */
typedef struct {
    const void* x; void* y; const float* gamma; const float* beta; int32_t rows, c, ldx, ldy; float eps;
} i2i_layernorm_params;

/* Row softmax of fp32 scores: p = softmax(scale * s) written as `dtype` with zero padding up to ldp.
 * The softmax step of F.scaled_dot_product_attention on the unfused path. */
typedef struct {
    const float* s; void* p; int64_t rows; int32_t cols, lds, ldp; float scale;
} i2i_softmax_params;

/* Fused flash-style attention (F.scaled_dot_product_attention, no mask, not causal).
 * q [b][tq][ldq] / k [b][tk][ldk] with head h at column h*d; vt is V^T: [b][heads*d][ldvt] (tk contiguous).
 * o = softmax(scale * q k^T) v.  The 16-bit d = 64 kernel works in log2 units: it multiplies q by scale * log2(e) once at load (one
 * more rounding of q to the 16-bit type) UNLESS scale * log2(e) == 1, i.e. the caller passes q already multiplied by the factor and
 * scale = ln 2 -- the same function, and what the model's planner does (the factor is folded into to_q's weights before they are
 * rounded: Packer out_scale / scale0). */
typedef struct {
    const void* q; const void* k; const void* vt; void* o;
    int32_t batch, heads, d, tq, tk, ldq, ldk, ldvt, ldo;
    int64_t q_bs, k_bs, vt_bs, o_bs; float scale;
    int32_t causal;            /* 1: query i attends to keys <= i (CLIP text tower); needs tq == tk */
    int32_t ksplit;            /* > 1 (the 16-bit LDS-DMA kernels, d = 512 and d = 64, no causal mask): the keys are divided among ksplit
                                  workgroups per query tile and a second launch merges the partial results -- for launches with too few
                                  query tiles to fill the chip (batch 1: 32 tiles of 128 queries on 256 CUs; the d = 64 self-attention
                                  over 4096 tokens: 64 serial key tiles per workgroup).  Needs `ws`; 0 / 1 = off */
    void* ws;                  /* fp32 workspace for ksplit: batch*heads*ksplit*tq*(d + 2) floats, 16-byte aligned */
} i2i_attention_params;

/* Token + position embedding of the CLIP text tower (transformers CLIPTextEmbeddings; the tokenizer side stays on the
 * host): y[row][:] = tok[ids[row]][:] + pos[row % T][:], rows = B*T, tables and output in `dtype`. */
typedef struct {
    const int64_t* ids; const void* tok; const void* pos; void* y; int32_t rows, T, c, vocab;
} i2i_embed_params;

/* Boundary layout ops.  NCHW fp32/`dtype` <-> NHWC `dtype` with channel padding (zeros).
 * With src_dtype / dst_dtype = I2I_U8 the outer tensor is a uint8 image batch [n][h][w][c] (HWC, as PIL / numpy hand
 * it over) and the callers' pre/post-processing is folded in:
 *   in : y = u8/255 * mul + add     (F.to_tensor, src/inference_paired.py:50; Normalize([0.5],[0.5]) = mul 2, add -1,
 *                                     src/inference_unpaired.py:47); with binarize_below: the sketch threshold, see the struct
 *   out: u8 = trunc(clamp01(v*mul + add) * 255)   (ToPILImage()(x*0.5+0.5) = mul .5, add .5: src/inference_paired.py:72) */
typedef struct {
    const void* x; void* y; int32_t n, c, h, w, cpad; int32_t src_dtype; float mul, add;
    int32_t binarize_below;    /* I2I_U8 sources only, 0 = off: v = (u8 < binarize_below) ? 1 : 0 instead of u8/255, then v*mul + add.
                                  128 = the sketch script's `F.to_tensor(image) < 0.5` (src/inference_paired.py:57-58: 127/255 < 0.5 <= 128/255) */
} i2i_nchw_to_nhwc_params;
typedef struct {
    const void* x; void* y; int32_t n, c, h, w, ldx; int32_t dst_dtype; int32_t clamp; /* clamp to [-1,1] */
    float mul, add;            /* applied after the clamp; 0,0 means 1,0 */
} i2i_nhwc_to_nchw_params;

/* DiagonalGaussianDistribution.sample() * scaling_factor (+ stochastic mix, src/pix2pix_turbo.py:210):
 * z = (mean + exp(.5*clamp(logvar,-30,20)) * eps) * sf ; u = z*r + noise*(1-r)  (r = 1 => u = z).
 * moments NHWC [n][hw][ldm] (mean = ch 0..lat-1, logvar = lat..2lat-1); eps/noise NCHW fp32 [n][lat][hw]
 * (noise may have n = 1 and is broadcast); u NHWC padded to ldu channels (zeros). */
typedef struct {
    const void* moments; const float* eps; const float* noise; void* u;
    int32_t n, hw, lat, ldm, ldu, noise_n; float sf, r;
    const float* r_dev; /* optional device scalar overriding `r` at run time (the program / hipGraph stays valid when the
                           caller changes r: gradio_sketch2image.py sweeps it per request) */
    float* u_f32;      /* optional fp32 copy [n][hw][lat] for the scheduler step (keeps latent math fp32) */
    int32_t moments_f32; /* 1: moments are fp32 (producer igemm stored with out_f32) */
} i2i_posterior_params;

/* DDPMScheduler.step at the single timestep + /scaling_factor + post_quant_conv (1x1, lat x lat):
 * x0 = (u - sqrt(1-abar)*e)/sqrt(abar) ; y = Wpq.(x0/sf) + bpq.  All fp32 in registers. */
typedef struct {
    const void* u; const void* e; void* y; const float* wpq; const float* bpq;
    int32_t n, hw, lat, ldu, lde, ldy; float sqrt_abar, sqrt_1m_abar, sf;
    int32_t u_f32, e_f32;  /* 1: that operand is fp32 (ldu/lde in fp32 elements) */
} i2i_ddpm_params;

/* Device-side LoRA re-merge into a packed weight tensor (peft's merged form; the reference keeps adapters as side branches
 * and rescales them per call: unet.set_adapters(["default"], weights=[r]) / set_weights_and_activate_adapters(vae, ..., [r])
 * src/pix2pix_turbo.py:206-207, decoder.gamma = r :217):
 *   dst[n][k] = cvt( (w0[n][k] + r * sum_j b[n][j] * a[j][k]) * (use_gamma ? gamma : 1) ),  (r, gamma) = rg[0..1] on the device.
 * w0 fp32 master in the packed layout, a fp32 [rank][K] with lora_alpha/rank folded in (adapters concatenated along rank),
 * b fp32 [N][rank].  K multiple of 4.  rg = NULL means r = gamma = 1. */
typedef struct {
    void* dst; const float* w0; const float* a; const float* b;
    int32_t N, K, rank, use_gamma;
    const float* rg;
    /* LayerNorm fold (ABI v9, all NULL = off): the consumer GEMM computes LN(x) . W^T from the un-normalised rows (i2i_igemm_params.ln_cs):
     *   dst[n][k]   = cvt( w'[n][k] * kscale[k] ),  w' = (w0 + r b.a) * g as above, kscale = the LayerNorm weight
     *   colsum[n]   = sum_k float(dst[n][k])                 (of the ROUNDED values: a constant row then cancels exactly)
     *   bias_out[n] = (bias0 ? bias0[n] : 0) + sum_k w'[n][k] * kshift[k],   kshift = the LayerNorm bias
     * summed per row in a fixed order (deterministic, r -> r' -> r reproduces the bits). */
    const float* kscale; const float* kshift; const float* bias0;
    float* colsum; float* bias_out;
} i2i_lora_merge_params;

/* One separable pass of Pillow's LANCZOS resampling on uint8 HWC image batches [n][hin][win][c] (c <= 4), bit-identical to
 * Image.resize(size, Image.LANCZOS) when the horizontal pass (axis = 1: win -> nout columns) is followed by the vertical pass
 * (axis = 0: hin -> nout rows): the reference's host-side resizes (src/inference_paired.py:38-41, src/inference_unpaired.py:40,53).
 * bounds[o] = (first tap, tap count), coeffs[o][ksize] = 22-bit fixed-point weights, both device int32 arrays computed on the
 * host (image_ops.py restates Pillow's precompute_coeffs / normalize_coeffs_8bpc); out = clip8((2^21 + sum in*k) >> 22). */
typedef struct {
    const void* src; void* dst; int32_t n, hin, win, c;
    int32_t axis;              /* 1 = horizontal pass (resample x), 0 = vertical pass (resample y) */
    int32_t nout, ksize;       /* output extent along `axis`; weights per output coordinate */
    const int32_t* bounds; const int32_t* coeffs;
} i2i_resize_u8_params;

/* Canny edge detection on uint8 HWC image batches (ABI v11): cv::Canny(src, low, high) for 8-bit input with aperture 3 and
 * L2gradient = false, restated in integer arithmetic, replicated to out_c channels -- the reference's host-side
 * canny_from_pil (src/image_prep.py:6-12: cv2.Canny + the 3-channel replication) between the resize and F.to_tensor of the
 * edge_to_image script (src/inference_paired.py:47-50).  Per pixel:
 *   1. 3x3 Sobel dx, dy per channel (BORDER_REPLICATE);  2. mag = |dx| + |dy|, the pixel takes (dx, dy, mag) of the channel with the
 *   largest mag (lowest channel on a tie);  3. non-maximum suppression along the gradient direction quantised to 0 / 45 / 90 / 135
 *   degrees with the integer tangents tan(22.5) = 13573 / 2^15, mag outside the image = 0: a surviving pixel with mag > low is a
 *   candidate, strong if mag > high;  4. hysteresis: a candidate is an edge iff its 8-connected component of candidates holds a
 *   strong pixel;  5. dst = 255 on edges, 0 elsewhere.
 * The result is a pure function of the input (bit-identical from run to run; tests/canny_ref.py is the CPU oracle of this text).
 * Parity with OpenCV itself is unpinned where cv2 is absent (tests/test_canny_emu.py pins it where cv2 imports).
 * Five launches whatever the image holds (class map, tile-local labels, lock-free union of the tile roots across tile edges, strong
 * flags, output); no read-back, no grid-wide wait.  `ws` is state of the run in flight (see the CONCURRENCY note of i2i_gn_stats_params). */
typedef struct {
    const void* src; void* dst;        /* uint8 [n][h][w][c] -> uint8 [n][h][w][out_c]; 4-byte aligned */
    int32_t n, h, w, c, out_c;         /* c 1..4; out_c 1 or 3 */
    int32_t low, high;                 /* swapped if low > high */
    const int32_t* thr_dev;            /* optional device {low, high} read at run time: a captured graph / loaded plan stays valid
                                          when the caller moves the sliders (gradio_canny2image.py), like posterior.r_dev */
    void* ws;                          /* >= i2i_canny_ws_bytes(n, h, w) bytes, 16-byte aligned; contents irrelevant before and after */
} i2i_canny_u8_params;

/* Seeded Gaussian noise on the device (ABI v12): the `torch.manual_seed(seed); torch.randn(...)` of the reference's inference scripts
 * (src/inference_paired.py:58-60, the seed slider of gradio_sketch2image.py:80-82) as an op of the program, so that one plan, one
 * captured graph and one plan file serve every seed and a replay draws fresh noise without the host.  Bit parity with torch.randn or
 * cuRAND is NOT a goal (neither stream is specified, and torch-ROCm's differs from CUDA's); this is the contract, and
 * tests/randn_ref.py is its CPU oracle (integer Philox + an fp64 transform).
 *
 * Counter based and stateless per element: the bits do not depend on the grid.
 *   STATE    four uint32 {seed_lo, seed_hi, step, reserved}; the reserved word is ignored, whatever it holds.
 *   ELEMENT  i (0-based flat index into dst), q = i >> 2: lane i & 3 of Philox4x32-10 with counter
 *            {q & 0xffffffff, q >> 32, step, stream_id} and key {seed_lo, seed_hi}.  Random123 constants: multipliers 0xD2511F53 /
 *            0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85, 10 rounds, the key bumped after each round.  One round maps
 *            (c0, c1, c2, c3) to (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)).  A tail with n % 4 != 0
 *            drops the unused lanes.
 *   RAW      dst is uint32: the words as they are.
 *   NORMAL   dst is fp32: the words (w0, w1) and (w2, w3) are two Box-Muller pairs (wa, wb):
 *              u1 = ((wa >> 8) + 1) * 2^-24   in (0, 1], exact in fp32;   u2 = (wb >> 8) * 2^-24   in [0, 1)
 *              rad = sqrtf(-2 * logf(u1));   outputs rad * cospif(2 * u2), rad * sinpif(2 * u2)
 *            with the precise library functions (logf and the pi-scaled trigonometric functions at <= 1 ulp, sqrtf correctly
 *            rounded) -- no fast forms, no fp32 product 2*pi*u2.  Each output is within rad * 2^-21 of the exact transform of
 *            the same words (logf's ulp halved by the root, the root, 4 * 2^-24 absolute for the trigonometric value, the product),
 *            exactly 0 where rad = 0, and |x| <= sqrt(48 ln 2) ~ 5.77.
 *   ADVANCE  one thread does state[2] += 1 (wrapping); nothing else is written.  Stream order serialises it.
 * Stream ids of a planned forward: 0 = "eps" (the posterior draw), 2 = "noise" (the sketch model's noise_map); 1 is reserved for the
 * reference's numerically dead scheduler draw and never generated.  The index is flat, so image 0 of a batch gets the noise a
 * batch-1 run gets at the same (seed, step).
 * dst needs 4-byte alignment only (slices are fine); nothing is written outside dst[0 .. n-1].  With `state` set the device state is
 * read at run time (like canny_u8.thr_dev); with state = NULL the immediate seed / step are used. */
typedef enum { I2I_RANDN_NORMAL = 0, I2I_RANDN_RAW = 1, I2I_RANDN_ADVANCE = 2 } i2i_randn_kind;
typedef struct {
    void* dst;                         /* fp32 (normal) or uint32 (raw) [n]; ignored by advance */
    int64_t n;
    const uint32_t* state;             /* optional device {seed_lo, seed_hi, step, reserved}; advance writes state[2] */
    uint64_t seed; uint32_t step;      /* used when state == NULL */
    uint32_t stream_id;
    int32_t kind;                      /* i2i_randn_kind */
} i2i_randn_params;

/* ---- ABI 14 additions: per-image request parameters of a batch (I2I_OP_RANDN_BATCH, I2I_OP_CANNY_U8_BATCH).  They are purely additive --
 * new opcodes, new structs, new exported functions; no existing struct, opcode number or signature changed and sizeof(i2i_op) did not
 * grow (the union is sized by i2i_igemm_params) -- so I2I_ABI_VERSION stays 14: every program, plan file and host written against 14
 * runs unchanged.  A library built before the additions is recognised by the missing symbols (i2i_randn_batch, i2i_canny_u8_batch), and
 * its plan loader refuses the new opcodes as unknown.
 *
 * Per-image seeded noise: i2i_randn over a batch with ONE STATE PER IMAGE, so that the noise of a request does not depend on the slot a
 * batching host put it in, two requests of one batch can carry their own seeds, and a batch sharded over devices does not repeat image 0's
 * noise on every shard.
 *   STATES   device uint32 [batch][4], row b = {seed_lo, seed_hi, step, reserved} of image b (the i2i_randn_params state, per image); the
 *            reserved word is ignored, whatever it holds.  Read at run time: one program / graph / plan file serves every table.
 *   ELEMENT  j of image b (dst[b * per_image + j]) is element j of i2i_randn with n = per_image and the state states[b]: lane j & 3 of
 *            Philox4x32-10 with counter {(j >> 2) & 0xffffffff, (j >> 2) >> 32, states[b][2], stream_id} and key {states[b][0],
 *            states[b][1]}, then (NORMAL) the same Box-Muller.  The same device functions run: row b of the output is BIT-IDENTICAL to a
 *            batch-1 i2i_randn at image b's seed and step, in any slot, at any batch size.  A tail with per_image % 4 != 0 drops the
 *            unused lanes PER IMAGE (image b + 1 starts again at counter 0).
 *   RAW / NORMAL  as i2i_randn (dst uint32 / fp32).
 *   ADVANCE  states[b][2] += 1 (wrapping) for every b < batch; nothing else is written (words 0, 1, 3 and dst stay).
 * dst needs 4-byte alignment only; nothing is written outside dst[0 .. batch * per_image).  One launch for the fill, one for the advance; no
 * allocation, no synchronisation, graph-capturable.  batch == 0 or per_image == 0 is a successful no-op for the fill kinds.
 * Errors (I2I_ERR_BAD_ARG): null params; states null or not 4-byte aligned; negative batch / per_image (or a product past 2^61); dst null
 * or not 4-byte aligned (fill kinds); unknown kind.
 * This fixes the NOISE of an image.  It does not make image b of a batch-8 forward bit-equal to a batch-1 forward of the same request:
 * the contraction kernels choose routes and tiles by batch size. */
typedef struct {
    void* dst;                         /* fp32 (normal) or uint32 (raw) [batch][per_image], contiguous; ignored by advance */
    int64_t per_image;                 /* elements per image, >= 0 */
    int32_t batch;                     /* >= 0 */
    const uint32_t* states;            /* REQUIRED device [batch][4]: {seed_lo, seed_hi, step, reserved} per image; advance writes [b][2] */
    uint32_t stream_id;
    int32_t kind;                      /* i2i_randn_kind: NORMAL / RAW / ADVANCE */
} i2i_randn_batch_params;

/* Per-image Canny thresholds (ABI 14 addition): i2i_canny_u8 with one {low, high} pair per image, read from the device at run time (the
 * low / high sliders of gradio_canny2image.py, one pair per request of a batch).  Image b uses {thr[2b], thr[2b + 1]}, swapped if
 * low > high.  Everything else -- the arithmetic, the five launches, the workspace (i2i_canny_ws_bytes), the alignment rules -- is
 * i2i_canny_u8's: image b of the result is BIT-IDENTICAL to i2i_canny_u8 on image b alone with image b's pair (images never interact:
 * tiles, labels and unions stay inside an image).  Errors as i2i_canny_u8, plus thr null or not 4-byte aligned. */
typedef struct {
    const void* src; void* dst;        /* uint8 [n][h][w][c] -> uint8 [n][h][w][out_c]; 4-byte aligned */
    int32_t n, h, w, c, out_c;         /* c 1..4; out_c 1 or 3 */
    const int32_t* thr;                /* REQUIRED device int32 [n][2] = {low, high} per image */
    void* ws;                          /* >= i2i_canny_ws_bytes(n, h, w) bytes, 16-byte aligned; contents irrelevant before and after */
} i2i_canny_u8_batch_params;

/* TwinConv fold on the device (ABI v13): the sketch model's conv_in, `conv_in_pretrained(x) * (1 - r) + conv_in_curr(x) * r`
 * (src/pix2pix_turbo.py:16-26), as ONE packed weight tensor written by a kernel, so that a new r costs no host computation and no upload
 * (with i2i_lora_merge / i2i_merge_group_run it makes r a few bytes of device state: Packer.scale_program).  All operands are packed fp32
 * as i2i_lora_merge takes them: w_* [N][K], a_* [rank_*][K] with lora_alpha/rank folded in, b_* [N][rank_*]; K a multiple of 4.
 *   dst[n][k] = cvt( (1-r) * (w_pre[n][k] + r * sum_j b_pre[n][j] * a_pre[j][k]) + r * (w_cur[n][k] + r * sum_j b_cur[n][j] * a_cur[j][k]) )
 *   bias[n]   = (1-r) * bias_pre[n] + r * bias_cur[n]                         (fp32; bias = NULL: not written)
 * r = rg[0] on the device (rg = NULL means r = 1; rg[1], the skip gamma, is not used).  Either rank may be 0 (its a / b are then ignored).
 * ARITHMETIC (fp32, every step one rounding):  s_x = the FMA chain over j in order, from 0, as in i2i_lora_merge;  p_x = fma(r, s_x, w_x);
 * q = 1 - r, computed once;  dst = cvt(fma(q, p_pre, r * p_cur));  bias = fma(q, bias_pre, r * bias_cur).  So each fp32 element is within
 * (rank_pre + rank_cur + 4) * 2^-24 * (|w_pre| + |w_cur| + sum |b_pre||a_pre| + sum |b_cur||a_cur|) of the exact value, r = 0 with
 * rank_pre = 0 stores cvt(w_pre) and r = 1 with rank_cur = 0 stores cvt(w_cur) bit for bit (r in [0, 1]).
 * Writes dst[0 .. N*K) and bias[0 .. N) only; one launch, no allocation, no synchronisation, graph-capturable. */
typedef struct {
    void* dst; float* bias;
    const float* w_pre; const float* a_pre; const float* b_pre; const float* bias_pre;
    const float* w_cur; const float* a_cur; const float* b_cur; const float* bias_cur;
    int32_t N, K, rank_pre, rank_cur;
    const float* rg;
} i2i_twin_fold_params;

/* Numerical health scan (ABI v14): counts of what left the number format in one activation tensor, accumulated into a 64-byte device
 * record -- the answer to "which stage of a 16-bit forward first produced a NaN / Inf, and how close to the limit were the others?"
 * without a read-back of the tensor, a synchronisation, or debug buffers (the planner places the op right behind the producer, while
 * the pooled buffer is live: ForwardPlan(health=...)).  A pure read of x; nothing but `rec` is written.
 *   VIEW     rows x cols elements of the op's dtype (I2I_F32 / I2I_BF16 / I2I_F16), row r at x + r * ld (ld >= cols, in elements).
 *            Elements [cols, ld) of a row are NOT read, whatever they hold.  x needs the alignment of its element type only.
 *   RECORD   eight uint64, 64-byte aligned, ACCUMULATED by every launch until the owner zeroes them:
 *              [0] runs        +1 per launch
 *              [1] n_nan       exponent all ones, mantissa != 0 (any payload, either sign)
 *              [2] n_pos_inf   [3] n_neg_inf
 *              [4] n_over      finite and |x| > limit (strict; limit is fp32, the comparison is exact)
 *              [5] max_abs     the fp32 bit pattern of the largest finite |x| seen (0 if none; bf16 / fp16 widen exactly, -0 counts as 0),
 *                              updated with an unsigned max: non-negative fp32 patterns order like their values
 *              [6] elements    +rows * cols per launch
 *              [7] reserved    stays 0
 *   Every update is an integer add or an unsigned max: the record is bit-identical for any grid, any workgroup order, and between
 *   the CPU emulator and the GPU (tests/health_ref.py is the CPU oracle of this text).  No float atomics.
 * One launch (capped grid, grid-stride loop, 16-byte loads per lane on the 16-byte aligned part of every row, element loads on the
 * rest), no allocation, no synchronisation, no read-back; graph-capturable.  Partial results are reduced lanes -> wave -> workgroup
 * (LDS) and a workgroup issues at most one agent-scope atomic per NON-ZERO field: a healthy tensor costs one max per workgroup.
 * Errors (I2I_ERR_BAD_ARG): null params / x / rec, limit not > 0 (NaN included), negative sizes, ld < cols, rec not 64-byte aligned,
 * x not aligned to its element, a dtype other than the three float types (I2I_U8 included). */
typedef struct {
    const void* x;
    int64_t rows; int32_t cols; int64_t ld;
    float limit;                       /* "near saturation" threshold, > 0 (the planner's default: half the dtype's largest finite value) */
    uint64_t* rec;                     /* the 8 x uint64 record above */
} i2i_scan_params;

/* ---- ABI 14 addition: mixed-size images in one batch (I2I_OP_RESIZE_U8_RAGGED).  Purely additive like the two above -- one new opcode, two
 * new structs, three new exported functions; no existing struct, opcode number or signature changed and sizeof(i2i_op) did not grow -- so
 * I2I_ABI_VERSION stays 14.  A library built before the addition is recognised by the missing symbol (i2i_resize_u8_ragged), and its plan
 * loader refuses the new opcode as unknown.
 *
 * One separable pass of i2i_resize_u8 over a RAGGED batch: every image has its own extents, its own place in a byte arena and its own tap
 * table, all read from device memory at run time -- the reference's per-request `Resize((512, 512), LANCZOS)` in front of the generator and
 * `output.resize(input size, LANCZOS)` behind it (src/inference_unpaired.py:40,53) for a batch of requests of different sizes, in two
 * launches per direction (axis = 1: win -> nout columns, then axis = 0: hin -> nout rows, Pillow's order) instead of two per image.
 *   IMAGE b  images[b] (48 bytes): the pass's source is dense HWC [hin][win][c] at src + src_off, its result dense HWC at dst + dst_off
 *            ([hin][nout][c] for axis = 1, [nout][win][c] for axis = 0).  hin == 0 or win == 0 is an EMPTY SLOT: nothing of it is read
 *            (not even its other fields) and nothing is written.  bounds[nout][2] = (first tap, tap count) at tables + bounds_off,
 *            coeffs[nout][ksize] at tables + coeffs_off, exactly the arrays i2i_resize_u8 takes (i2i_lanczos_tables below writes them).
 *   ARITHMETIC  i2i_resize_u8's: out = clip8((2^21 + sum_t in[first + t] * k[t]) >> 22) in int32.  Image b of the result is BIT-IDENTICAL to
 *            i2i_resize_u8 on image b alone with the same tables, hence (c = 1, c = 3) to Pillow.  An image that changes along one axis
 *            only still runs both passes: Pillow's same-size table is an exact identity (one tap of weight 2^22 per coordinate).
 *   GRID     a function of n and grid_units ONLY (grid y = image, min(ceil(grid_units / 256), 1024) workgroups of 256 per image in x, each
 *            striding over that image's outputs), so a captured graph stays valid when the host rewrites descriptors, tables and pixels in
 *            place.  grid_units is a capacity hint -- the largest number of output pixels (axis = 1) or output dwords (axis = 0) any image
 *            of any request will have; results do not depend on it (1 is correct, only slow).
 *   SAFETY   Nothing is written outside [dst_off, dst_off + output bytes) of any image; nothing is read outside [0, src_bytes) of the source
 *            arena (the horizontal pass's 8-byte window loads fall back to byte loads at the arena's end) or outside [0, tables_len) of the
 *            pool.  The vertical pass uses dword or byte access per image (win * c % 4), chosen at run time.  Before touching pixels every
 *            workgroup checks its image: offsets non-negative and multiples of 4, source and result inside src_bytes / dst_bytes, both
 *            tables inside tables_len, nout / ksize >= 1, and every bounds row (0 <= first, 0 <= count <= ksize, first + count <= the
 *            source extent along `axis`).  An image that fails is SKIPPED as a whole (its destination bytes stay as they were) and bit
 *            (b & 31) is OR-ed into *bad_mask (if given; the owner zeroes it); the other images are unaffected.  A wrong descriptor or
 *            table entry is a flag, never a fault.  Images must not overlap in dst; src and dst must not overlap.
 * One launch, no allocation, no synchronisation, no read-back; graph-capturable.  n == 0 is a successful no-op.
 * Errors (I2I_ERR_BAD_ARG): null params; c outside 1..4; n < 0; axis not 0 / 1; grid_units < 1; negative src_bytes / dst_bytes / tables_len;
 * (n > 0) src / dst / images / tables null, src / dst / tables / bad_mask not 4-byte aligned, images not 8-byte aligned. */
typedef struct {                       /* device, one per image, 48 bytes */
    int64_t src_off, dst_off;          /* byte offsets into the arenas, multiples of 4 */
    int32_t hin, win;                  /* extent of this pass's source; hin == 0 or win == 0: empty slot */
    int32_t nout, ksize;               /* output extent along `axis`; taps per output coordinate (row length of coeffs) */
    int32_t bounds_off, coeffs_off;    /* int32-element offsets into `tables` */
    int32_t reserved[2];               /* ignored */
} i2i_resize_image;
typedef struct {
    const void* src; void* dst;        /* uint8 arenas, 4-byte aligned */
    int64_t src_bytes, dst_bytes;      /* arena capacities */
    const i2i_resize_image* images;    /* device [n] */
    const int32_t* tables; int64_t tables_len;   /* device int32 pool and its length in elements */
    int32_t n, c, axis;                /* c 1..4, shared by the batch; axis as i2i_resize_u8 */
    int64_t grid_units;                /* capacity hint that sizes the grid ONLY (>= 1) */
    uint32_t* bad_mask;                /* optional device word */
} i2i_resize_u8_ragged_params;

/* ---- ABI 14 addition: per-image health in a batch (I2I_OP_SCAN_BATCH, I2I_OP_SCAN_VERDICT).  Purely additive like the ones above -- two
 * new opcodes, two new structs, two new exported functions; no existing struct, opcode number or signature changed and sizeof(i2i_op) did
 * not grow -- so I2I_ABI_VERSION stays 14.  A library built before the addition is recognised by the missing symbols (i2i_scan_batch,
 * i2i_scan_verdict), and its plan loader refuses the new opcodes as unknown.
 *
 * i2i_scan over the images of a batch-outermost tensor, ONE RECORD PER IMAGE, in one launch: "which request of the batch went non-finite"
 * (nothing in the forward mixes images, so the other requests of the replay are good and the host can say which).
 *   IMAGE b  the rows x cols view (row pitch ld, in elements) at x + b * img_stride elements; img_stride >= (rows - 1) * ld + cols.  Images
 *            may start at any element: every image is split into its own unaligned head, 16-byte chunks and tail from ITS start address.
 *            Nothing outside [0, cols) of a row of an image is read -- not the padding of a row, not the gap between two images.
 *   RECORD b the 8 x uint64 record of i2i_scan_params at rec + b * rec_stride BYTES (rec 64-byte aligned, rec_stride a multiple of 64, >= 64).
 *   CONTRACT after one launch on zeroed records, record b equals BIT FOR BIT what i2i_scan writes for image b's view alone (runs = 1,
 *            elements = rows * cols per image; rows = 0 or cols = 0 counts a run and reads nothing).  The classification is the same device
 *            code; every update is an integer add or an unsigned max, so the records do not depend on the grid or on which load path an
 *            image took, and are identical between the CPU emulator and the GPU.
 * One launch: the grid is (slices of an image) x (images), capped in total; a workgroup works on one image at a time and issues at most one
 * agent-scope atomic per non-zero field and image.  No allocation, no synchronisation, no read-back; graph-capturable.
 * Errors (I2I_ERR_BAD_ARG, the records stay untouched): null params / x / rec; images < 1; negative rows / cols; ld < cols; img_stride smaller
 * than one image's extent (or sizes whose products leave 2^61); limit not > 0 (NaN included); rec not 64-byte aligned; rec_stride < 64 or
 * not a multiple of 64; x not aligned to its element; a dtype other than the three float types. */
typedef struct {
    const void* x;
    int32_t images;                    /* >= 1 */
    int32_t cols;
    int64_t rows, ld;                  /* rows per image; row pitch in elements, >= cols */
    int64_t img_stride;                /* elements between image starts */
    float limit;                       /* as i2i_scan_params.limit */
    uint64_t* rec;                     /* record of image 0 */
    int64_t rec_stride;                /* BYTES between the records of consecutive images */
} i2i_scan_batch_params;

/* The per-image verdict over a table of such records, computed on the device.  Records are TAP-MAJOR: record (t, b) = rec[(t * images + b) * 8
 * .. + 8), t < taps in program order (what a planner gets with rec = table + t * images * 64 and rec_stride = 64 in tap t's
 * i2i_scan_batch_params).  verdict = images rows of four uint32 {first_bad, first_over, runs, bad_runs}.
 *   I2I_VERDICT_CLEAR  zeroes every record of the table.  `verdict` is not touched (it may be NULL).
 *   I2I_VERDICT_JUDGE  one lane per image b:  first_bad = 1 + the smallest t whose record has n_nan | n_pos_inf | n_neg_inf != 0, or 0 if there
 *                      is none;  first_over = the same for n_over;  runs += 1;  bad_runs += (first_bad != 0).  The records are only read.  A
 *                      lane owns its row: plain loads and stores, no atomics.
 * CLEAR as the first op of a program and JUDGE as its last: after any run or graph replay the records describe THAT run in detail and the
 * verdict rows carry the running totals, with nothing staged by the host in between.  The owner zeroes the verdict rows.
 * One launch each; no allocation, no synchronisation, no read-back; graph-capturable.  taps == 0 is valid (JUDGE then only counts the run).
 * Errors (I2I_ERR_BAD_ARG, nothing written): null params / rec; rec not 8-byte aligned; taps < 0 (or taps * images past 2^40); images < 1;
 * an unknown mode; (JUDGE) verdict null or not 4-byte aligned. */
typedef enum { I2I_VERDICT_CLEAR = 0, I2I_VERDICT_JUDGE = 1 } i2i_verdict_mode;
typedef struct {
    uint64_t* rec;                     /* [taps][images][8] */
    int32_t taps, images;
    uint32_t* verdict;                 /* [images][4] = {first_bad, first_over, runs, bad_runs} */
    int32_t mode;                      /* i2i_verdict_mode */
} i2i_scan_verdict_params;

/* ---- ABI 14 addition: automatic per-image Canny thresholds (I2I_OP_CANNY_AUTO_THR).  Purely additive like the ones above -- one new opcode,
 * one new struct, two new exported functions (plus the host-side table functions i2i_resample_*); no existing struct, opcode number or
 * signature changed and sizeof(i2i_op) did not grow -- so I2I_ABI_VERSION stays 14.  A library built before the addition is recognised by
 * the missing symbol (i2i_canny_auto_thr), and its plan loader refuses the new opcode as unknown.
 *
 * The "auto-Canny" median rule, low = (1 - sigma) * median, high = (1 + sigma) * median, computed on the device from the image itself and
 * WRITTEN into the threshold table i2i_canny_u8_batch reads, so that photo -> thresholds -> Canny -> generator is one asynchronous sequence
 * with nothing chosen or staged by the host.  The rule is NOT part of the reference (its scripts take two hand-set numbers, defaults 100 /
 * 200: src/inference_paired.py, gradio_canny2image.py); this comment is its contract and tests/canny_auto_ref.py the CPU oracle of it.
 * sigma = 0.33 is the customary default of the rule, not a tuned value.  Per image b, N = h * w * c bytes, all in integers:
 *   HISTOGRAM  256 bins over ALL bytes of the image, every channel (the np.median(image) form of the rule).
 *   RANKS      a = the order statistic of 0-based rank (N - 1) / 2, b = the one of rank N / 2 (integer divisions);
 *              m2 = a + b = 2 * np.median(image) exactly, 0 .. 510.
 *   THRESHOLDS s = min(sigma_q16[b], 65536):  low = max(0, (m2 * (65536 - s)) >> 17),  high = min(255, (m2 * (65536 + s)) >> 17)
 *              (both products fit in int32).  thr[b] = {low, high}; median2[b] = m2 if median2 is given.
 *   MANUAL     sigma_q16[b] < 0 writes NOTHING for image b -- not thr[b], not median2[b] -- and reads none of its pixels: a request with
 *              hand-set sliders keeps its pair in the same table, one batch mixes automatic and manual requests.
 * Every update on the way is an integer add: the result is bit-identical for any grid and any workgroup order, and between the CPU
 * emulator and the GPU.  No float anywhere.
 * Three launches whose grids depend on n, h, w, c only (clear of ws; histogram: (slices of an image) x (images), capped in total, 256
 * lanes, 16-byte loads on the aligned part of an image and byte loads on its head and tail -- an image may start at ANY byte --, one
 * 256-bin copy per wave in LDS, one agent-scope add per non-zero bin and workgroup; select: one wave per image).  Nothing outside
 * [0, n * N) of src is read.  No allocation, no synchronisation, no read-back; graph-capturable.  `ws` is state of the run in flight (see
 * the CONCURRENCY note of i2i_gn_stats_params).  n == 0 is a successful no-op (checked after the sizes, before the pointers).
 * Errors (I2I_ERR_BAD_ARG, nothing written): null params; c outside 1..4; negative n / h / w; (n > 0) an empty image (h * w == 0), N past
 * 2^31 - 1, src / sigma_q16 / thr / ws null, thr / sigma_q16 / median2 not 4-byte aligned, ws not 16-byte aligned. */
typedef struct {
    const void* src;            /* uint8 [n][h][w][c], c 1..4, any byte alignment of an image start is allowed */
    int32_t n, h, w, c;
    const int32_t* sigma_q16;   /* device int32 [n]: sigma * 65536 per image, 0..65536; NEGATIVE = leave thr[b] untouched (manual sliders) */
    int32_t* thr;               /* device int32 [n][2] = {low, high}: exactly i2i_canny_u8_batch_params.thr */
    uint32_t* median2;          /* optional device uint32 [n]: the doubled median, for the caller's display; NULL = not wanted */
    void* ws;                   /* >= i2i_canny_auto_ws_bytes(n), 16-byte aligned; contents irrelevant before and after */
} i2i_canny_auto_thr_params;

/* ---- ABI 14 addition: device fingerprints (I2I_OP_DIGEST).  Purely additive like the ones above -- one new opcode, one new struct, two new
 * exported functions (i2i_digest, i2i_plan_verify); no existing struct, opcode number or signature changed and sizeof(i2i_op) did not grow -- so
 * I2I_ABI_VERSION stays 14.  A library built before the addition is recognised by the missing symbol (i2i_digest), and its plan loader refuses
 * the new opcode as unknown.
 *
 * A position-sensitive, order-independent digest of a tensor view, computed on the device: "did two runs, two GPUs, two hosts compute the
 * same BITS, and from which stage and which request on did they stop doing so" -- what the health scan cannot say (a finite wrong value: a
 * corrupted weight, a stale pooled buffer, a flipped byte of a plan file).  A pure read of x; nothing but the records is written.
 *   VIEW      as i2i_scan_batch_params: `images` views of rows x cols elements (I2I_U8 / I2I_F16 / I2I_BF16 / I2I_F32 = 1 / 2 / 2 / 4 bytes),
 *             row r of image b at x + b * img_stride + r * ld elements (ld >= cols, img_stride >= (rows - 1) * ld + cols).  Elements
 *             [cols, ld) of a row and the gaps between images are NEVER read.  x needs the alignment of its element type only.
 *   INDEX     element p = row * cols + col of an image (pitch pads do not count) has the logical index j = index0 + p (uint64, wraps mod
 *             2^64); index0 is the same for every image.
 *   RECORD b  four uint64 {s0, s1, elements, reserved} at rec + b * 32 bytes (rec 8-byte aligned).  The op ADDS into it; the owner zeroes
 *             it (or I2I_DIGEST_CLEAR does).  reserved is never written (stays 0).
 *   VALUE     v = the element's bit pattern, zero-extended to 32 bits.  Per element, mod 2^64:
 *               s0 += H0(j, v)     s1 += H1(j, v)     elements += 1
 *   MIXERS    integer only, all arithmetic mod 2^64, >> is a logical shift:
 *               m  = (j * 0x9E3779B97F4A7C15) ^ v
 *               m ^= m >> 33;  m *= 0xFF51AFD7ED558CCD;  m ^= m >> 33;  m *= 0xC4CEB9FE1A85EC53;  m ^= m >> 33;       H0 = m
 *               t  = (H0 ^ (H0 >> 31)) * 0xD6E8FEB86659FD93;  H1 = t ^ (t >> 32)
 *             (H0 is the 64-bit finaliser of MurmurHash3 over the Weyl-stepped index xor the value; H1 is one more multiply / xor-shift
 *             round on H0 -- a bijection of it -- so the pair (sum of H0, sum of H1) is a 128-bit multiset digest of the per-element 64-bit
 *             hashes.)  For a fixed j, v -> H0 and v -> H1 are injective: a change of ONE element always changes the record.  Every bit of
 *             (j, v) flips every bit of (H0, H1) with probability ~1/2 (tests/test_digest_emu.py::test_mixer_avalanche).
 *   FOLLOWS   Every update is an integer add, so the record is INDEPENDENT of the grid, the order the workgroups arrive in, the alignment
 *             of x and the pitch, and is BIT-EQUAL between the CPU emulator and the GPU (tests/digest_ref.py is the oracle of this text).
 *             digest(A || B) = digest(A) + digest(B, index0 = len A), field by field: a buffer can be digested in pieces.
 *             The value is the bit pattern: -0.0 != +0.0, and every NaN payload counts.
 *   SCOPE     This detects ACCIDENTS (bit rot, truncation, stale or mixed-up buffers, nondeterminism).  It is NOT cryptographic: the
 *             mixers are public and invertible, anyone can construct a second tensor with the same record.
 *   KIND      I2I_DIGEST_ADD    the above.  images == 0 or rows * cols == 0 is a successful no-op (nothing written, x / rec not needed).
 *             I2I_DIGEST_CLEAR  zeroes the n_records records (all four words each) from rec on, nothing else -- as I2I_VERDICT_CLEAR does
 *                               for the health records -- so a planned program needs no host fill.  Only rec / n_records are read.
 * ADD is one launch: the grid is (slices of an image) x (images), capped in total, grid-stride loops; 16-byte loads on the 16-byte aligned
 * part of every image (several in flight per lane), element loads on its head and tail; every lane keeps s0 / s1 in 64-bit registers,
 * reduced lanes -> wave -> workgroup (LDS) -> ONE agent-scope add per sum, workgroup and image; `elements` comes from one lane per image.
 * No allocation, no synchronisation, no read-back; graph-capturable.
 * Errors (I2I_ERR_BAD_ARG, nothing written): null params; an unknown kind; rec null or not 8-byte aligned; (CLEAR) n_records < 0 or past
 * 2^40; (ADD) images < 0, negative rows / cols, ld < cols, img_stride smaller than one image's extent (or sizes whose products leave 2^61),
 * x null or not aligned to its element, a dtype outside the four above. */
typedef enum { I2I_DIGEST_ADD = 0, I2I_DIGEST_CLEAR = 1 } i2i_digest_kind;
typedef struct {
    const void* x;
    int32_t images;                    /* >= 0 */
    int32_t cols;
    int64_t rows, ld;                  /* rows per image; row pitch in elements, >= cols */
    int64_t img_stride;                /* elements between image starts */
    uint64_t index0;                   /* logical index of the first element of EVERY image */
    uint64_t* rec;                     /* record of image 0; record b at rec + 4 * b words */
    int32_t kind;                      /* i2i_digest_kind */
    int32_t reserved;
    int64_t n_records;                 /* I2I_DIGEST_CLEAR: records to zero */
} i2i_digest_params;

/* ---- ABI 14 addition: variations, one input image -> V outputs (I2I_OP_REPEAT).  Purely additive like the ones above -- one new opcode, two
 * new structs, one new exported function; no existing struct, opcode number or signature changed and sizeof(i2i_op) did not grow (208 bytes
 * inside the union i2i_igemm_params sizes) -- so I2I_ABI_VERSION stays 14.  A library built before the addition is recognised by the missing
 * symbol (i2i_repeat), and its plan loader refuses the new opcode as unknown.
 *
 * torch.repeat_interleave(x, V, dim = 0) of up to I2I_REPEAT_MAX_SEGMENTS batch-outermost tensors ("segments") in ONE launch: the broadcast
 * from B encoded inputs to B * V generator inputs of ForwardPlan(variations = V) -- the posterior moments and the four encoder skips, which
 * do not depend on the seed (src/pix2pix_turbo.py:197-198: the seed enters at latent_dist.sample()), so the VAE encoder runs once per input
 * ("try different seeds to generate different results", gradio_sketch2image.py) and everything behind this op is the ordinary program at
 * batch B * V.
 *   LAYOUT     segment s is `batch` images of bytes_per_image bytes each, contiguous, at src; dst holds batch * variations such images.
 *              Bytes, not elements: the op does not look at the element type (the op's dtype is ignored), segments of one launch may differ.
 *   ORDER      IMAGE-MAJOR:  dst[(b * variations + v) * n + i] = src[b * n + i]   for b < batch, v < variations, i < n = bytes_per_image:
 *              the variations of input b are the consecutive output slots b * V .. b * V + V - 1.
 *   ALIGNMENT  bytes_per_image is a multiple of 16 and src / dst are 16-byte aligned (NHWC activations with C padded to 8 and the fp32
 *              moments are); bytes_per_image < 2^35.  bytes_per_image == 0 is an empty segment: nothing of it is read or written (src / dst
 *              must still be given).
 *   TABLE      the segments travel BY VALUE inside this struct -- in an i2i_op of a program, a captured graph or a plan file, and from there in
 *              the kernel-argument segment of the launch, which is how the device sees them: no device-side table to allocate, upload or
 *              keep alive, and the plan loader relocates seg[s].src / seg[s].dst like any other pointer field.
 *   READ ONCE  every 16-byte vector of a source is loaded ONCE and stored `variations` times (dwordx4 both ways): the traffic is (1 + V) / V
 *              bytes per output byte, not 2.  src and dst must not overlap; segments must not overlap in dst.
 * One launch: a 1-D grid over the 16-byte vectors of all segments together, 1024 vectors per workgroup; a workgroup finds its segment from a
 * prefix array of workgroup counts by blockIdx alone (wave-uniform, as i2i_merge_group_run does).  All offsets are 64-bit (64 images of a
 * 128-channel 512 x 512 skip are 4 GiB).  No LDS, no atomics, no allocation, no synchronisation; graph-capturable; runs on the caller's stream.
 * batch == 0 or n_segments == 0 is a successful no-op.
 * Errors (I2I_ERR_BAD_ARG, nothing written; the message names the field): null params; variations < 1; batch < 0; n_segments outside
 * 0 .. I2I_REPEAT_MAX_SEGMENTS; a segment's bytes_per_image negative, not a multiple of 16 or >= 2^35; its src or dst null or not 16-byte
 * aligned; sizes whose product leaves 2^61 or a grid past 2^31 - 1 workgroups. */
#define I2I_REPEAT_MAX_SEGMENTS 8
typedef struct {
    const void* src;                   /* [batch][bytes_per_image] */
    void* dst;                         /* [batch * variations][bytes_per_image] */
    int64_t bytes_per_image;           /* multiple of 16 */
} i2i_repeat_segment;
typedef struct {
    int32_t batch, variations;         /* B >= 0, V >= 1 */
    int32_t n_segments;                /* 0 .. I2I_REPEAT_MAX_SEGMENTS */
    int32_t reserved;                  /* ignored */
    i2i_repeat_segment seg[I2I_REPEAT_MAX_SEGMENTS];      /* entries from n_segments on are ignored (keep them zero in a plan file) */
} i2i_repeat_params;

/* ---- ABI 14 addition: tiled forward at native resolution (I2I_OP_TILE_CUT, I2I_OP_TILE_BLEND_U8).  Purely additive like the ones above -- two
 * new opcodes, three new structs, three new exported functions; no existing struct, opcode number or signature changed and sizeof(i2i_op)
 * did not grow -- so I2I_ABI_VERSION stays 14.  A library built before the addition is recognised by the missing symbols (i2i_tile_cut,
 * i2i_tile_blend_u8, i2i_tile_positions), and its plan loader refuses the new opcodes as unknown.
 *
 * A request larger than the model size is cut into overlapping tiles of the model size, the tiles run through the ordinary forward as one
 * batch, and the tile outputs are blended back with a linear feather.  Tiling is NOT part of the reference (its scripts resize the request
 * to the model size, src/inference_unpaired.py:40,53); it sits where variations= and the automatic Canny thresholds sit.
 *
 * THE LAYOUT RULE (i2i_tile_positions, one axis of length L, tile extent t, overlap ov):
 *   conditions  t > 0, t % 8 == 0, ov % 8 == 0, 0 <= ov <= t / 2, L >= t
 *   stride      s = t - ov;  count n = 1 + ceil((L - t) / s);  positions x_k = min(k * s, L - t), k = 0 .. n - 1
 * The first tile starts at 0, the last ends at L, positions increase strictly, neighbours overlap by at least ov, every position but the
 * last is a multiple of 8, every pixel is covered by 1 .. 3 tiles per axis, and x_k / 8 + t / 8 <= ceil(L / 8) (integer division): the
 * crop of a [ceil(L / 8)] latent-resolution field at x_k / 8 stays inside it.  1280, 512, 64 -> {0, 448, 768};  34, 16, 8 -> {0, 8, 16, 18}.
 * The tiles of a request are numbered row-major (ky outer, kx inner); the tiles of request b follow those of request b - 1.
 * i2i_tile_positions: plain host code, no GPU.  Returns n and writes n positions to `out`; out == NULL only counts.  I2I_ERR_BAD_ARG
 * (nothing written) for arguments outside the conditions or capacity < n.  Bit-equal to image_ops.tile_positions.
 *
 * REQUEST b  reqs[b] (i2i_tile_request, 48 bytes, device memory), shared by both ops: the request's pixels are dense
 *            [planes][h][w] pixels of px_bytes bytes at arena + off (uint8 HWC images: planes = 1, px_bytes = c; fp32 planar fields:
 *            px_bytes = 4), its nx * ny tiles occupy the tile slots tile0 .. tile0 + nx * ny - 1 (slot tile0 + ky * nx + kx has its origin at
 *            (ys[ky], xs[kx])), xs[nx] at pos + xs_off and ys[ny] at pos + ys_off.  h == 0 or w == 0 is an EMPTY SLOT: nothing else of it is
 *            read, nothing is written.
 * GRID       a function of n and grid_units ONLY (grid y = request, min(ceil(grid_units / 1024), 1024) workgroups of 256 per request in x,
 *            each striding over the request's rows), so a captured graph stays valid when the host rewrites descriptors, positions and
 *            pixels in place.  grid_units is a capacity hint -- the largest number of tile-batch dwords (cut) / image bytes (blend) any
 *            request will have; results do not depend on it (1 is correct, only slow).
 * SAFETY     Before touching a pixel every workgroup checks its request: h, w, nx, ny positive; off non-negative, a multiple of 4 and the
 *            request's planes * h * w * px_bytes bytes inside arena_bytes; xs_off / ys_off non-negative with nx / ny elements inside
 *            pos_len; tile0 >= 0 and tile0 + nx * ny <= tiles_capacity; every position 0 <= x and x + tw <= w (0 <= y, y + th <= h).
 *            i2i_tile_blend_u8 also wants the positions of an axis strictly increasing with xs[k + 3] >= xs[k] + tw (at most 3 tiles over a
 *            pixel per axis, 9 in 2-D: what the layout rule gives).  A request that fails is SKIPPED as a whole (its destination bytes
 *            stay as they were) and bit (b & 31) is OR-ed into *bad_mask (if given; the owner zeroes it); the other requests are
 *            unaffected.  A wrong descriptor is a flag, never a fault.  Requests must not share tile slots; the arena and the tile batch must
 *            not overlap.
 *
 * i2i_tile_cut: tiles[slot][planes][th][tw] = the request's [planes][y0 .. y0 + th)[x0 .. x0 + tw), ONE launch for every tile of every
 * request: pure byte movement, bit-equal to slicing.  Dword stores (and dword loads: one where the source is aligned, the enclosing aligned
 * pair where it is not, bytes at the arena's last dword) when tw * px_bytes is a multiple of 4, byte access otherwise, chosen at run time.
 * The noise rule of a tiled forward is this op on fp32 fields: a request draws ONE field [lat][ceil(h / 8)][ceil(w / 8)] and the eps of the
 * tile at (y0, x0) is its crop at (y0 / 8, x0 / 8) -- descriptors with extents ceil(. / 8), positions / 8 and a tile of (tw / 8, th / 8).
 *
 * i2i_tile_blend_u8: the inverse.  tiles[slot][th][tw][c] uint8 -> every request's [h][w][c] at arena + off, GATHER form: one thread owns
 * output bytes and sums over the tiles that cover them -- no atomics, the result does not depend on grid or scheduling.  INTEGER CONTRACT:
 *   weight of tile pixel (i, j):  w = wx(i) * wy(j),  wx(i) = min(i + 1, tw - i, ramp),  wy(j) = min(j + 1, th - j, ramp),  1 <= ramp <= 256
 *   over the covering tiles:      num = sum w * u8,  den = sum w;   out = (2 * num + den) / (2 * den)   (integer division: rounds half up)
 * A weight is never zero, so image borders and the wider overlap of a last tile come out right by the normalisation alone; ramp = 1 is the
 * plain average of the covering tiles, overlap 0 a plain paste; blend(cut(img)) == img.  The accumulators are uint32: at most 9 covering
 * tiles (the check above) of weight <= ramp^2 <= 2^16 give 2 * num + den <= 9 * 2^16 * 511 < 2^32.  A pixel that NO tile covers is written
 * as 0 and its request's bit is set in *bad_mask (the request is still written; the layout rule never produces one).
 * Both: one launch, no allocation, no synchronisation, no read-back; graph-capturable.  n == 0 is a successful no-op.
 * Errors (I2I_ERR_BAD_ARG, the message names the field): null params; n < 0; planes < 1; px_bytes / c outside 1..4; tw / th < 1;
 * tiles_capacity < 0; ramp outside 1..256; grid_units < 1; negative arena_bytes / pos_len; (n > 0) arena / tiles / reqs / pos null, arena /
 * tiles / pos / bad_mask not 4-byte aligned, reqs not 8-byte aligned. */
typedef struct {                       /* device, one per request, 48 bytes */
    int64_t off;                       /* byte offset of the request's pixels in the arena, a multiple of 4 */
    int32_t h, w;                      /* extent in pixels; h == 0 or w == 0: empty slot */
    int32_t tile0;                     /* first tile slot of the request */
    int32_t nx, ny;                    /* tiles per row / per column */
    int32_t xs_off, ys_off;            /* int32-element offsets into `pos` */
    int32_t reserved[3];               /* ignored */
} i2i_tile_request;
typedef struct {
    const void* src; void* dst;        /* the request arena; the tile batch [tiles_capacity][planes][th][tw] pixels; both 4-byte aligned */
    int64_t arena_bytes;               /* capacity of src */
    const i2i_tile_request* reqs;      /* device [n] */
    const int32_t* pos; int64_t pos_len;   /* device int32 pool of positions and its length in elements */
    int32_t n, planes, px_bytes;       /* px_bytes 1..4 */
    int32_t tw, th;                    /* tile extent in pixels */
    int32_t tiles_capacity;            /* tile slots dst holds */
    int64_t grid_units;                /* capacity hint that sizes the grid ONLY (>= 1) */
    uint32_t* bad_mask;                /* optional device word */
} i2i_tile_cut_params;
typedef struct {
    const void* tiles; void* dst;      /* the tile batch [tiles_capacity][th][tw][c] uint8; the request arena; both 4-byte aligned */
    int64_t arena_bytes;               /* capacity of dst */
    const i2i_tile_request* reqs;      /* device [n]: the descriptors of the cut with planes = 1, px_bytes = c */
    const int32_t* pos; int64_t pos_len;
    int32_t n, c, ramp;                /* c 1..4; ramp 1..256 (the model classes pass max(overlap, 1)) */
    int32_t tw, th;
    int32_t tiles_capacity;
    int64_t grid_units;
    uint32_t* bad_mask;
} i2i_tile_blend_u8_params;

/* ---- ABI 14 addition: baseline JPEG encoding of a ragged uint8 batch on the device (i2i_jpeg_encode_u8, i2i_jpeg_workspace_bytes,
 * i2i_jpeg_header).  Purely additive -- two new structs, three new exported functions, NO opcode (the entry is an eager call on the
 * caller's stream, graph-capturable; plan files do not carry it) and i2i_op is untouched -- so I2I_ABI_VERSION stays 14.  A library built
 * before the addition is recognised by the missing symbols.
 *
 * The last host line of the reference's scripts is output_pil.save(...) (src/inference_paired.py:75, src/inference_unpaired.py:58).  This
 * entry writes, per image, the COMPLETE FILE Pillow with libjpeg-turbo writes for Image.save(f, "JPEG", quality=q, subsampling=s), byte
 * for byte (tests/jpeg_ref.py is the integer restatement the tests pin against the installed Pillow).  THE RULES, all integer:
 *   header    623 bytes: SOI, APP0 JFIF 1.01 (units 0, density 1 x 1, no thumbnail), DQT 0, DQT 1 (8-bit, zigzag order), SOF0 (precision 8,
 *             h, w, components 1, 2, 3 with sampling 0x22 (4:2:0) or 0x11 (4:4:4) for Y and 0x11 for Cb, Cr, tables 0, 1, 1), DHT DC0, AC0,
 *             DC1, AC1 (the typical tables of ITU-T T.81 Annex K.3), SOS (three components, selectors 0x00, 0x11, 0x11, Ss 0, Se 63, 0).
 *   tables    Annex K.1 scaled by s = 5000 / q (q < 50) or 200 - 2 q, entry (t * s + 50) / 100 clamped to 1 .. 255; q clamped to 1 .. 100.
 *   colour    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16;  Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   padding   columns replicate the last input column, rows of Y (and of 4:4:4 chroma) the last input row; for 4:2:0 the input is padded to
 *             an even height, downsampled as (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, .. along a row, and the DOWNSAMPLED plane's last
 *             row is replicated.
 *   DCT       libjpeg's jfdctint ("islow", CONST_BITS 13, PASS1_BITS 2) on samples - 128, rows then columns.
 *   quantise  d = 8 * table entry;  (|c| + (d >> 1)) / d with the sign restored.
 *   scan      one interleaved scan, MCU = Y Cb Cr (4:4:4) or Y00 Y01 Y10 Y11 Cb Cr (4:2:0).  A Y block of a 4:2:0 MCU beyond ceil(w / 8)
 *             columns or ceil(h / 8) rows is a DUMMY block: no AC coefficients, the DC of the block before it in the MCU.  DC differences
 *             per component, ZRL per 16 zeros, EOB when a block ends in zeros, bits packed MSB first, the last byte padded with 1-bits, 0x00
 *             stuffed after every 0xFF byte of the scan, then EOI.
 * IMAGE b    images[b] (i2i_jpeg_image, 48 bytes, DEVICE memory): dense [h][w][c] uint8 pixels at src + src_off, c = 3 (RGB) or 1 (grey,
 *            replicated into the three channels as convert("RGB") does).  The file goes to dst + dst_off (any alignment), at most `capacity`
 *            bytes; length[b] receives its size.  Sizes, quality and subsampling are DEVICE STATE: a captured graph serves every quality
 *            and every set of sizes whose blocks fit max_blocks.
 * GRID       a function of n and max_blocks only.  max_blocks is the capacity hint: the largest number of 8 x 8 blocks in scan order (dummy
 *            blocks included: 3 * ceil(w / 8) * ceil(h / 8) for 4:4:4, 6 * ceil(w / 16) * ceil(h / 16) for 4:2:0) any image will have.  It
 *            sizes the grids and the per-image slot of the workspace (i2i_jpeg_workspace_bytes(n, max_blocks)); results do not depend on it.
 * SAFETY     Every workgroup of every stage checks its image before it touches a pixel: h, w in 1 .. 65535, c 1 or 3, subsampling 0 or 2,
 *            the pixels inside src_bytes, the slot inside dst_bytes, the block count <= max_blocks.  The last stage also checks that the file
 *            fits `capacity`.  An image that fails gets length 0, NOTHING of its slot (or outside it) is written and bit (b & 31) is OR-ed into
 *            *bad_mask (if given; the owner zeroes it); the other images are unaffected.  A flagged image is a result, never a fault.
 * STAGES     five launches whatever the batch holds, no read-back, no host decision, no kernel waits on another workgroup: (1) colour, padding,
 *            downsample, DCT, quantisation -> int16 coefficients in zigzag order at the block's index in scan order, and the bit buffer
 *            zeroed; (2) each block's code length and the prefix sum inside chunks of 256 blocks; (3) the chunk sums reduced per workgroup (the
 *            second level, behind a launch boundary), every block's bits OR-ed in at its bit offset; (4) 0xFF bytes per 1024-byte chunk of
 *            the packed stream; (5) header from a template, stuffed scan, EOI, length.
 * Errors (I2I_ERR_BAD_ARG): null params; n < 0; max_blocks outside 1 .. 2^21; negative src_bytes / dst_bytes; (n > 0) src / dst / images /
 * length / ws null, src / length / bad_mask not 4-byte aligned, images not 8-byte aligned, ws not 16-byte aligned, ws_bytes too small. */
typedef struct {                       /* device, one per image, 48 bytes */
    int64_t src_off;                   /* byte offset of the image's pixels in the arena */
    int64_t dst_off;                   /* byte offset of the image's file in the output pool */
    int32_t h, w;                      /* 1 .. 65535 */
    int32_t c;                         /* channels of the source: 3, or 1 (replicated) */
    int32_t quality;                   /* clamped to 1 .. 100 */
    int32_t subsampling;               /* Pillow's numbers: 0 = 4:4:4, 2 = 4:2:0 */
    int32_t capacity;                  /* bytes of the slot at dst_off */
    int32_t reserved[2];               /* ignored */
} i2i_jpeg_image;
typedef struct {
    const void* src; int64_t src_bytes;    /* the pixel arena (4-byte aligned) and its capacity */
    void* dst; int64_t dst_bytes;          /* the output pool and its capacity */
    const i2i_jpeg_image* images;      /* device [n] */
    uint32_t* length;                  /* device [n]: bytes of every file (0: flagged) */
    uint32_t* bad_mask;                /* optional device word */
    void* ws; int64_t ws_bytes;        /* >= i2i_jpeg_workspace_bytes(n, max_blocks), 16-byte aligned; scratch, needs no initialisation */
    int32_t n;
    int32_t reserved;                  /* ignored */
    int64_t max_blocks;                /* capacity hint, 1 .. 2^21 */
} i2i_jpeg_encode_u8_params;
#define I2I_JPEG_HEADER_BYTES 623

/* ---- ABI 14 addition: PNG encoding of a ragged uint8 batch on the device (i2i_png_encode_u8, i2i_png_workspace_bytes, i2i_png_bound).
 * Purely additive like the JPEG entry -- two new structs, three new exported functions, NO opcode, i2i_op untouched, I2I_ABI_VERSION stays
 * 14; plan files do not carry it.  A library built before the addition is recognised by the missing symbols.
 *
 * What output_pil.save(...) writes when the name ends in .png (src/inference_paired.py:75, src/inference_unpaired.py:58), and with
 * flags bit 0 the script's canny_viz_inv.save(..._canny.png) (src/inference_paired.py:48-49).  PNG is lossless and the compressed bytes are
 * not Pillow's: the CONTAINER and the FILTERED SCANLINE STREAM are Pillow's, the DEFLATE STREAM is this project's own and fully specified
 * here (tests/png_ref.py is the integer restatement; device == oracle on whole files).  THE RULES, all integer:
 *   container the 8-byte signature; IHDR (w, h, bit depth 8, colour type 2 for c = 3 or 0 for c = 1, 0, 0, 0); ONE IDAT; IEND; no other
 *             chunk; a CRC-32 on every chunk.  IDAT holds 78 9C, the deflate stream and the big-endian Adler-32 of the filtered stream.
 *   filter    Pillow's adaptive rule (ZipEncode.c, ZIP_PNG, no optimize), per row: bpp = c, the row above row 0 is zeros,
 *             cost = sum over the filtered bytes of (v < 128 ? v : 256 - v).  Start with filter 0 (None); while the best cost is > 0 try
 *             2 (Up), 1 (Sub), 4 (Paeth) in this order and take one only if its cost is STRICTLY smaller.  3 (Average) is never used.
 *             Paeth: p = a + b - c; a if pa <= pb && pa <= pc, else b if pb <= pc, else c.  The filtered stream F is h rows of
 *             S = 1 + w c bytes (the filter type, then the row).  flags bit 0: every pixel is 255 - x before filtering.
 *   blocks    F is cut every I2I_PNG_BLOCK_BYTES = 16384 bytes; every piece is one deflate block with BTYPE = 2 and its own codes; BFINAL
 *             on the last; zero bits up to the byte boundary behind it.  No stored block, no fixed block.
 *   matches   position p looks at the distances 1, c, S, S - c, S + c in this order.  A distance > 32768 or > p is dropped.  The match
 *             length is the number of k with F[p + k] == F[p + k - d] from k = 0 on, at most 258 and clipped at the end of p's block (the
 *             source may lie in the block before).  The longest wins, ties go to the first candidate; under 3 the position is a literal.
 *             The tokens are the greedy parse from the block's first byte: next = p + max(1, length).
 *   lengths   for the literal/length alphabet (286 symbols, end-of-block always counted once; limit 15), the distance alphabet (30; limit
 *             15) and the code-length alphabet (19; limit 7): the used symbols sorted ascending by (frequency, symbol); no used symbol: all
 *             lengths 0 (a block without a match sends HDIST = 0 and one distance length of 0); one used symbol: length 1.  Otherwise
 *             Huffman's merge over two queues (the sorted leaves, the internal nodes in the order they were made; of two equal weights the
 *             leaf is taken first; each step takes two and appends their sum); the leaves' depths clipped at the limit and counted per
 *             length; REPAIR while the Kraft sum exceeds 1, once per 2^-limit of excess: the largest length l < limit with a leaf loses one
 *             leaf, l + 1 gains two, the limit row loses one; then the lengths are dealt by the sorted order, the longest to the rarest.
 *   codes     canonical (RFC 1951 3.2.2).
 *   header    HLIT = n_lit - 257 and HDIST = n_dist - 1 with trailing zero lengths cut (n_lit >= 257, n_dist >= 1); the n_lit + n_dist
 *             lengths are ONE sequence, run-length coded greedily: a run of zeros emits 18 (11 .. 138) while >= 11 remain, then 17 (3 .. 10)
 *             if >= 3 remain, then single zeros; a run of v > 0 emits v, then 16 (3 .. 6) while >= 3 remain, then single v.  HCLEN cuts
 *             trailing zeros of the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, at least 4.
 *   bits      LSB first; Huffman codes bit-reversed, extra bits as they are.
 * IMAGE b    images[b] (i2i_png_image, 48 bytes, DEVICE memory): dense [h][w][c] uint8 pixels at src + src_off, c = 3 (RGB) or 1 (grey).
 *            The file goes to dst + dst_off (any alignment), at most `capacity` bytes (i2i_png_bound(w, h, c) always suffices); length[b]
 *            receives its size.  Sizes and flags are DEVICE STATE: one captured graph serves every set of sizes under the hint.
 * GRID       a function of n and max_bytes only.  max_bytes, 1 .. 2^27, is the capacity hint: the largest h (1 + w c) any image will
 *            have.  It sizes the grids and the per-image slot of the workspace (i2i_png_workspace_bytes); results do not depend on it.
 * SAFETY     as for i2i_jpeg_image: every workgroup of every stage checks its image before it touches a pixel (h, w in 1 .. 65535, c 1 or
 *            3, the pixels inside src_bytes, the slot inside dst_bytes, h (1 + w c) <= max_bytes); the last stage also checks that the file
 *            fits `capacity`.  An image that fails gets length 0, NOTHING of its slot is written and bit (b & 31) is OR-ed into *bad_mask
 *            (if given; the owner zeroes it); the other images are unaffected.  A flagged image is a result, never a fault.
 * STAGES     SIX launches whatever the batch holds, no read-back, nothing allocated, no kernel waits on another workgroup: (1) filter rows
 *            -> F, bit buffer zeroed; (2) the longest candidate match of every position; (3) per deflate block: greedy parse, histograms,
 *            code lengths, codes, block header, bit offsets of its 256 segments; (4) bits in front of the block reduced per workgroup
 *            (behind the launch boundary), tokens packed at their offsets; (5) Adler-32 and CRC-32 terms per 1024 bytes, each carried to
 *            the end of its stream (Adler: A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1) mod 65521; CRC: times x^(8 len) mod the
 *            polynomial); (6) the file and length[b].
 * Errors (I2I_ERR_BAD_ARG): null params; n < 0; max_bytes outside 1 .. 2^27; negative src_bytes / dst_bytes; (n > 0) src / dst / images /
 * length / ws null, length / bad_mask not 4-byte aligned, images not 8-byte aligned, ws not 16-byte aligned, ws_bytes too small. */
typedef struct {                       /* device, one per image, 48 bytes */
    int64_t src_off;                   /* byte offset of the image's pixels in the arena */
    int64_t dst_off;                   /* byte offset of the image's file in the output pool */
    int32_t h, w;                      /* 1 .. 65535 */
    int32_t c;                         /* 3 (RGB, colour type 2) or 1 (grey, colour type 0) */
    int32_t flags;                     /* bit 0: invert (255 - x) before filtering; other bits ignored */
    int32_t capacity;                  /* bytes of the slot at dst_off */
    int32_t reserved[3];               /* ignored */
} i2i_png_image;
typedef struct {
    const void* src; int64_t src_bytes;    /* the pixel arena and its capacity */
    void* dst; int64_t dst_bytes;          /* the output pool and its capacity */
    const i2i_png_image* images;       /* device [n] */
    uint32_t* length;                  /* device [n]: bytes of every file (0: flagged) */
    uint32_t* bad_mask;                /* optional device word */
    void* ws; int64_t ws_bytes;        /* >= i2i_png_workspace_bytes(n, max_bytes), 16-byte aligned; scratch, needs no initialisation */
    int32_t n;
    int32_t reserved;                  /* ignored */
    int64_t max_bytes;                 /* capacity hint, 1 .. 2^27 */
} i2i_png_encode_u8_params;
#define I2I_PNG_BLOCK_BYTES 16384

typedef struct { int32_t unused; } i2i_nop_params;

typedef struct {
    int32_t opcode;    /* i2i_opcode */
    int32_t dtype;     /* i2i_dtype */
    union {
        i2i_igemm_params igemm;
        i2i_gn_stats_params gn_stats;
        i2i_gn_apply_params gn_apply;
        i2i_layernorm_params layernorm;
        i2i_softmax_params softmax;
        i2i_attention_params attention;
        i2i_nchw_to_nhwc_params to_nhwc;
        i2i_nhwc_to_nchw_params to_nchw;
        i2i_posterior_params posterior;
        i2i_ddpm_params ddpm;
        i2i_embed_params embed;
        i2i_lora_merge_params lora_merge;
        i2i_resize_u8_params resize_u8;
        i2i_nop_params nop;
        i2i_canny_u8_params canny_u8;
        i2i_randn_params randn;
        i2i_twin_fold_params twin_fold;
        i2i_scan_params scan;
        i2i_randn_batch_params randn_batch;
        i2i_canny_u8_batch_params canny_u8_batch;
        i2i_resize_u8_ragged_params resize_u8_ragged;
        i2i_scan_batch_params scan_batch;
        i2i_scan_verdict_params scan_verdict;
        i2i_canny_auto_thr_params canny_auto_thr;
        i2i_digest_params digest;
        i2i_repeat_params repeat;
        i2i_tile_cut_params tile_cut;
        i2i_tile_blend_u8_params tile_blend_u8;
    } u;
} i2i_op;

/* ---- library ---- */
int i2i_abi_version(void);
const char* i2i_backend(void);            /* "gfx950" (product) */
const char* i2i_last_error(void);
size_t i2i_sizeof_op(void);               /* sanity check for FFI struct layout */

/* ---- single-op entry points (each = one or two kernel launches on `stream`) ---- */
int i2i_igemm(const i2i_igemm_params* p, int dtype, void* stream);
/* Number of partial-sum slots per image this op would write through gn_part (its spatial tile count), or 0 if
 * the kernel that will run it cannot produce GroupNorm partials (planner query; launches nothing). */
int i2i_igemm_gn_parts(const i2i_igemm_params* p, int dtype, int groups);
/* Name of the kernel family i2i_igemm() routes this op to ("conv3x3_w32_kernel", "conv3x3_w32_kernel<SUBPIX>",
 * "conv3x3_halo_kernel", "conv3x3_halo_kernel<SUBPIX>", "gemm_w32_kernel", "conv_narrow_kernel", "igemm_dma_kernel", "igemm_kernel"): reporting only (bench.py groups its per-op
 * timings by it; the planner does not have to mirror the routing rules).  Launches nothing; never NULL. */
const char* i2i_igemm_route(const i2i_igemm_params* p, int dtype);
int i2i_gn_stats(const i2i_gn_stats_params* p, int dtype, void* stream);
int i2i_gn_apply(const i2i_gn_apply_params* p, int dtype, void* stream);
int i2i_layernorm(const i2i_layernorm_params* p, int dtype, void* stream);
int i2i_softmax(const i2i_softmax_params* p, int dtype, void* stream);
int i2i_attention(const i2i_attention_params* p, int dtype, void* stream);
int i2i_nchw_to_nhwc(const i2i_nchw_to_nhwc_params* p, int dtype, void* stream);
int i2i_nhwc_to_nchw(const i2i_nhwc_to_nchw_params* p, int dtype, void* stream);
int i2i_posterior(const i2i_posterior_params* p, int dtype, void* stream);
int i2i_ddpm_postquant(const i2i_ddpm_params* p, int dtype, void* stream);
int i2i_embed(const i2i_embed_params* p, int dtype, void* stream);
int i2i_lora_merge(const i2i_lora_merge_params* p, int dtype, void* stream);
int i2i_resize_u8(const i2i_resize_u8_params* p, int dtype, void* stream);   /* dtype ignored (uint8 data) */
int i2i_canny_u8(const i2i_canny_u8_params* p, int dtype, void* stream);     /* dtype ignored (uint8 data); five launches */
size_t i2i_canny_ws_bytes(int n, int h, int w);                              /* bytes of i2i_canny_u8_params.ws (0 for a non-positive size) */
int i2i_randn(const i2i_randn_params* p, int dtype, void* stream);           /* dtype ignored (fp32 / uint32 data); one launch */
int i2i_twin_fold(const i2i_twin_fold_params* p, int dtype, void* stream);   /* one launch */
int i2i_scan(const i2i_scan_params* p, int dtype, void* stream);             /* one launch; dtype = element type of x */
/* ABI 14 additions (per-image request parameters; the version number did not move: see i2i_randn_batch_params) */
int i2i_randn_batch(const i2i_randn_batch_params* p, int dtype, void* stream);         /* dtype ignored; one launch */
int i2i_canny_u8_batch(const i2i_canny_u8_batch_params* p, int dtype, void* stream);   /* dtype ignored; five launches */
int i2i_resize_u8_ragged(const i2i_resize_u8_ragged_params* p, int dtype, void* stream);   /* dtype ignored; one launch */
int i2i_scan_batch(const i2i_scan_batch_params* p, int dtype, void* stream);           /* one launch; dtype = element type of x */
int i2i_scan_verdict(const i2i_scan_verdict_params* p, int dtype, void* stream);       /* dtype ignored; one launch */
int i2i_canny_auto_thr(const i2i_canny_auto_thr_params* p, int dtype, void* stream);   /* dtype ignored (uint8 data); three launches */
size_t i2i_canny_auto_ws_bytes(int n);                                                 /* bytes of i2i_canny_auto_thr_params.ws (0 for n < 1) */
int i2i_digest(const i2i_digest_params* p, int dtype, void* stream);                   /* one launch; dtype = element type of x (I2I_U8 allowed) */
int i2i_repeat(const i2i_repeat_params* p, int dtype, void* stream);                   /* dtype ignored (bytes); one launch */
int i2i_tile_cut(const i2i_tile_cut_params* p, int dtype, void* stream);               /* dtype ignored (bytes); one launch */
int i2i_tile_blend_u8(const i2i_tile_blend_u8_params* p, int dtype, void* stream);     /* dtype ignored (uint8 data); one launch */
/* The tile positions of one axis (the layout rule above i2i_tile_request): host code, returns the count or I2I_ERR_BAD_ARG. */
int i2i_tile_positions(int L, int t, int ov, int32_t* out, int capacity);
/* Baseline JPEG files of a ragged uint8 batch, byte-identical to Pillow's (the contract is the comment of i2i_jpeg_image); five launches. */
int i2i_jpeg_encode_u8(const i2i_jpeg_encode_u8_params* p, int dtype, void* stream);   /* dtype ignored (uint8 data) */
/* Bytes of the workspace for n images of at most max_blocks blocks each: host code; 0 for arguments outside the contract. */
size_t i2i_jpeg_workspace_bytes(int n, int64_t max_blocks);
/* The I2I_JPEG_HEADER_BYTES bytes the device writes in front of the scan, for hosts that are not Python: host code, no GPU.  subsampling 0 or
 * 2, w and h in 1 .. 65535; returns the byte count or I2I_ERR_BAD_ARG (nothing written). */
int i2i_jpeg_header(int quality, int subsampling, int w, int h, uint8_t* out);
/* PNG files of a ragged uint8 batch: Pillow's container and filtered stream, this project's deflate stream (the contract is the comment of
 * i2i_png_image); six launches. */
int i2i_png_encode_u8(const i2i_png_encode_u8_params* p, int dtype, void* stream);     /* dtype ignored (uint8 data) */
/* Bytes of the workspace for n images of at most max_bytes filtered bytes each: host code; 0 for arguments outside the contract. */
size_t i2i_png_workspace_bytes(int n, int64_t max_bytes);
/* A file size the contract can never exceed: host code.  A literal costs at most 15 bits for one byte of F and a match at most
 * 15 + 5 + 15 + 13 = 48 bits for at least three, so 16 bits per byte; a block adds 3 + 14 + 19 * 3 header bits, at most 7 bits per code
 * length (a run symbol with its extra bits spends at most 14 bits on at least 3 lengths) for 286 + 30 lengths and 15 bits of end-of-block,
 * 2301 bits.  With N = h (1 + w c) and K = ceil(N / 16384): 43 + ceil(2301 K / 8) + 2 N + 20.  I2I_ERR_BAD_ARG for w, h outside
 * 1 .. 65535 or c not 1 or 3. */
int64_t i2i_png_bound(int w, int h, int c);
/* Pillow's LANCZOS tap tables for one axis, for hosts that are not Python: plain host code, no GPU, no allocation kept.  They restate
 * precompute_coeffs / normalize_coeffs_8bpc (src/libImaging/Resample.c) in double precision and are bit-equal to image_ops.lanczos_coeffs.
 * i2i_lanczos_ksize: taps per output coordinate, 2 * ceil(3 * max(in / out, 1)) + 1, or I2I_ERR_BAD_ARG for a size < 1.
 * i2i_lanczos_tables: bounds[out][2] = (first tap, tap count) and coeffs[out][ksize_capacity] (22-bit fixed-point weights, zero behind the
 * count; ksize_capacity >= ksize is the row length, i.e. the `ksize` to put into i2i_resize_u8_params / i2i_resize_image).  Returns ksize,
 * or I2I_ERR_BAD_ARG (null pointer, size < 1, ksize_capacity too small) with nothing written. */
int i2i_lanczos_ksize(int in_size, int out_size);
int i2i_lanczos_tables(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize_capacity);
/* The same two functions for any of Pillow's filters the resize kernels are fed with (the kernels take their taps from the tables and do not
 * care which filter made them): I2I_FILTER_LANCZOS (support 3; what i2i_lanczos_* compute, bit for bit) and I2I_FILTER_BICUBIC (Pillow's
 * bicubic_filter, a = -0.5, support 2: the DEFAULT of Image.resize for 8-bit images, i.e. gradio_canny2image.py:16's `input_image.resize((w8,
 * h8))` with no filter argument).  Normalisation and the 22-bit rounding are the same; ksize = 2 * ceil(support * max(in / out, 1)) + 1.
 * Bit-equal to image_ops.resample_coeffs(in, out, "lanczos" | "bicubic").  An unknown filter is I2I_ERR_BAD_ARG. */
typedef enum { I2I_FILTER_LANCZOS = 0, I2I_FILTER_BICUBIC = 1 } i2i_resample_filter;
int i2i_resample_ksize(int filter, int in_size, int out_size);
int i2i_resample_tables(int filter, int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize_capacity);

/* ---- grouped LoRA re-merge (ABI v13): every adapted layer of a network in ONE launch.  `create` checks the n layers as i2i_lora_merge
 * would (an error names the layer index) and uploads them as a device table with an int32 prefix array of tile counts (synchronous: setup,
 * not the latency path); `run` is a single launch of a 1-D grid over all tiles -- a workgroup finds its layer by binary search in the
 * prefix and runs the per-element arithmetic of i2i_lora_merge (the same device function: bit-identical) -- with no allocation and no
 * synchronisation, graph-capturable.  The table holds copies of the structs: the operands they point at (and rg) must stay alive, their
 * CONTENTS are read at run time.  Plain layers only: a layer in the LayerNorm-fold form (kscale ..) is refused by `create` and stays a
 * per-layer i2i_lora_merge after the group (its row sums want one workgroup per row block).  All layers share `dtype`. */
int i2i_merge_group_create(const i2i_lora_merge_params* layers, int n, int dtype, void** group_out);
int i2i_merge_group_run(void* group, void* stream);
int i2i_merge_group_destroy(void* group);

/* ---- calibration micro-kernels (csrc/calib.hip; bench.py's `calib` block: what THIS box delivers on three elementary loads, so that
 * lines measured on different boxes of a pool can be compared).  Not on the forward path. */
int i2i_nop(void* stream);                                                         /* one empty kernel (1 wave) */
/* 1024 waves (one per SIMD) each issue `iters` x 8 independent v_mfma_f32_32x32x16 on operands read from `operands` (>= 64 KiB of dtype
 * data, random for a power-realistic reading); FLOPs = 1024 * iters * 8 * 32768.  `sink`: >= 1024*64 floats (keeps the work alive). */
int i2i_calib_mfma(int dtype, int iters, const void* operands, float* sink, void* stream);
/* dst[i] = src[i] over `bytes` (multiple of 16), 16 bytes per lane, grid-stride: 2 * bytes of HBM traffic */
int i2i_calib_stream(const void* src, void* dst, size_t bytes, void* stream);

/* ---- programs: a forward pass is a flat array of ops executed in order on one stream ---- */
int i2i_run(const i2i_op* ops, int n_ops, void* stream);
/* Same, with a hipEvent pair around every op; ms[i] = duration of op i (synchronises at the end). */
int i2i_run_timed(const i2i_op* ops, int n_ops, void* stream, float* ms);
/* Capture the program into a hipGraph (launch-bound bs=1 path) and replay it. */
int i2i_graph_create(const i2i_op* ops, int n_ops, void** graph_out);
int i2i_graph_launch(void* graph, void* stream);
int i2i_graph_destroy(void* graph);

/* ---- plan files (ABI v8): a planned forward saved by the Python planner (img2img_turbo_amd/plan_file.py: the op program, every buffer
 * its pointers refer to -- packed weights with their contents, activations as zero-filled scratch --, named input / output buffers and a
 * relocation table), loaded and run without Python.  The whole-forward entry for C / C++ hosts: what `model(x, caption_enc=..., eps=...)`
 * (src/pix2pix_turbo.py:186-219) is for a Python host, for one fixed (batch, size, dtype, mode).  Names of the pix2pix / CycleGAN plans:
 * "x" (fp32 NCHW images in [-1, 1], or uint8 NHWC with the u8 boundary), "ctx" ([1 | B][77][1024] text states in the plan's dtype),
 * "eps" (fp32 [B][4][H/8][W/8] posterior noise), "noise" (stochastic plans), "out" (images, NCHW in the plan's output dtype or uint8 NHWC);
 * plans exported with a seed also have "seed" (16 bytes: the i2i_randn_params state; the program then fills "eps" / "noise" itself;
 * 16 * B bytes, one state row per image, in a plan exported with per-image seeds: i2i_randn_batch_params.states, examples/batch_host.c);
 * edge plans have "canny_thr" (8 bytes {low, high}, or 8 * B bytes with per-image thresholds: i2i_canny_u8_batch_params.thr) and "canny_edges"
 * (uint8 [B][H][W][3]: the edge map the generator saw, 255 on edges; the reference's saved view is 255 - it); automatic-threshold plans
 * (i2i_canny_auto_thr_params: the program writes "canny_thr" itself) also have "canny_sigma" (4 * B bytes: int32 sigma * 65536 per image,
 * negative = that image keeps the pair the host wrote to "canny_thr") and "canny_median2" (4 * B bytes: uint32 doubled medians of the
 * last run): examples/auto_canny_host.c;
 * plans built with health= also have "health" (n_taps x 8 uint64: the i2i_scan_params records in program order, accumulated over the runs;
 * zero them with i2i_plan_write) and "health_names" (the n_taps labels, each NUL-terminated, as bytes): examples/health_host.c;
 * plans built with per-image health have "health" as n_taps x B x 8 uint64 (tap-major, one i2i_scan_batch_params record per tap and image,
 * zeroed by the program itself at the start of every run), "health_names" unchanged, and "verdict" (16 * B bytes: one row of four uint32
 * {first_bad, first_over, runs, bad_runs} per image, i2i_scan_verdict_params; saved zeroed, totals over the runs): examples/batch_health_host.c.
 * load / write / read are synchronous; run only enqueues (i2i_run); i2i_plan_ops() hands the program to i2i_graph_create(). */
int i2i_plan_load(const char* path, void** plan_out);
int i2i_plan_io(void* plan, const char* name, void** dev_ptr, size_t* bytes);       /* device address + size of a named buffer */
int i2i_plan_write(void* plan, const char* name, const void* host_src, size_t bytes);
int i2i_plan_read(void* plan, const char* name, void* host_dst, size_t bytes);     /* synchronises the device first */
int i2i_plan_ops(void* plan, const i2i_op** ops, int* n_ops);
int i2i_plan_run(void* plan, void* stream);
int i2i_plan_destroy(void* plan);
/* Live LoRA scale (ABI v13): a file exported with live_scale (magic "I2IPLAN2") also carries the scale program of its packers -- the
 * per-layer merge ops and the TwinConv fold with their fp32 masters, A, B and the device (r, gamma) pairs.  i2i_plan_set_scale writes
 * (r, gamma) to every such pair (one small launch on `stream`, ordered after whatever the stream still runs) and enqueues the scale
 * program on `stream`: one grouped launch for the plain layers, built at load through i2i_merge_group_create, then the remaining ops.  The
 * next i2i_plan_run on that stream computes at the new scale.  i2i_plan_has_scale: 1 / 0; set_scale on a plan without a scale program
 * returns I2I_ERR_UNSUPPORTED.  i2i_plan_ops() is the forward alone either way. */
int i2i_plan_has_scale(void* plan);
int i2i_plan_set_scale(void* plan, float r, float gamma, void* stream);
/* Self-verifying plan files (ABI 14 addition).  A file exported with digests (plan_file.py --digests / export_plan(digests=True)) ends with
 * an optional section behind the data: "I2IDIGS1", u32 count, u32 pad, then count x { u32 buf; u32 pad; u64 s0, s1, elements } -- one
 * i2i_digest_params record (I2I_U8 view of the whole buffer, index0 = 0, computed on the exporting device) for every buffer that is saved
 * with contents AND that no op of the program writes and no io name exposes: the weights, constants and tables.  A file without the
 * section is byte for byte what it was before and loads as before.  The loader checks the section like the rest of the file (count against
 * the buffer table and the bytes left in the file, every buf index in range, kind 1, no duplicates, elements == the buffer's size); a
 * malformed section fails the load.  Plans built with fingerprint= also have the io names "fingerprint" (taps x B x 4 uint64, tap-major:
 * one i2i_digest_params record per tap and image, zeroed by the program itself at the start of every run) and "fingerprint_names" (the tap
 * labels, NUL-terminated, as "health_names"): examples/fingerprint_host.c.
 * i2i_plan_verify digests those buffers again on the device (on `stream`, which it synchronises, as i2i_plan_read does) and compares:
 * 0 = all equal; I2I_ERR_MISMATCH = the first differing buffer's index in *first_bad_buffer (if given) and in i2i_last_error() with both
 * records; I2I_ERR_UNSUPPORTED = the file carries no digests.  On a live-scale file the records describe the weights AS EXPORTED: after
 * i2i_plan_set_scale to another r the merged weights differ by design, and back at the export scale they verify again. */
int i2i_plan_verify(void* plan, void* stream, int* first_bad_buffer);

#ifdef __cplusplus
}
#endif
#endif /* I2I_TURBO_H */

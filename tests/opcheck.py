"""Per-op parity checks shared by the CPU-emulator tests and the GPU tests.

Each check builds seeded inputs, runs ONE op of the HIP library through the C ABI
(``_capi.Library`` -- the real gfx950 build on a GPU box, the emulator twin on the CPU) and compares with
a plain PyTorch fp32 statement of the same op (the building blocks of oracle/nn.py).
"""
import math
import os

import torch
import torch.nn.functional as F

from img2img_turbo_amd import _capi as K
from img2img_turbo_amd import ops as O

TOL = {torch.float32: 2e-4, torch.bfloat16: 4e-2, torch.float16: 6e-3}
# unit roundoff of the storage types (round to nearest: half an ulp of 1)
U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
EPS32 = 2.0 ** -24
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)


def run_op(lib, opcode, params, dtype, device):
    prog = K.Program()
    prog.add(opcode, O.DT[dtype], params)
    prog.freeze()
    stream = torch.cuda.current_stream().cuda_stream if device != "cpu" else 0
    lib.run(prog, stream)
    if device != "cpu":
        torch.cuda.synchronize()


def pack_conv_weight(w, dtype, cpad=None):
    """OIHW -> [O][KH*KW*Ipad] (k = (ky,kx,ci), ci contiguous)."""
    o, i, kh, kw = w.shape
    ip = cpad or ((i + 7) // 8 * 8)
    wp = torch.zeros(o, kh, kw, ip, dtype=torch.float32)
    wp[..., :i] = w.permute(0, 2, 3, 1)
    return wp.reshape(o, kh * kw * ip).to(dtype).contiguous()


def nhwc(x, dtype, cpad=None):
    n, c, h, w = x.shape
    cp = cpad or ((c + 7) // 8 * 8)
    y = torch.zeros(n, h, w, cp, dtype=torch.float32)
    y[..., :c] = x.permute(0, 2, 3, 1)
    return y.to(dtype).contiguous()


def rel_err(got, ref):
    return float((got.float() - ref.float()).abs().max() / (ref.float().abs().max() + 1e-12))


def gn_scale_shift(x, groups, gamma, beta, eps):
    """fp32 reference of the (scale, shift) pairs i2i_gn_stats must produce. x: NCHW."""
    n, c, h, w = x.shape
    xg = x.reshape(n, groups, -1)
    mean = xg.mean(-1)
    var = xg.var(-1, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    cpg = c // groups
    sc = rstd.repeat_interleave(cpg, 1) * gamma[None]
    sh = beta[None] - mean.repeat_interleave(cpg, 1) * sc
    return torch.stack([sc, sh], -1).contiguous()  # [n][c][2]


def check_conv(lib, device, dtype, *, n=2, cin=16, cout=32, h=10, w=12, ks=3, stride=1, pad=1, ups=0,
               cin2=0, gn=False, act=0, bias=True, res=False, alpha=1.0, asym_pad=False, tile=0, seed=0, groups=4, splitk=0, subpix=False, k2c=0):
    """k2c: channels of a second NHWC tensor at output resolution whose 1x1 convolution is accumulated into the same output
    (i2i_igemm_params.k2_a: the decoder's skip conv folded into the upsampler)."""
    g = torch.Generator().manual_seed(seed)
    ct = cin + cin2
    x = torch.randn(n, ct, h, w, generator=g)
    wt = torch.randn(cout, ct, ks, ks, generator=g) / math.sqrt(ct * ks * ks)
    b = torch.randn(cout, generator=g) * 0.1 if bias else None
    xin = x.to(dtype).float()  # what the kernel sees
    ref_in = xin
    ss = None
    if gn:
        gamma = 1 + 0.1 * torch.randn(ct, generator=g)
        beta = 0.1 * torch.randn(ct, generator=g)
        ss = gn_scale_shift(xin, groups, gamma, beta, 1e-5)
        ref_in = xin * ss[:, :, 0][:, :, None, None] + ss[:, :, 1][:, :, None, None]
        if act:
            ref_in = F.silu(ref_in)
        ref_in = ref_in.to(dtype).float()  # kernel rounds the transformed operand to dtype
    if ups:
        ref_in = F.interpolate(ref_in, scale_factor=2.0, mode="nearest")
    wq = wt.to(dtype).float()
    if asym_pad:
        ref = F.conv2d(F.pad(ref_in, (0, 1, 0, 1)), wq, b, stride=stride)
        kpad = 0
    else:
        ref = F.conv2d(ref_in, wq, b, stride=stride, padding=pad)
        kpad = pad
    ref = ref * alpha if b is None else (ref - b[None, :, None, None]) * alpha + b[None, :, None, None]
    ho, wo = ref.shape[-2:]
    r = None
    if res:
        r = torch.randn(n, cout, ho, wo, generator=g)
        ref = ref + r.to(dtype).float()
    k2 = None
    if k2c:
        sk = torch.randn(n, k2c, ho, wo, generator=g)
        w2 = torch.randn(cout, k2c, generator=g) / math.sqrt(k2c)
        ref = ref + alpha * F.conv2d(sk.to(dtype).float(), w2.to(dtype).float()[:, :, None, None])
        k2 = (nhwc(sk, dtype).to(device), w2.to(dtype).contiguous().to(device), k2c)
    # device tensors
    x0 = nhwc(x[:, :cin], dtype).to(device)
    x1 = nhwc(x[:, cin:], dtype).to(device) if cin2 else None
    # weights: k = (ky,kx,[c0 | c1]) with each source padded to 8
    c0p = x0.shape[-1]
    c1p = x1.shape[-1] if cin2 else 0
    wp = torch.zeros(cout, ks, ks, c0p + c1p)
    wp[..., :cin] = wt[:, :cin].permute(0, 2, 3, 1)
    if cin2:
        wp[..., c0p:c0p + cin2] = wt[:, cin:].permute(0, 2, 3, 1)
    wp = wp.reshape(cout, -1).to(dtype).contiguous().to(device)
    if subpix:     # product packing of the sub-pixel form; the reference above stays F.conv2d on the upsampled input
        from img2img_turbo_amd.packer import subpixel_weights
        assert ups == 1 and not cin2 and c0p == cin
        wp = subpixel_weights(wt).reshape(4 * cout, 4 * cin).to(dtype).contiguous().to(device)
    ssd = None
    if gn:
        ssp = torch.zeros(n, c0p + c1p, 2)
        ssp[:, :cin] = ss[:, :cin]
        if cin2:
            ssp[:, c0p:c0p + cin2] = ss[:, cin:]
        ssd = ssp.contiguous().to(device)
    coutp = (cout + 7) // 8 * 8
    out = torch.full((n, ho, wo, coutp), float("nan"), dtype=dtype, device=device)
    rd = nhwc(r, dtype, coutp).to(device) if res else None
    bd = b.float().to(device) if bias else None
    wsd = torch.full((splitk * n * ho * wo * cout,), float("nan"), device=device) if splitk > 1 else None   # keep alive
    opcode, p = O.conv(x0, wp, out, nimg=n, hin=h, win=w, ho=ho, wo=wo, ks=ks, stride=stride, pad=kpad, ups=ups,
                       x1=x1, c0=c0p, c1=c1p, N=cout, gn_ss=ssd, act=act, bias=bd, alpha=alpha, res=rd, tile=tile,
                       splitk=splitk, ws=wsd, subpix=1 if subpix else 0, k2=k2)
    run_op(lib, opcode, p, dtype, device)
    got = out.cpu().float()[..., :cout].permute(0, 3, 1, 2)
    assert torch.isfinite(got).all(), "non-finite output"
    err = rel_err(got, ref)
    assert err < TOL[dtype], f"conv rel err {err}"
    return err


def check_geglu(lib, device, dtype, *, rows=70, cin=32, cff=64, seed=0, tile=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cin, generator=g)
    w = torch.randn(2 * cff, cin, generator=g) / math.sqrt(cin)
    b = torch.randn(2 * cff, generator=g) * 0.1
    xq, wq = x.to(dtype).float(), w.to(dtype).float()
    hgl = F.linear(xq, wq, b)
    a, gt = hgl.chunk(2, -1)
    ref = a * F.gelu(gt)
    # interleave rows per 16: [a 16][g 16]
    idx = []
    for j in range(cff // 16):
        idx += list(range(16 * j, 16 * j + 16)) + list(range(cff + 16 * j, cff + 16 * j + 16))
    idx = torch.tensor(idx)
    wp = w[idx].to(dtype).contiguous().to(device)
    bp = b[idx].float().contiguous().to(device)
    xd = x.to(dtype).contiguous().to(device)
    out = torch.full((rows, cff), float("nan"), dtype=dtype, device=device)
    opcode, p = O.conv(xd, wp, out, nimg=1, hin=1, win=rows, ho=1, wo=rows, ks=1, bias=bp, geglu=1, ldc=cff, tile=tile)
    run_op(lib, opcode, p, dtype, device)
    err = rel_err(out.cpu(), ref)
    assert err < TOL[dtype], f"geglu rel err {err}"
    return err


def check_bgemm(lib, device, dtype, *, batch=2, heads=2, M=40, N=24, Kd=64, out_f32=1, seed=0, tile=0):
    g = torch.Generator().manual_seed(seed)
    C = heads * Kd
    a = torch.randn(batch, M, C, generator=g).to(dtype)
    b = torch.randn(batch, N, C, generator=g).to(dtype)
    ref = torch.einsum("bmhk,bnhk->bhmn", a.float().view(batch, M, heads, Kd), b.float().view(batch, N, heads, Kd)) * 0.5
    ad, bd = a.to(device), b.to(device)
    out = torch.full((batch, heads, M, N), float("nan"), dtype=torch.float32 if out_f32 else dtype, device=device)
    opcode, p = O.bgemm(ad, bd, out, M=M, N=N, Kdim=Kd, lda=C, ldb=C, ldc=N, batch=batch, heads=heads,
                        a_bs=(M * C, Kd), b_bs=(N * C, Kd), c_bs=(heads * M * N, M * N), alpha=0.5, out_f32=out_f32, tile=tile)
    run_op(lib, opcode, p, dtype, device)
    err = rel_err(out.cpu(), ref)
    assert err < TOL[dtype], f"bgemm rel err {err}"
    return err


def check_gn_stats(lib, device, dtype, *, n=2, c0=32, c1=0, h=9, w=7, groups=8, nparts=3, eps=1e-5, seed=0, sliced=False):
    """sliced: hand the single-launch kernel its ticket counters (i2i_gn_stats_params.counters, ABI v7): the pixels of an image are
    cut into up to `nparts` slices, the last-arriving workgroup of an (image, group set) finalises.  Checked: same statistics,
    counters back at zero, and a second launch gives the same bits (slices are summed in slice order whoever arrives last)."""
    g = torch.Generator().manual_seed(seed)
    ct = c0 + c1
    x = torch.randn(n, ct, h, w, generator=g) * 1.5 + 0.3
    gamma = 1 + 0.1 * torch.randn(ct, generator=g)
    beta = 0.1 * torch.randn(ct, generator=g)
    xq = x.to(dtype).float()
    ref = gn_scale_shift(xq, groups, gamma, beta, eps)
    x0 = nhwc(x[:, :c0], dtype).to(device)
    x1 = nhwc(x[:, c0:], dtype).to(device) if c1 else None
    partial = torch.zeros(n * nparts * groups * 2, device=device)
    ss = torch.full((n, ct, 2), float("nan"), device=device)
    counters = torch.zeros(n * groups, dtype=torch.int32, device=device) if sliced else None
    gd, bd = gamma.to(device), beta.to(device)          # (named: the descriptor holds raw pointers, and the op runs twice below)
    opcode, p = O.gn_stats(x0, gd, bd, partial, ss, nimg=n, hw=h * w, groups=groups, eps=eps,
                           nparts=nparts, x1=x1, c0=c0, c1=c1, counters=counters)
    run_op(lib, opcode, p, dtype, device)
    err = rel_err(ss.cpu(), ref)
    assert err < 1e-4, f"gn_stats rel err {err}"
    if sliced:
        assert int(counters.abs().sum()) == 0, "the ticket counters must be left at zero"
        first = ss.clone()
        ss.fill_(float("nan"))
        run_op(lib, opcode, p, dtype, device)
        assert torch.equal(ss, first), "sliced statistics are not run-to-run identical"
        assert int(counters.abs().sum()) == 0
    return err


def check_gn_stats_offset(lib, device, dtype, *, n=2, c=32, h=48, w=40, groups=8, nparts=3, mean=100.0, std=0.1, seed=0, finalize_only=False, sliced=False):
    """GroupNorm statistics of a tensor sitting on a large offset (|mean| = 1000 sigma): E[x^2] - mu^2 in fp32 would return
    noise for the variance; the second, shifted pass over the flagged groups must bring x*scale + shift within 1e-3 of
    F.group_norm (which is two-pass).  Channels get different offsets so that groups differ.  finalize_only: the partial sums
    are handed over as a conv epilogue would (one-pass (sum, sum of squares) per part), the tensor rides along."""
    g = torch.Generator().manual_seed(seed)
    base = mean * (1 + 0.05 * torch.arange(groups).float()).repeat_interleave(c // groups)
    x = torch.randn(n, c, h, w, generator=g) * std + base[None, :, None, None]
    gamma = 1 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    xq = x.to(dtype).float()
    ref = F.group_norm(xq.double(), groups, gamma.double(), beta.double(), 1e-5).float()
    x0 = nhwc(x, dtype).to(device)
    ss = torch.full((n, c, 2), float("nan"), device=device)
    if finalize_only:
        cpg = c // groups
        xs = xq.reshape(n, groups, cpg, h * w)
        per = -(-(h * w) // nparts)
        parts = torch.zeros(n, nparts, groups, 2)
        for k in range(nparts):
            sl = xs[..., k * per:(k + 1) * per]
            parts[:, k, :, 0] = sl.sum((-1, -2))
            parts[:, k, :, 1] = (sl * sl).sum((-1, -2))
        partial = parts.reshape(-1).contiguous().to(device)
    else:
        partial = torch.zeros(n * nparts * groups * 2, device=device)
    counters = torch.zeros(n * groups, dtype=torch.int32, device=device) if sliced else None
    gd, bd = gamma.to(device), beta.to(device)
    opcode, p = O.gn_stats(x0, gd, bd, partial, ss, nimg=n, hw=h * w, groups=groups, eps=1e-5,
                           nparts=nparts, c0=c, finalize_only=1 if finalize_only else 0, counters=counters)
    run_op(lib, opcode, p, dtype, device)
    sc = ss.cpu()
    y = xq * sc[:, :, 0][:, :, None, None] + sc[:, :, 1][:, :, None, None]
    err = (y - ref).abs().max().item()
    scale = ref.abs().max().item()
    # fp32: 1e-3 of the output scale.  16-bit storage: one rounding step of the dtype the consumer applies / stores the normalised
    # value in (2^-8 bf16, 2^-11 fp16) -- csrc/norm.hip flags a group for the second pass only when the one-pass variance error
    # could exceed that (GnRefine<T>::RATIO)
    tol = {torch.float32: 1e-3, torch.float16: max(1e-3, 2.0 ** -11), torch.bfloat16: 2.0 ** -8}[dtype]
    assert torch.isfinite(y).all() and err < tol * max(scale, 1.0), f"gn_stats with offset: max-abs {err} (outputs up to {scale}, tol {tol})"
    return err


def _row_offset(mu_sigma, rows):
    """A per-row DC offset in units of the row's sigma: a number (every row) or a tensor that is tiled over the rows (rows of both
    signs and rows of offset 0 in ONE launch)."""
    if torch.is_tensor(mu_sigma):
        return mu_sigma.double().flatten().repeat(-(-rows // mu_sigma.numel()))[:rows].float()
    return torch.full((rows,), float(mu_sigma))


def check_layernorm(lib, device, dtype, *, rows=9, c=320, seed=0, mu_sigma=None, sigma=2.0):
    """mu_sigma (number or per-row tensor): rows sit on a DC offset of mu_sigma standard deviations.  Then the output is also held to a
    per-element bound against F.layer_norm in fp64 on the rounded input.  csrc/norm.hip is TWO-pass (mean first, then the sum of
    (x - mean)^2 over the registers), so no E[x^2] - mu^2 cancellation exists and the offset enters only through the error of the
    mean: a lane adds c/64 values and the wave sum adds 6 levels, |d mu| <= (c/64 + 6) eps mean|x| <= (c/64 + 6) eps (|mu| + sigma),
    which moves every normalised value by d mu / sigma -- LINEAR in mu/sigma (the one-pass form would be eps (mu/sigma)^2; the
    linear term is the smaller, stricter one for mu/sigma > 1).  The sum of squares has the same summation error, relative
    (c/64 + 6) eps, half of it lands in rstd; rsqrt, the subtraction, the two multiplies and the add are one rounding each
    (<= 6 eps of |y| + |beta|).  With u the roundoff of the stored type (one rounding of y):
        |got - y| <= u |y| + eps (c/64 + 12) (|gamma| (|mu|/sigma + 1) + |y| + |beta|),   eps = 2^-24."""
    g = torch.Generator().manual_seed(seed)
    if mu_sigma is None:
        x = torch.randn(rows, c, generator=g) * 2 + 0.5
    else:
        x = (torch.randn(rows, c, generator=g) + _row_offset(mu_sigma, rows)[:, None]) * sigma
    gamma = 1 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    ref = F.layer_norm(x.to(dtype).float(), (c,), gamma, beta, 1e-5)
    xd = x.to(dtype).to(device)
    y = torch.full((rows, c), float("nan"), dtype=dtype, device=device)
    opcode, p = O.layernorm(xd, y, gamma.to(device), beta.to(device), rows=rows, c=c)
    run_op(lib, opcode, p, dtype, device)
    err = rel_err(y.cpu(), ref)
    assert err < TOL[dtype], f"layernorm rel err {err}"
    if mu_sigma is not None:
        x64 = x.to(dtype).double()
        y64 = F.layer_norm(x64, (c,), gamma.double(), beta.double(), 1e-5)
        mu = x64.mean(1, keepdim=True).abs()
        sd = (x64.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
        bound = U[dtype] * y64.abs() + EPS32 * (c / 64 + 12) * (gamma.double().abs()[None] * (mu / sd + 1) + y64.abs() + beta.double().abs()[None])
        got = y.cpu().double()
        assert torch.isfinite(got).all()
        ratio = ((got - y64).abs() / bound).max().item()
        print("[numerics] layernorm %s rows=%d c=%d mu/sigma<=%.0f: max |err|/bound = %.3f (max-abs err %.3e, rel_err %.2e)"
              % (str(dtype).split(".")[-1], rows, c, float((mu / sd).max()), ratio, (got - y64).abs().max().item(), err))
        assert ratio <= 1.0, f"layernorm on a DC offset: error {ratio:.3f} x its per-element bound"
    return err


def check_softmax(lib, device, dtype, *, rows=11, cols=77, ldp=80, seed=0, flavour=None, scale=0.125):
    """flavour: adversarial rows -- 'span' (logits over +-300 before the scale), 'const' (every logit equal: p = 1/cols exactly),
    'dominant' (one column 200 above the rest: p = 1 there, underflow elsewhere), mixed with ordinary rows in one launch.  These are
    held to a per-element bound against an fp64 softmax of the fp32 scores:
        |got - p| <= u p + (cols + 4) eps p + (8 |z|max + 1) eps p,   eps = 2^-24
    u p: the one rounding to the stored type; (cols + 4) eps: the fp32 row sum (cols additions), the exponential, the reciprocal and
    the product.  The last term is the exponent's own rounding, an ABSOLUTE error there and so a relative one in p: z = fl(scale s)
    is off by eps |z|, x = fl(z - max) by eps |x| with |x| <= 2 |z|max, and __expf forms 2^(x log2 e), a third rounding of eps |x| plus
    half of one for the constant: eps (|z| + 2.5 |x|) <= 6 eps |z|max for the element itself.  The same errors enter the row sum
    weighted by p = e^x, where |x| e^x <= 0.37: at most (2 |z|max + 1) eps more.  (Sized for the +-300 rows; it vanishes on ordinary
    ones.)  fp16 is subnormal below 2^-14: there the error is at most half the subnormal step, 2^-25, absolute; f32 / bf16 results
    below the smallest normal number may be flushed: 2^-126 absolute."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, cols, generator=g) * 4
    if flavour == "span":
        s = (torch.rand(rows, cols, generator=g) * 2 - 1) * 300 / scale
        s[::3] = torch.randn(-(-rows // 3), cols, generator=g) * 4
    elif flavour == "const":
        s[::2] = torch.randn(-(-rows // 2), 1, generator=g) * 50
    elif flavour == "dominant":
        s[torch.arange(rows), torch.arange(rows) * 7 % cols] += 200 / scale
    ref = torch.softmax(s * scale, -1)
    sd = s.to(device)
    pout = torch.full((rows, ldp), float("nan"), dtype=dtype, device=device)
    opcode, p = O.softmax(sd, pout, rows=rows, cols=cols, lds=cols, ldp=ldp, scale=scale)
    run_op(lib, opcode, p, dtype, device)
    got = pout.cpu().float()
    assert (got[:, cols:] == 0).all()
    err = rel_err(got[:, :cols], ref)
    assert err < TOL[dtype], f"softmax rel err {err}"
    if flavour is not None:
        z = s.double() * float(torch.tensor(scale, dtype=torch.float32))
        p64 = torch.softmax(z, -1)
        zmax = z.abs().max(1, keepdim=True).values
        bound = p64 * (U[dtype] + (cols + 4) * EPS32 + (8 * zmax + 1) * EPS32) + (2.0 ** -25 if dtype == torch.float16 else 2.0 ** -126)
        g64 = got[:, :cols].double()
        assert torch.isfinite(g64).all()
        ratio = ((g64 - p64).abs() / bound).max().item()
        print("[numerics] softmax %s %s rows=%d cols=%d: max |err|/bound = %.3f (rel_err %.2e)" % (str(dtype).split(".")[-1], flavour, rows, cols, ratio, err))
        assert ratio <= 1.0, f"softmax ({flavour}): error {ratio:.3f} x its per-element bound"
        if flavour == "const":
            assert (g64[::2] - 1.0 / cols).abs().max() <= (U[dtype] + (cols + 4) * EPS32) / cols
    return err


def check_gn_apply(lib, device, dtype, *, n=2, c=64, c1=0, h=6, w=7, act=1, seed=0):
    """Standalone GroupNorm apply (+SiLU) from a (scale, shift) table; ``c1``: a second source whose channels follow the first's
    (i2i_gn_apply_params.x1, ABI v10: the concatenated input of an up-block resnet in one launch)."""
    g = torch.Generator().manual_seed(seed)
    ct = c + c1
    x = torch.randn(n, h * w, ct, generator=g).to(dtype)
    ss = torch.stack([1 + 0.2 * torch.randn(n, ct, generator=g), 0.3 * torch.randn(n, ct, generator=g)], -1).contiguous()
    ref = x.float() * ss[:, None, :, 0] + ss[:, None, :, 1]
    if act:
        ref = F.silu(ref)
    x0 = x[..., :c].contiguous().to(device)
    x1 = x[..., c:].contiguous().to(device) if c1 else None
    y = torch.full((n, h * w, ct), float("nan"), dtype=dtype, device=device)
    opcode, p = O.gn_apply(x0, y, ss.to(device), nimg=n, hw=h * w, c=c, act=act, ldy=ct, ss_ld=ct, x1=x1, c1=c1)
    run_op(lib, opcode, p, dtype, device)
    got = y.cpu().float()
    assert torch.isfinite(got).all()
    err = rel_err(got, ref)
    assert err < TOL[dtype], f"gn_apply rel err {err}"
    return err


def attention_kernel_of(dtype, d):
    """Which kernel of csrc/attention.hip a (dtype, head dim) pair reaches for the aligned operands these checks build."""
    return "reg" if dtype == torch.float32 else ("wide" if d == 512 else "dma")


def attention_ref64(q, k, v, *, heads, d, scale, dtype, causal=False, ideal=False):
    """fp64 statement of what each kernel documents, from the dtype-rounded q, k, v ([batch][T][heads * d]).

    * 16-bit, d = 64 (attention_dma_kernel; include/i2i_turbo.h, i2i_attention_params): works in log2 units; with
      scale * log2(e) != 1 it multiplies q by that factor ONCE at load and re-rounds it to the 16-bit type, with scale = ln 2 the
      caller's q is used as it is.  Reference: q' = round_T(fl32(q * fl32(scale * log2 e))) resp. q' = q, L = q' . k, p = 2^L / sum.
    * f32 (attention_kernel) and 16-bit d = 512 (attention_wide_kernel): their header comments describe softmax(scale * q k^T) v
      with q untouched -- the scores are scaled in fp32 after the contraction (by scale and e^x, resp. by scale * log2 e and
      2^x).  Reference: L = (q . k) * scale * log2 e, p = 2^L / sum.
    Returns (O, A, L, T) as [batch][heads][tq][..] fp64: O = p V, A = p |V| (the per-element scale of O), the log2 scores L (masked
    ones -inf) and T, the weight of the score-rounding term of attention_bound per output element: with t_ij = sum_c |q'_ic k_jc| in
    log2 units (the size of the terms the fp32 contraction of score (i, j) adds),  T = (sum_j p_j t_ij |v_j|) / A + sum_j p_j t_ij."""
    batch, tq = q.shape[:2]
    kern = "reg" if ideal else attention_kernel_of(dtype, d)       # ideal: q NOT re-rounded (what the re-rounding costs is measured against it)
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)       # fp32, as the kernel forms it
    ready = abs(float(c2) - 1.0) < 1e-6
    if kern == "dma" and not ready:
        q = (q.float() * c2).to(dtype)
    post = 1.0 if kern == "dma" else float(c2)
    qh, kh, vh = (t.double().view(batch, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    L = (qh @ kh.transpose(-1, -2)) * post
    T = (qh.abs() @ kh.abs().transpose(-1, -2)) * post
    if causal:
        L = L.masked_fill(torch.ones(tq, tq, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(L * LN2, -1)
    A = p @ vh.abs()
    T.mul_(p)
    T = (T @ vh.abs()) / (A + 1e-300) + T.sum(-1, keepdim=True)
    return p @ vh, A, L, T


def attention_bound(dtype, d, tk, ksplit, A, T, vmax):
    """Per-element bound on |got - O| / A, derived (not fitted):
      16-bit types, u = 2^-8 (bf16) / 2^-11 (fp16):
        u   every probability is rounded once to the 16-bit type before the second contraction: sum_j u p_j |v_j| = u A;
        u   the row sum is taken over those same rounded numbers: u |O| <= u A (the d = 512 kernel sums the unrounded ones: no worse);
        u   the output is rounded once: u |O| <= u A                                                             -> 3u
      f32: the probability operand of attention_kernel<float> is the fp32 accumulator itself (fp32 MFMA), so only the output rounding
        of u = 2^-24 remains of the three.
      fp32 arithmetic, eps = 2^-24:
        (tk + 4) eps          the two fp32 accumulations over tk keys (P.V and the row sum), v_exp, the reciprocal, the product;
        2 ksplit eps          key splits: the merge weighs and adds ksplit partials of O and of the row sum;
        ln2 (d + 2) eps T     SCORE ROUNDING (the term the first-order list leaves out): the log2 score of (query i, key j) is an fp32
                              contraction of d products (+ the reference it starts from, + the scale factor where the kernel applies it
                              afterwards), off by at most dL_ij = (d + 2) eps t_ij, t_ij = sum_c |q_ic k_jc|; an absolute error dL in an
                              exponent is a relative error ln2 dL in p, so to first order
                              |dO| <= ln2 (sum_j p_j dL_ij |v_j| + (sum_j p_j dL_ij) A): the numerator and the row sum, each key weighed
                              by its OWN t_ij and its probability (T of attention_ref64, per output element; not the row's maximum of
                              t).  Negligible for N(0,1) operands (t ~ 7), the leading fp32 term when all scores sit on a common
                              offset of +-120.
      fp16 only: tk 2^-25 max|v| / A   probabilities below 2^-14 are subnormal (absolute error <= 2^-25 each, the reference never
                              exceeds the row maximum so the row sum is >= 1)."""
    f32 = dtype == torch.float32
    b = (1.0 if f32 else 3.0) * U[dtype] + (tk + 4 + 2 * max(ksplit, 0)) * EPS32 + LN2 * (d + 2) * EPS32 * T
    b = b.expand_as(A).clone()
    if dtype == torch.float16:
        b = b + tk * 2.0 ** -25 * vmax / (A + 1e-300)
    return b


def run_attention(lib, device, dtype, q, k, v, *, heads, d, scale, causal=False, ksplit=0, fused_qk=False):
    """One i2i_attention call on [batch][T][heads * d] operands; returns the output as fp64 on the CPU.  fused_qk: q and k live in ONE
    [batch][T][2C] buffer (ldq = ldk = 2C, q_bs = k_bs = T * 2C, the k pointer offset by C) as the UNet planner's and the text tower's
    [q|k] projection leaves them."""
    batch, tq, C = q.shape
    tk = k.shape[1]
    epc = 4 if dtype == torch.float32 else 8
    ldvt = (tk + epc - 1) // epc * epc
    vt = torch.full((batch, C, ldvt), float("nan"), dtype=dtype)  # padding deliberately poisoned
    vt[:, :, :tk] = v.transpose(1, 2)
    vtd = vt.to(device)
    if fused_qk:
        assert tq == tk
        qk = torch.cat([q, k], -1).contiguous().to(device)
        qd, kd, ldqk, qk_bs = qk, qk.view(-1)[C:], 2 * C, tq * 2 * C
    else:
        qd, kd, ldqk, qk_bs = q.to(device), k.to(device), C, None
    o = torch.full((batch, tq, C), float("nan"), dtype=dtype, device=device)
    ws = torch.full((batch * heads * ksplit * tq * (d + 2),), float("nan"), device=device) if ksplit > 1 else None
    opcode, p = O.attention(qd, kd, vtd, o, batch=batch, heads=heads, d=d, tq=tq, tk=tk, ldq=ldqk, ldk=ldqk, ldvt=ldvt, ldo=C,
                            q_bs=qk_bs or tq * C, k_bs=qk_bs or tk * C, vt_bs=C * ldvt, o_bs=tq * C, scale=scale, causal=int(causal),
                            ksplit=ksplit, ws=ws)
    run_op(lib, opcode, p, dtype, device)
    return o.cpu()


def attention_numerics(got, q, k, v, *, heads, d, scale, dtype, causal, ksplit, what):
    """E = max |got - O| / (A + tiny) against attention_ref64, its bound (attention_bound), one [numerics] line; asserts E <= bound
    per element.  Returns (E / bound at the worst element, L)."""
    batch, tq, C = q.shape
    tk = k.shape[1]
    O64, A, L, T = attention_ref64(q, k, v, heads=heads, d=d, scale=scale, dtype=dtype, causal=causal)
    g64 = got.double().view(batch, tq, heads, d).transpose(1, 2)
    assert torch.isfinite(g64).all(), "non-finite attention output"
    bound = attention_bound(dtype, d, tk, ksplit, A, T, float(v.float().abs().max()))
    E = (g64 - O64).abs() / (A + 1e-300)
    ratio = E / bound
    i = int(ratio.argmax())
    worst = float(ratio.flatten()[i])
    ref = O64.transpose(1, 2).reshape(batch, tq, C)
    extra = ""
    if attention_kernel_of(dtype, d) == "dma" and abs(scale * LOG2E - 1.0) >= 1e-6:      # measured, not gated: the same output against q WITHOUT the re-rounding
        Oi, Ai, _, _ = attention_ref64(q, k, v, heads=heads, d=d, scale=scale, dtype=dtype, causal=causal, ideal=True)
        extra = "  [vs un-re-rounded q: E = %.3e]" % float(((g64 - Oi).abs() / (Ai + 1e-300)).max())
    print("[numerics] attention %s %s: E = %.3e (worst vs bound: E = %.3e, bound %.3e, ratio %.3f)  rel_err %.2e%s"
          % (str(dtype).split(".")[-1], what, float(E.max()), float(E.flatten()[i]), float(bound.flatten()[i]), worst, rel_err(got, ref), extra))
    assert worst <= 1.0, f"attention {what}: |got - O| / A = {float(E.flatten()[i]):.3e} exceeds the derived bound {float(bound.flatten()[i]):.3e}"
    return worst, L


def check_attention(lib, device, dtype, *, batch=2, heads=2, tq=70, tk=77, d=64, seed=0, spike=False, ksplit=0,
                    prescaled=False, fused_qk=False, causal=False):
    """ksplit > 1: keys divided among ksplit workgroups per query tile + the merge launch (i2i_attention_params.ksplit, d = 512).
    prescaled: the product's convention -- q = round_T(q0 * scale * log2 e) is built on the host and the op gets scale = ln 2 (the
    reference uses that q as it is).  fused_qk: q and k in one [batch][T][2C] buffer (run_attention).  causal: tq == tk, keys > query
    masked (the reference by triu(1)).  Besides the historic rel_err gate every call is held to the per-element bound of
    attention_bound against the fp64 reference of attention_ref64."""
    g = torch.Generator().manual_seed(seed)
    C = heads * d
    q = torch.randn(batch, tq, C, generator=g).to(dtype)
    k = torch.randn(batch, tk, C, generator=g).to(dtype)
    v = torch.randn(batch, tk, C, generator=g).to(dtype)
    if spike:  # force a late running-max jump (rescale branch) on one query
        k[0, tk - 3, :d] = q[0, 5, :d] * 3
    scale = 1.0 / math.sqrt(d)
    qf, kf, vf = (t.float().view(batch, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    s32 = qf @ kf.transpose(-1, -2) / math.sqrt(d)
    if causal:
        assert tq == tk
        s32 = s32.masked_fill(torch.ones(tq, tq, dtype=torch.bool).triu(1), float("-inf"))
    ref = torch.softmax(s32, -1) @ vf
    ref = ref.transpose(1, 2).reshape(batch, tq, C)
    if prescaled:
        q = (q.float() * (scale * LOG2E)).to(dtype)
        scale = LN2
    got = run_attention(lib, device, dtype, q, k, v, heads=heads, d=d, scale=scale, causal=causal, ksplit=ksplit, fused_qk=fused_qk)
    assert torch.isfinite(got.float()).all()
    err = rel_err(got, ref)
    assert err < TOL[dtype], f"attention rel err {err}"
    what = "b%d h%d tq%d tk%d d%d%s%s%s%s%s" % (batch, heads, tq, tk, d, " ksplit=%d" % ksplit if ksplit else "", " prescaled" if prescaled else "",
                                               " fused_qk" if fused_qk else "", " causal" if causal else "", " spike" if spike else "")
    attention_numerics(got, q, k, v, heads=heads, d=d, scale=scale, dtype=dtype, causal=causal, ksplit=ksplit, what=what)
    return err


def check_attention_causal_ksplit_refused(lib, device, dtype, *, tq=136, d=64):
    """causal with ksplit > 1 is not implemented: the call must return I2I_ERR_UNSUPPORTED and leave the output untouched."""
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(1, tq, d, generator=g).to(dtype) for _ in range(3))
    vt = v.transpose(1, 2).contiguous()
    ldvt = vt.shape[-1]
    assert ldvt % 8 == 0
    qd, kd, vtd = q.to(device), k.to(device), vt.to(device)
    o = torch.full((1, tq, d), 7.0, dtype=dtype, device=device)
    ws = torch.zeros(2 * tq * (d + 2), device=device)
    opcode, p = O.attention(qd, kd, vtd, o, batch=1, heads=1, d=d, tq=tq, tk=tq, ldq=d, ldk=d, ldvt=ldvt, ldo=d, q_bs=tq * d, k_bs=tq * d,
                            vt_bs=d * ldvt, o_bs=tq * d, scale=0.125, causal=1, ksplit=2, ws=ws)
    import ctypes
    rc = lib.lib.i2i_attention(ctypes.byref(p), O.DT[dtype], None)          # the entry point itself: the error CODE is the contract
    assert rc == -3, "causal attention with ksplit = 2: expected I2I_ERR_UNSUPPORTED (-3), got %d" % rc
    if device != "cpu":
        torch.cuda.synchronize()
    assert (o.cpu().float() == 7.0).all(), "a refused call wrote to its output"


# ---------------------------------------------------------------- score-pattern stress of the lazy softmax reference
def att_qf():
    """Query fragments per wave attention_dma_kernel is launched with.  The trigger map has to replay the wave width that really ran,
    so the caller FORCES it (I2I_ATT_QF = 1 / 2, read by launch_att_dma at every launch) on the emulator and on the GPU alike -- a
    copy of the launcher's own choice here would go stale silently when that rule changes."""
    force = int(os.environ.get("I2I_ATT_QF", "0") or 0)
    assert force in (1, 2), "check_attention_scores (d = 64): set I2I_ATT_QF to 1 or 2, the replay must know the wave width"
    return force


def expected_moves(pattern, events, *, batch, heads, nwave, wave_q, bkv, ntile, ksplit):
    """What each pattern is NAMED for, per (batch, head, wave, key split), stated without looking at any score: the tiles (of bkv keys)
    at which the reference has to move.  A split covers tiles [lo, hi); its first tile only sets the reference.
      stair9            the level rises 9 units every 64 keys: a move at every later tile that starts a new level;
      stair7            7 units every 64 keys: the lazy reference (64-key tiles, threshold 8) moves on every SECOND tile of the split,
                        a running maximum (d = 512) at every tile that starts a new level;
      everything else   `events` = (batch | None, head | None, query | None, key): a key that dominates what came before it, for one
                        query or for all -- one move at its tile for the wave(s) it concerns, unless that tile is the split's first."""
    S = max(ksplit, 1)
    per = -(-ntile // S)
    r = 64 // bkv
    exp = {}
    for b in range(batch):
        for h in range(heads):
            for w in range(nwave):
                for s_ in range(S):
                    lo, hi = s_ * per, min(s_ * per + per, ntile)
                    if pattern == "stair9" or (pattern == "stair7" and r > 1):
                        mv = [t for t in range(lo + 1, hi) if t % r == 0]
                    elif pattern == "stair7":
                        mv = list(range(lo + 2, hi, 2))
                    else:
                        mv = sorted({j // bkv for (eb, eh, ei, j) in events if eb in (None, b) and eh in (None, h)
                                     and (ei is None or ei // wave_q == w) and lo < j // bkv < hi})
                    exp[(b, h, w, s_)] = mv
    return exp


def replay_reference(L, *, wave_q, bkv, lazy, ksplit):
    """The documented rule of the softmax reference in plain Python, per wave (wave_q queries: 16 * QF; the d = 512 kernel: 16) and key
    tile (bkv keys), per key split: the reference of a query starts at its maximum over the split's first tile; a later tile moves
    the references of the WHOLE wave (each to max(reference, tile maximum)) when some query of the wave has a score more than `lazy`
    above its reference (wave-uniform test; lazy = 0: the running maximum of attention_wide_kernel).  L: [batch][heads][tq][tk] log2
    scores (fp64, masked = -inf).  Returns {(b, h, wave, split): [tile indices at which the reference moved]}."""
    batch, heads, tq, tk = L.shape
    ntile = -(-tk // bkv)
    S = max(ksplit, 1)
    per = -(-ntile // S)
    tmax = torch.stack([L[..., t * bkv:(t + 1) * bkv].max(-1).values for t in range(ntile)], -1)      # [b][h][tq][ntile]
    moves = {}
    for b in range(batch):
        for h in range(heads):
            for w in range(-(-tq // wave_q)):
                tm = tmax[b, h, w * wave_q:(w + 1) * wave_q]
                for s in range(S):
                    lo, hi = s * per, min(s * per + per, ntile)
                    mv = []
                    if lo < hi:
                        ref = tm[:, lo].clone()
                        for t in range(lo + 1, hi):
                            if bool((tm[:, t] - ref > lazy).any()):
                                mv.append(t)
                                ref = torch.maximum(ref, tm[:, t])
                    moves[(b, h, w, s)] = mv
    return moves


ATT_PATTERNS = ("stair7", "stair9", "under", "over", "spike_query", "split_place", "split_far", "offset", "descending")


def check_attention_scores(lib, device, dtype, pattern, *, d=64, ksplit=0, tq=128, tk=None, qbase=0, seed=0):
    """Designed score patterns against the lazy reference of attention_dma_kernel (d = 64), the running maximum of
    attention_wide_kernel (d = 512) and the merge of key splits.  q and k are built from disjoint channel blocks so that the log2 score
    of (query i, key j) is close to a designed level:  block 0 (d/4 channels): q = 1, k = level_j / (d/4)  -> a per-key level common to
    all queries;  block 1: q = 1 on the spiked query only, k = 30 / (d/4) on its key  -> +30 for ONE (query, key) pair;  block 2: q = 1,
    k = +-120 / (d/4) -> a common offset, exact in every format;  block 3: N(0, s) noise worth 0.05 log2 units, so queries differ.
    The op is called the product's way (q carries the factor, scale = ln 2), so the log2 score is q . k itself.

    The TRIGGER MAP comes first: the real scores are recomputed in fp64 from the rounded tensors, the documented rule is replayed
    (replay_reference), and the number and position of the reference moves is asserted to be what the pattern is named for, with no
    tile within 0.05 units of the threshold -- on the CPU, before the op runs: a pattern that misses its branch fails as a test bug.
    The named property is stated a second time without any score (expected_moves) and asserted per (wave, key split), for every
    ksplit and for both kernels.  Then the op runs and is held to attention_bound per element.  d = 64: the caller forces the wave
    width (I2I_ATT_QF, att_qf); returns it.

    Patterns (tk defaults to 6 key tiles, the last one ragged):
      stair7 / stair9   the level rises 7 / 9 units per 64-key tile over 7 tiles: moves on every second tile / on every tile;
      under / over      one key of a middle tile sits 7.5 / 8.5 above everything else for every query: no move at all (P ~ 180 beside
                        P <= 1) / exactly one move, there;
      spike_query       +30 on exactly one query per (batch, head): lr 0 / 15 x fragment 0 / 1 x wave 0 / 3 over the batch, the key in
                        the first, a middle and the ragged last tile over the heads; only that query's wave moves, only there;
      split_place       one key 30 above the rest for all queries, in the first tile of every split in turn (heads), and a launch with
                        more splits than key tiles when tk is given below 128 (ksplit = 4: tk = 100 is two tiles of 64, tk = 40 two of 32);
      split_far         the keys of the second half sit 70 units above the first half: with key splits the merge multiplies a partial by
                        2^-70 (without: one move);
      offset            all scores shifted by +120 and by -120: finite, within the bound, and equal to the unshifted run within twice
                        the bound (the shift is exact in the operands, so the fp64 reference does not change);
      descending        the first tile holds the maximum, every later tile sits 40 below: no move, probabilities underflow in fp16."""
    g = torch.Generator().manual_seed(seed)
    kern = attention_kernel_of(dtype, d)
    assert kern in ("dma", "wide")
    bkv, lazy = (64, 8.0) if kern == "dma" else (32, 0.0)
    nb = d // 4                                                   # channels per block
    batch, heads = 1, 2
    if pattern == "spike_query":
        batch, heads = 8, 3
    if pattern == "split_place":
        heads = max(ksplit, 1) + 1
    if tk is None:
        tk = 7 * 64 - 20 if pattern.startswith("stair") else 325
    tq = tq + qbase
    ntile64 = -(-tk // 64)
    level = torch.zeros(batch, heads, tk, dtype=torch.float64)
    spike = []                                                   # (b, h, query, key)
    key_tile = torch.arange(tk) // 64
    mid = (3 if ksplit == 4 else 2) * 64          # the "middle tile" key: never in the FIRST tile of its key split (6 x 64 resp. 11 x 32 keys over 1 / 2 / 4 splits)
    events = []                                   # (batch | None, head | None, query | None, key): expected_moves
    if pattern in ("stair7", "stair9"):
        level[:] = (key_tile * (7.0 if pattern == "stair7" else 9.0))[None, None]
    elif pattern in ("under", "over"):
        level[:, :, mid + 37] = 7.5 if pattern == "under" else 8.5
        if pattern == "over" or kern == "wide":   # (a running maximum moves for 7.5 as well)
            events.append((None, None, None, mid + 37))
    elif pattern == "spike_query":
        for b in range(batch):
            lr, frag, wave = (0, 15)[b & 1], (b >> 1) & 1, (0, 3)[b >> 2]
            for h in range(heads):
                spike.append((b, h, qbase + wave * 32 + frag * 16 + lr, (5, mid + 41, tk - 3)[h]))
        events = list(spike)
    elif pattern == "split_place":
        per = -(-ntile64 // max(ksplit, 1))
        for h in range(heads):
            level[:, h, min(h * per * 64 + 9, tk - 2)] = 30.0     # head h: the dominant key in split h (the last head: the last tile)
            events.append((None, h, None, min(h * per * 64 + 9, tk - 2)))
    elif pattern == "split_far":
        half = -(-ntile64 // 2) * 64
        level[:, :, half:] = 70.0
        events.append((None, None, None, half))
    elif pattern == "descending":
        level[:, :, 64:] = -40.0
    elif pattern != "offset":
        raise ValueError(pattern)

    def build(shift):
        q = torch.zeros(batch, tq, heads, d)
        k = torch.zeros(batch, tk, heads, d)
        q[..., :nb] = 1.0
        k[..., :nb] = (level / nb).float().permute(0, 2, 1)[..., None]
        for (b, h, i, j) in spike:
            q[b, i, h, nb:2 * nb] = 1.0
            k[b, j, h, nb:2 * nb] = 30.0 / nb
        if shift:
            q[..., 2 * nb:3 * nb] = 1.0
            k[..., 2 * nb:3 * nb] = shift / nb
        sn = math.sqrt(0.05 / math.sqrt(nb))
        q[..., 3 * nb:] = torch.randn(batch, tq, heads, nb, generator=torch.Generator().manual_seed(seed + 11)) * sn
        k[..., 3 * nb:] = torch.randn(batch, tk, heads, nb, generator=torch.Generator().manual_seed(seed + 12)) * sn
        return q.reshape(batch, tq, heads * d).to(dtype), k.reshape(batch, tk, heads * d).to(dtype)

    v = torch.randn(batch, tk, heads * d, generator=g).to(dtype)
    qf = att_qf() if kern == "dma" else 1
    wave_q = 16 * qf
    design = level[:, :, None, :].expand(batch, heads, tq, tk).clone()
    for (b, h, i, j) in spike:
        design[b, h, i, j] += 30.0
    want = replay_reference(design, wave_q=wave_q, bkv=bkv, lazy=lazy, ksplit=ksplit)
    if pattern == "split_place" and tk < 128:
        assert ksplit > -(-tk // bkv), "this is the case with more splits than key tiles (empty splits)"
    outs = []
    for shift in ((0.0, 120.0, -120.0) if pattern == "offset" else (0.0,)):
        q, k = build(shift)
        _, _, L, _ = attention_ref64(q, k, v, heads=heads, d=d, scale=LN2, dtype=dtype)
        # ---- the trigger map of the REAL scores, and the property the pattern is named for
        have = replay_reference(L, wave_q=wave_q, bkv=bkv, lazy=lazy, ksplit=ksplit)
        if kern == "dma":
            assert have == want, "pattern %s: the rounded tensors do not move the reference where the design does" % pattern
            for eps in (-0.05, 0.05):       # nothing near the threshold: the fp32 kernel decides every tile as the fp64 replay does
                assert replay_reference(L, wave_q=wave_q, bkv=bkv, lazy=lazy + eps, ksplit=ksplit) == have, "pattern %s: a tile within 0.05 of the threshold" % pattern
        nmoves = sum(len(m) for m in have.values())
        first = have[(0, 0, 0, 0)]
        # ---- the NAMED property, per (wave, key split), from expected_moves (no score enters it): exact for the lazy reference; for the
        # running maximum of d = 512 (threshold 0: the 0.05 units of noise move it among equal levels) the named moves must be there
        ntile = -(-tk // bkv)
        S, per_t = max(ksplit, 1), -(-ntile // max(ksplit, 1))
        exp = expected_moves(pattern, events, batch=batch, heads=heads, nwave=-(-tq // wave_q), wave_q=wave_q, bkv=bkv, ntile=ntile, ksplit=ksplit)
        assert exp.keys() == have.keys()
        if kern == "dma":
            assert have == exp, "pattern %s: moves %s, named for %s" % (pattern, have, exp)
        else:
            assert all(set(exp[key]) <= set(have[key]) for key in exp), "pattern %s: moves %s lack some of %s" % (pattern, have, exp)
            if pattern == "descending":           # no move once the first 64 keys (the maximum) are past; later splits are flat at -40: noise only
                assert all(t < 64 // bkv for (b, h, w, s_), m in have.items() if s_ == 0 for t in m), have
        nexp = sum(len(m) for m in exp.values())
        # (stair7 through the lazy reference needs splits of three tiles to move at all; ksplit = 4 over these 7 tiles leaves two per
        # split: each split then ends 7 units above its reference, P up to 2^7 -- the named property there is "no move", exact above)
        if (pattern in ("stair9", "over", "spike_query") or (pattern == "stair7" and (kern == "wide" or per_t >= 3))
                or (pattern == "under" and kern == "wide")):
            assert nexp > 0, "pattern %s with ksplit = %d names no move at all: the case misses its branch" % (pattern, ksplit)
        if pattern in ("under", "descending", "offset") and kern == "dma":
            assert nmoves == 0, have
        if pattern in ("under", "over"):          # the key sits 7.5 / 8.5 above the reference its split started from, and not in that first tile
            j = mid + 37
            lo = j // bkv // per_t * per_t
            assert j // bkv > lo, "the key sits in the first tile of its split"
            gap = L[..., j] - L[..., lo * bkv:(lo + 1) * bkv].max(-1).values
            # (against the noisy maximum of that first tile, up to ~0.5 above its level: under stays a large P below the threshold)
            assert (6.5 < float(gap.min()) and float(gap.max()) < 8.0) if pattern == "under" else float(gap.max()) > 8.0, (float(gap.min()), float(gap.max()))
        if pattern == "spike_query":              # exactly one query per (batch, head) is lifted, by 30 units
            for (b, h, i, j) in spike:
                lift = L[b, h, :, j] - L[b, h, :, (j + 1) % tk]
                assert float(lift[i]) > 29.0 and int((lift > 1.0).sum()) == 1
        if pattern == "split_place":              # the dominant key visits every non-empty split in turn, the first included
            hit = {min(j // bkv // per_t, S - 1) for (_, _, _, j) in events}
            assert hit == {s_ for s_ in range(S) if s_ * per_t < ntile}, (hit, S, per_t, ntile)
        if pattern == "split_far" and ksplit:     # the splits' references differ by what the pattern says
            m_s = torch.stack([L[..., s_ * per_t * bkv:(s_ + 1) * per_t * bkv].max(-1).values for s_ in range(S) if s_ * per_t * bkv < tk], -1)
            assert float((m_s.max(-1).values - m_s.min(-1).values).min()) > 60.0
            if ksplit == 2:
                assert nmoves == 0 or kern == "wide", have     # 3 + 3 tiles: each split is flat, the 70 units meet in the merge
        print("[numerics] attention_scores %s %s d%d ksplit=%d QF=%d shift=%+.0f tq%d tk%d: %d reference moves over %d (wave, split) pairs; (b0 h0 wave0): %s"
              % (pattern, str(dtype).split(".")[-1], d, ksplit, qf, shift, tq, tk, nmoves, len(have), first))
        got = run_attention(lib, device, dtype, q, k, v, heads=heads, d=d, scale=LN2, ksplit=ksplit)
        what = "%s d%d ksplit=%d QF=%d shift=%+.0f" % (pattern, d, ksplit, qf, shift)
        attention_numerics(got, q, k, v, heads=heads, d=d, scale=LN2, dtype=dtype, causal=False, ksplit=ksplit, what=what)
        outs.append((got, q, k))
    if pattern == "offset":        # shift invariance: same fp64 reference, so two runs differ by at most the sum of their bounds
        O64, A, _, T0 = attention_ref64(outs[0][1], outs[0][2], v, heads=heads, d=d, scale=LN2, dtype=dtype)
        for (got, q, k) in outs[1:]:
            O2, A2, _, T = attention_ref64(q, k, v, heads=heads, d=d, scale=LN2, dtype=dtype)
            assert (O2 - O64).abs().max() <= 1e-9 * A.max(), "the shift is not exact in the operands"
            vmax = float(v.float().abs().max())
            b2 = attention_bound(dtype, d, tk, ksplit, A, T0, vmax) + attention_bound(dtype, d, tk, ksplit, A, T, vmax)
            diff = (got.double() - outs[0][0].double()).view(batch, tq, heads, d).transpose(1, 2).abs() / (A + 1e-300)
            assert float((diff / b2).max()) <= 1.0, "attention is not shift invariant within its bound"
    return qf


def check_boundary(lib, device, dtype, *, n=2, h=6, w=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, h, w, generator=g)
    y = torch.full((n, h, w, 8), float("nan"), dtype=dtype, device=device)
    opcode, p = O.nchw_to_nhwc(x.to(device), y, n=n, c=3, h=h, w=w, cpad=8, mul=2.0, add=-1.0)
    run_op(lib, opcode, p, dtype, device)
    ref = nhwc(x * 2 - 1, dtype)
    assert torch.equal(y.cpu().float(), ref.float())
    # back
    t = (torch.randn(n, h, w, 8, generator=g) * 1.5).to(dtype)
    out = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=device)
    opcode, p = O.nhwc_to_nchw(t.to(device), out, n=n, c=3, h=h, w=w, ldx=8, clamp=1)
    run_op(lib, opcode, p, dtype, device)
    assert torch.equal(out.cpu(), t.float()[..., :3].permute(0, 3, 1, 2).clamp(-1, 1))
    return 0.0


def check_latent_ops(lib, device, dtype, *, n=2, h=4, w=6, seed=0, r=0.4):
    g = torch.Generator().manual_seed(seed)
    hw, lat = h * w, 4
    moments = torch.randn(n, 2 * lat, h, w, generator=g)
    eps = torch.randn(n, lat, h, w, generator=g)
    noise = torch.randn(1, lat, h, w, generator=g)
    mean, logvar = moments.chunk(2, 1)
    z = (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * eps) * 0.18215
    u_ref = z * r + noise * (1 - r)
    md = moments.permute(0, 2, 3, 1).contiguous().to(device)  # fp32 NHWC moments
    u = torch.full((n, hw, 8), float("nan"), dtype=dtype, device=device)
    u32 = torch.full((n, hw, lat), float("nan"), device=device)
    opcode, p = O.posterior(md, eps.to(device), u, n=n, hw=hw, lat=lat, ldm=2 * lat, ldu=8, sf=0.18215, r=r,
                            noise=noise.to(device), noise_n=1, u_f32=u32, moments_f32=1)
    run_op(lib, opcode, p, dtype, device)
    ref_nhwc = u_ref.permute(0, 2, 3, 1).reshape(n, hw, lat)
    assert rel_err(u32.cpu(), ref_nhwc) < 1e-5
    assert rel_err(u.cpu()[..., :lat], ref_nhwc) < TOL[dtype]
    assert (u.cpu().float()[..., lat:] == 0).all()
    # ddpm + post_quant
    e = torch.randn(n, hw, lat, generator=g)
    wpq = torch.randn(lat, lat, generator=g) * 0.5
    bpq = torch.randn(lat, generator=g) * 0.1
    sa, s1 = 0.06826489, 0.99766723
    x0 = (ref_nhwc - s1 * e) / sa / 0.18215
    ref = x0 @ wpq.t() + bpq
    y = torch.full((n, hw, 8), float("nan"), dtype=dtype, device=device)
    opcode, p = O.ddpm_postquant(u32, e.to(device), y, wpq.to(device), bpq.to(device), n=n, hw=hw, lat=lat, ldu=lat, lde=lat, ldy=8,
                                 sqrt_abar=sa, sqrt_1m_abar=s1, sf=0.18215, u_f32=1, e_f32=1)
    run_op(lib, opcode, p, dtype, device)
    err = rel_err(y.cpu()[..., :lat], ref)
    assert err < max(TOL[dtype], 1e-4) and (y.cpu().float()[..., lat:] == 0).all()
    return err


def check_conv_gn_part(lib, device, dtype, *, n=2, cin=64, cout=64, h=16, w=16, groups=8, tile=10, res=True, seed=0, subpix=False,
                       ks=3, stride=1, skip_if_declined=False):
    """3x3 conv whose epilogue emits the GroupNorm partial sums of its OUTPUT (gn_part), finished by
    gn_stats(finalize_only): the (scale, shift) pairs must match statistics taken from the stored tensor."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, ks, ks, generator=g) / math.sqrt(cin * ks * ks)
    b = torch.randn(cout, generator=g) * 0.1
    r = torch.randn(n, cout, h // stride, w // stride, generator=g) if res else None
    gamma = 1 + 0.1 * torch.randn(cout, generator=g)
    beta = 0.1 * torch.randn(cout, generator=g)
    x0 = nhwc(x, dtype).to(device)
    wp = pack_conv_weight(wt, dtype).to(device)
    ho, wo = (2 * h, 2 * w) if subpix else (h // stride, w // stride)
    if subpix:      # Upsample2D in sub-pixel form: the partial sums cover the 2h x 2w OUTPUT, four parity workgroups per tile
        from img2img_turbo_amd.packer import subpixel_weights
        wp = subpixel_weights(wt).reshape(4 * cout, 4 * cin).to(dtype).contiguous().to(device)
        r = torch.randn(n, cout, ho, wo, generator=g) if res else None
    out = torch.full((n, ho, wo, cout), float("nan"), dtype=dtype, device=device)
    rd = nhwc(r, dtype).to(device) if res else None
    bdev = b.to(device)      # keep alive: the op only holds raw pointers
    opcode, p = O.conv(x0, wp, out, nimg=n, hin=h, win=w, ho=ho, wo=wo, ks=ks, stride=stride, pad=ks // 2, ups=1 if subpix else 0, N=cout, bias=bdev,
                       res=rd, tile=tile, subpix=1 if subpix else 0)
    parts = lib.igemm_gn_parts(p, O.DT[dtype], groups)
    if parts == 0 and skip_if_declined:
        import pytest
        pytest.skip("this build of the library does not emit GroupNorm partials for this op (compile-time gated feature)")
    assert parts > 0, "kernel declined GroupNorm partials"
    part = torch.full((n * parts * groups * 2,), float("nan"), device=device)
    p.gn_part, p.gn_part_groups = part.data_ptr(), groups
    ss = torch.full((n, cout, 2), float("nan"), device=device)
    gd, bd = gamma.to(device), beta.to(device)
    op2, p2 = O.gn_stats(None, gd, bd, part, ss, nimg=n, hw=ho * wo, groups=groups, eps=1e-5, nparts=parts, c0=cout, ld0=cout, finalize_only=1)
    prog = K.Program()
    prog.add(opcode, O.DT[dtype], p)
    prog.add(op2, O.DT[dtype], p2)
    prog.freeze()
    lib.run(prog, torch.cuda.current_stream().cuda_stream if device != "cpu" else 0)
    if device != "cpu":
        torch.cuda.synchronize()
    stored = out.cpu().float().permute(0, 3, 1, 2)
    ref = gn_scale_shift(stored, groups, gamma, beta, 1e-5)
    err = rel_err(ss.cpu(), ref)
    assert err < 2e-4, f"fused gn stats rel err {err}"
    return err


def check_u8_boundary(lib, device, dtype, *, n=2, h=6, w=10, seed=0):
    """uint8 HWC <-> NHWC with the callers' pre/post-processing folded in (to_tensor / Normalize / x*0.5+0.5 / ToPILImage)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    y = torch.full((n, h, w, 8), float("nan"), dtype=dtype, device=device)
    imgd = img.to(device)
    opcode, p = O.nchw_to_nhwc(imgd, y, n=n, c=3, h=h, w=w, cpad=8, mul=2.0, add=-1.0)
    run_op(lib, opcode, p, dtype, device)
    ref = (img.float() / 255.0) * 2.0 - 1.0
    got = y.cpu().float()
    assert (got[..., 3:] == 0).all()
    assert (got[..., :3] - ref.to(dtype).float()).abs().max() <= (1e-6 if dtype == torch.float32 else 8e-3)
    # the sketch script's binarisation F.to_tensor(img) < 0.5 (src/inference_paired.py:57-58): exact, every byte value
    ramp = torch.arange(256, dtype=torch.uint8).repeat(n * h * w * 3 // 256 + 1)[: n * h * w * 3].reshape(n, h, w, 3).contiguous()
    rampd = ramp.to(device)
    yb = torch.full((n, h, w, 8), float("nan"), dtype=dtype, device=device)
    opcode, p = O.nchw_to_nhwc(rampd, yb, n=n, c=3, h=h, w=w, cpad=8, binarize_below=128)
    run_op(lib, opcode, p, dtype, device)
    assert torch.equal(yb.cpu().float()[..., :3], ((ramp.float() / 255.0) < 0.5).float()) and (yb.cpu().float()[..., 3:] == 0).all()
    # output side: values on an exact 1/255 grid survive the round trip bit for bit in fp32
    x = torch.zeros(n, h, w, 8)
    x[..., :3] = ref
    x = x * 1.0
    xd = x.to(dtype).to(device)
    out = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=device)
    opcode, p = O.nhwc_to_nchw(xd, out, n=n, c=3, h=h, w=w, ldx=8, clamp=1, mul=0.5, add=0.5)
    run_op(lib, opcode, p, dtype, device)
    exp = ((xd.cpu().float()[..., :3].clamp(-1, 1) * 0.5 + 0.5).clamp(0, 1) * 255.0).to(torch.uint8)
    assert (out.cpu().int() - exp.int()).abs().max() <= (0 if dtype == torch.float32 else 1)


LN_RMS_GATE, LN_MAX_GATE = 1.25, 1.5          # the project's floor gates (tests/test_e2e_gpu.py RMS_GATE, MAX_GATE)


def check_ln_gemm(lib, device, dtype, *, rows=200, cin=128, nq=160, nv=0, geglu=False, tile=52, lora_rank=4, r=0.7, seed=0, offset=0.0,
                  mu_sigma=None, gate=True, flat=False, col0=None):
    """LayerNorm folded into the wide GEMM (i2i_igemm_params.ln_cs) together with the device-side merge that prepares its operands
    (i2i_lora_merge_params.kscale ..): out = F.linear(F.layer_norm(x), W + r B.A, b) from the UN-normalised rows, `nv` further
    output columns written transposed (the V^T of a self-attention block), or the GEGLU form.  Reference: plain fp32 torch on the
    rounded inputs, LayerNorm output NOT rounded (the kernel never materialises it).

    mu_sigma (a number, or a tensor tiled over the rows: both signs and offset 0 in one launch): the rows sit on a DC offset of that
    many standard deviations -- mu^2 / var = mu_sigma^2, the cancellation hazard of the one-pass var = E[x^2] - mu^2 and of
    rstd (acc - mu colsum).  Gate: a FLOOR.  Exact = fp64 LayerNorm of the rounded rows times the STORED weights, plus the stored
    bias.  Floor = the error, against exact, of the unfused pair the planner falls back to, emulated in plain torch:
    round_T(LayerNorm64(x)) times the stored weights in fp64, plus bias, rounded to T.  Per |offset| value the kernel's RMS error must
    be <= 1.25 x the floor's and its max-abs error <= 1.5 x the floor's (gate=False: print only).

    col0 (with mu_sigma): the fp16 kernel shifts its sums by a pivot p, the MEDIAN of the row's first, middle and last element
    (columns 0, K/2, K-1); a pivot r sigma from the mean leaves the sums as exposed as plain ones at an offset of r sigma.
      "zero" / "outlier"    column 0 of every row is overwritten, by 0 or by an outlier 30 of the other elements' standard deviations
                            above them: the median ignores it.  Same floor, same gates.
      "zero2" / "outlier2"  columns 0 AND K/2: the median IS the overwritten value now, the pivot unrepresentative.  It is still an
                            element of the row, (p - mu)^2 <= sum_k (x_k - mu)^2 = K var: the sums never see more than sqrt(K) sigma
                            (36 at K = 1280), the row's own variance growing with the outliers.  Call it with gate=False for fp16:
                            measured and printed beside the floor like the offsets beyond the supported range (a worst-case bound
                            of the fp32 sums, 1.5 (K/4 + 4) 2^-24 (1 + r^2) of rstd, is 100 x what is measured and pins nothing);
                            finite output is asserted.  bf16 takes plain sums whatever the pivot and keeps the gates.

    flat (plain and transposed forms): the rows are CONSTANT, x[m][:] = 1.3 mu_sigma[m] -- variance exactly 0, so the one-pass
    E[x^2] - mu^2 is pure fp32 rounding of either sign (the fmaxf(var, 0) of the epilogue; a negative variance under eps = 1e-5 would
    be rsqrt of a negative number).  LayerNorm of a constant row is 0, the exact output is the folded bias.  No floor applies (the
    unfused pair is exact here), the bound is derived instead: rstd <= eps^-1/2 multiplies what is left of acc - mu colsum, two fp32
    contractions of K terms of size |mu| |w_k| each:  |got - bias'| <= u |bias'| + eps^-1/2 * 2 (K + 2) 2^-24 |mu| sum_k |w_nk|.
    (A worst-case bound, linear in K; what it pins is that the output stays finite and of the size of that noise.)"""
    g = torch.Generator().manual_seed(seed)
    N = nq + nv
    if mu_sigma is None:
        x = (torch.randn(rows, cin, generator=g) * 1.3 + offset + 0.2 * torch.randn(rows, 1, generator=g)).to(dtype)
    else:
        row_off = _row_offset(mu_sigma, rows)
        x = (torch.randn(rows, cin, generator=g) * (0.0 if flat else 1.0) + row_off[:, None]) * 1.3
        if col0 is not None:
            for col in ((0,) if col0 in ("zero", "outlier") else (0, cin // 2)):
                x[:, col] = torch.zeros(rows) if col0.startswith("zero") else (row_off + 30.0) * 1.3
        x = x.to(dtype)
    W = torch.randn(N, cin, generator=g) / math.sqrt(cin)
    b = torch.randn(N, generator=g) * 0.1
    A = torch.randn(lora_rank, cin, generator=g) / math.sqrt(cin)
    Bm = torch.randn(N, lora_rank, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(cin, generator=g)
    beta = 0.2 * torch.randn(cin, generator=g)
    Wm = W + r * (Bm @ A)
    if geglu:
        half = N // 2
        idx = torch.arange(half).reshape(-1, 16)
        idx = torch.cat([idx, idx + half], 1).reshape(-1)
        Wp, bp, Bp = W[idx], b[idx], Bm[idx]
    else:
        Wp, bp, Bp = W, b, Bm
    dev = lambda t, dt=torch.float32: t.to(dt).contiguous().to(device)
    wd = torch.zeros(N, cin, dtype=dtype, device=device)
    cs = torch.full((N,), float("nan"), device=device)
    bout = torch.full((N,), float("nan"), device=device)
    rg = dev(torch.tensor([r, 1.0]))
    mp = K.LoraMergeParams()
    keep = [dev(Wp), dev(A), dev(Bp), dev(gamma), dev(beta), dev(bp)]
    mp.dst, mp.w0, mp.a, mp.b, mp.N, mp.K, mp.rank, mp.use_gamma, mp.rg = wd.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), N, cin, lora_rank, 0, rg.data_ptr()
    mp.kscale, mp.kshift, mp.bias0, mp.colsum, mp.bias_out = keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), cs.data_ptr(), bout.data_ptr()
    run_op(lib, K.OP_LORA_MERGE, mp, dtype, device)
    # the merge: stored weights = cvt(W' * gamma), colsum of the STORED values, bias' = b + W'.beta
    wq = (Wm * gamma[None]).to(dtype)
    wref = wq[idx] if geglu else wq
    assert rel_err(wd.cpu(), wref) < (1e-6 if dtype == torch.float32 else 1e-2), "ln-fold merge: weights"
    assert rel_err(cs.cpu(), wd.cpu().float().sum(1)) < 1e-5, "ln-fold merge: column sums"
    bref = b + Wm @ beta
    assert rel_err(bout.cpu(), bref[idx] if geglu else bref) < 1e-5, "ln-fold merge: bias"
    # the GEMM
    xd = x.to(device)
    n_out = N // 2 if geglu else nq
    out = torch.full((rows, n_out), float("nan"), dtype=dtype, device=device)
    out2 = torch.full((max(nv, 1), rows), float("nan"), dtype=dtype, device=device)
    opcode, p = O.conv(xd, wd, out, nimg=1, hin=1, win=rows, ho=1, wo=rows, ks=1, c0=cin, lda0=cin, N=N, bias=bout, ldc=n_out, geglu=int(geglu), tile=tile)
    p.ln_cs, p.ln_eps = cs.data_ptr(), 1e-5
    if nv:
        p.n_trans, p.c2, p.ldc2 = nq, out2.data_ptr(), rows
    assert lib.igemm_route(p, O.DT[dtype]) == "gemm_w32_kernel"
    run_op(lib, opcode, p, dtype, device)
    x64 = x.double()
    xn64 = (x64 - x64.mean(1, keepdim=True)) * torch.rsqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-5)      # LayerNorm64 without the affine: gamma rides in the stored weights, beta in the bias
    unpack = (lambda t: t.index_copy(1, idx, t)) if geglu else (lambda t: t)      # GEGLU: the stored rows are interleaved (idx); back to [a | gate]
    full64 = unpack(xn64 @ wd.cpu().double().T + bout.cpu().double()[None])        # exact for the floor gates: the STORED operands (the merge's outputs, checked above)
    full = unpack(xn64 @ wref.double().T + (bref[idx] if geglu else bref).double()[None]).float()      # the historic rel_err gate keeps host-side operands: independent of the merge
    if geglu:
        ref = full[:, :half] * F.gelu(full[:, half:])
        err = rel_err(out.cpu(), ref)
    else:
        err = rel_err(out.cpu(), full[:, :nq])
        if nv:
            err = max(err, rel_err(out2.cpu(), full[:, nq:].T))
    # (gate=False: the measure-only offsets beyond the supported range; flat: rstd = eps^-1/2 amplifies fp32 noise, bounded below)
    assert err < TOL[dtype] or not gate or flat, f"ln gemm rel err {err}"
    if flat:
        assert not geglu
        got = torch.cat([out.cpu().double(), out2.cpu().double().T], 1) if nv else out.cpu().double()
        assert torch.isfinite(got).all(), "LayerNorm fold: non-finite output on a constant row"
        bound = U[dtype] * full64.abs() + 1e-5 ** -0.5 * 2 * (cin + 2) * EPS32 * x64[:, :1].abs() * wd.cpu().double().abs().sum(1)[None]
        bound = bound + (2.0 ** -25 if dtype == torch.float16 else 0.0)          # fp16 outputs below 2^-14 are subnormal: half a step of 2^-24
        ratio = ((got - full64).abs() / (bound + 1e-300)).max().item()
        print("[numerics] ln_gemm %s cin=%d constant rows: max |err|/bound = %.3f" % (str(dtype).split(".")[-1], cin, ratio))
        assert ratio <= 1.0, f"LayerNorm fold on constant rows: error {ratio:.3f} x its bound"
    elif mu_sigma is not None:
        floor_full = unpack(xn64.to(dtype).double() @ wd.cpu().double().T + bout.cpu().double()[None])
        if geglu:
            fin = lambda t: t[:, :half] * F.gelu(t[:, half:])
            exact, floor, got = fin(full64), fin(floor_full).to(dtype).double(), out.cpu().double()
        else:
            exact, floor = full64, floor_full.to(dtype).double()
            got = torch.cat([out.cpu().double(), out2.cpu().double().T], 1) if nv else out.cpu().double()
        assert torch.isfinite(got).all()
        for val in sorted(set(row_off.abs().tolist())):
            sel = row_off.abs() == val
            ek, ef = (got - exact)[sel], (floor - exact)[sel]
            rk, rf = ek.pow(2).mean().sqrt().item(), ef.pow(2).mean().sqrt().item()
            mk, mf = ek.abs().max().item(), ef.abs().max().item()
            print("[numerics] ln_gemm %s cin=%d %s tile=%d |mu/sigma|=%g: kernel rms %.3e max %.3e | floor rms %.3e max %.3e | ratio rms %.3f max %.3f%s"
                  % (str(dtype).split(".")[-1], cin, ("geglu" if geglu else ("q|k|vT" if nv else "plain")) + (" col0=" + col0 if col0 else ""), tile, val, rk, mk, rf, mf, rk / rf, mk / mf,
                     "" if gate else "  (measured, not gated)"))
            if gate:
                assert rk <= LN_RMS_GATE * rf and mk <= LN_MAX_GATE * mf, \
                    f"LayerNorm fold at |mu/sigma| = {val}: rms {rk:.3e} vs floor {rf:.3e}, max {mk:.3e} vs floor {mf:.3e}"
    return err

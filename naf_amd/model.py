"""NAF upsampler module: the reference's public operator (``naf(image, lr_features, target_size)``)
on MI355X-native kernels.

Mirrors the reference's module tree so that ``state_dict`` keys, constructor arguments and the
attributes callers read are identical (src/model/naf.py:72-116, src/layers/convolutions.py:6-92,
src/layers/rope.py:39-83, src/layers/attentions.py:32-47):

    NAF.image_encoder.encoder / .sem_encoder    nn.Sequential(Conv2d, EncBlock, ...)  (1x1 / 3x3-reflect)
    NAF.image_encoder.rope.periods              persistent buffer [D_head / 4]
    NAF.query_encoder, NAF.key_encoder          parameter-free
    NAF.upsampler.kernel_size / .num_heads / .scale / .dilation

The forward pass differs in HOW, not WHAT:
  * K/V are never upsampled to the output grid and the score tensor is never materialised
    (attentions.py:60-61,20-23 do both);
  * RoPE, the identity query encoder and the key pooling are one HIP pass (naf_rope_pool_fwd);
  * attention runs in the fused HIP kernel (naf_xna_fwd): MFMA cell kernel for integer ratios,
    table-driven kernel otherwise and for ``return_weights``.
Contract: bf16 queries/keys/values, fp32 softmax and accumulation; the output dtype follows
``features`` (bf16 -> bf16, anything else -> fp32) and is returned as a logical [B, C, Ho, Wo]
view of a channels-last buffer -- the same view the reference returns on its fused NATTEN path
(attentions.py:75).  Inputs must live on a ROCm device; there is no CPU path.
"""
from __future__ import annotations

import collections
import math
import os

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import ops


class EncBlock(nn.Module):
    """GroupNorm(8) -> SiLU -> Conv -> GroupNorm(8) -> SiLU -> Conv, reflect padding, no skip
    (convolutions.py:6-64 with residual=False, in == out channels so no shortcut conv exists)."""

    def __init__(self, channels: int, kernel_size: int, num_groups: int = 8, bias: bool = True):
        super().__init__()
        pad = kernel_size // 2
        self.norm1 = nn.GroupNorm(num_groups, channels)
        self.conv1 = nn.Conv2d(channels, channels, kernel_size, padding=pad, padding_mode="reflect", bias=bias)
        self.norm2 = nn.GroupNorm(num_groups, channels)
        self.conv2 = nn.Conv2d(channels, channels, kernel_size, padding=pad, padding_mode="reflect", bias=bias)


def make_branch(in_dim: int, hidden: int, kernel_size: int, ks_res: int, num_layers: int) -> nn.Sequential:
    """Same parameter layout as the reference's ``encoder(...)`` (convolutions.py:67-92)."""
    return nn.Sequential(
        nn.Conv2d(in_dim, hidden, kernel_size, padding=kernel_size // 2, padding_mode="reflect", bias=True),
        *[EncBlock(hidden, ks_res) for _ in range(num_layers)],
    )


class RoPE(nn.Module):
    """Holds the `periods` buffer (rope.py:77-81,128-135) and caches the device sin/cos tables per
    output size, like the reference caches coordinates per (H, W) (rope.py:159-161).  ``tables`` are the deterministic
    eval-mode tables the HIP kernels read; ``train_tables`` adds the train-time coordinate augmentation (shift / jitter /
    rescale, rope.py:107-124) for ``NAF.forward_train`` when the module is in training mode."""

    def __init__(self, embed_dim: int, num_heads: int, base: float = 100.0, rescale_coords: Optional[float] = None):
        super().__init__()
        if embed_dim % (4 * num_heads):
            raise AssertionError("embed_dim must be divisible by 4 * num_heads")
        self.num_heads = num_heads
        self.base = base
        self.D_head = embed_dim // num_heads
        self.rescale_coords = rescale_coords
        self.shift_coords = None          # rope.py:49-51: not set by NAF (naf.py:29), kept for parity of the attribute set
        self.jitter_coords = None
        d = self.D_head
        periods = base ** (2 * torch.arange(d // 4, dtype=torch.float32) / (d // 2))
        self.register_buffer("periods", periods, persistent=True)
        self._tables = None
        self._tables_key = None
        # train-time coordinate augmentation (rope.py:107-124): the reference caches the coordinates per (H, W)
        # (rope.py:159-161), so its augmentation is drawn ONCE per resolution and even survives .eval(); the default here
        # redraws it on every training step (what the augmentation is for).  Set True to reproduce the reference's caching.
        self.cache_train_coords = False
        self._train_tables = {}

    def tables(self, Ho: int, Wo: int):
        p = self.periods
        key = (Ho, Wo, str(p.device), p.data_ptr(), p._version)
        if key != self._tables_key:
            self._tables = ops.rope_tables(p, Ho, Wo)
            self._tables_key = key
        return self._tables


def _rope_train_tables(rope: "RoPE", Ho: int, Wo: int):
    """cos / sin tables [Ho, 2, P], [Wo, 2, P] like ops.rope_tables, with the reference's train-time augmentation of the
    coordinates (rope.py:107-124): one uniform shift per axis, one log-uniform jitter per axis, one log-uniform rescale for
    both, drawn per call while ``rope.training``.  'separate' normalisation (rope.py:98-100)."""
    import math
    p = rope.periods
    dev = p.device
    cy = 2.0 * (torch.arange(Ho, device=dev, dtype=torch.float32) + 0.5) / Ho - 1.0
    cx = 2.0 * (torch.arange(Wo, device=dev, dtype=torch.float32) + 0.5) / Wo - 1.0
    if rope.training and rope.shift_coords is not None:
        sh = torch.empty(2, device=dev).uniform_(-rope.shift_coords, rope.shift_coords)
        cy, cx = cy + sh[0], cx + sh[1]
    if rope.training and rope.jitter_coords is not None:
        j = torch.empty(2, device=dev).uniform_(-math.log(rope.jitter_coords), math.log(rope.jitter_coords)).exp()
        cy, cx = cy * j[0], cx * j[1]
    if rope.training and rope.rescale_coords is not None:
        r = torch.empty(1, device=dev).uniform_(-math.log(rope.rescale_coords), math.log(rope.rescale_coords)).exp()
        cy, cx = cy * r, cx * r
    ay = (2.0 * math.pi * cy)[:, None] / p[None, :]                                   # rope.py:139
    ax = (2.0 * math.pi * cx)[:, None] / p[None, :]
    return torch.stack([ay.cos(), ay.sin()], dim=1), torch.stack([ax.cos(), ax.sin()], dim=1)


class _GroupNormTrain(torch.autograd.Function):
    """GroupNorm for the training stem.  ATen's ROCm forward computes the statistics with one workgroup per
    (sample, group) -- 8 workgroups at batch 1, 2.1 ms per layer at 448^2 (profiles/r01_train_step.txt).  Here the
    moments are a per-channel reduction over the channels-last rows ([HW, C]: C outputs, parallel over HW) folded
    into groups on [B, C] values; the normalisation is one fused multiply-add; the backward is ATen's own
    native_group_norm_backward (0.25 ms), fed with the saved mean / rstd."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps):
        B, C, H, W = x.shape
        xv = x.permute(0, 2, 3, 1).reshape(B, H * W, C).float()                       # rows of C contiguous channels (a view
        HW = H * W                                                                    # for channels-last input), fp32 statistics
        S = next((d for d in (512, 256, 128, 64, 32, 16) if HW % d == 0 and HW // d >= 8), 0)
        if C >= 96 or S == 0:
            var_c, mean_c = torch.var_mean(xv, dim=1, unbiased=False)                 # [B, C], Welford
        else:
            # few channels = few outputs: ATen's column reduction then runs on a handful of workgroups (0.3 ms for 48
            # channels at 256^2); reduce in two stages, S partial sums per channel first -- mean, then CENTRED squares
            mean_c = xv.view(B, S, HW // S, C).sum(2).sum(1) / HW
            dc = xv - mean_c.unsqueeze(1)
            var_c = (dc * dc).view(B, S, HW // S, C).sum(2).sum(1) / HW
        # fold channels into groups without E[x^2] - mean^2 (activations with |mean| >> std would lose every variance
        # bit): var_g = mean_c(var_c) + mean_c((mean_c - mean_g)^2), both terms non-negative
        mean_cg = mean_c.view(B, groups, -1)
        mean = mean_cg.mean(-1)                                                        # [B, G]
        var = var_c.view(B, groups, -1).mean(-1) + ((mean_cg - mean.unsqueeze(-1)) ** 2).mean(-1)
        rstd = torch.rsqrt(var + eps)
        scale = (rstd.unsqueeze(-1) * weight.float().view(groups, -1)).reshape(B, C)
        shift = bias.float().unsqueeze(0) - (mean.unsqueeze(-1) * scale.view(B, groups, -1)).reshape(B, C)
        ctx.save_for_backward(x, mean, rstd, weight)
        ctx.groups = groups
        return torch.addcmul(shift.view(B, C, 1, 1).to(x.dtype), x, scale.view(B, C, 1, 1).to(x.dtype))

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, weight = ctx.saved_tensors
        B, C, H, W = x.shape
        # ATen's kernel indexes dense NCHW memory (autograd hands it grad.contiguous() as well)
        # (and one dtype: under autocast x / dy arrive in bf16 while the statistics and the affine parameters are fp32)
        dx, dw, db = torch.ops.aten.native_group_norm_backward(dy.float().contiguous(), x.float().contiguous(), mean, rstd,
                                                               weight.float(), B, C, H * W, ctx.groups, [True, True, True])
        return dx.to(x.dtype).contiguous(memory_format=torch.channels_last), dw.to(weight.dtype), db.to(weight.dtype), None, None


class _ReflectPad(torch.autograd.Function):
    """F.pad(mode="reflect") whose backward folds the border strips back with slice adds (ATen's
    reflection_pad2d_backward is a scalar atomic kernel: 0.85 ms per layer at 448^2 on gfx950)."""

    @staticmethod
    def forward(ctx, x, pad):
        ctx.pad = pad
        return F.pad(x, (pad, pad, pad, pad), mode="reflect")

    @staticmethod
    def backward(ctx, g):
        p = ctx.pad
        H, W = g.shape[-2] - 2 * p, g.shape[-1] - 2 * p
        gx = g[..., :, p:p + W].clone()                                   # columns first: [.., H + 2p, W]
        gx[..., :, 1:p + 1] += g[..., :, :p].flip(-1)                     # left strip mirrors columns 1..p
        gx[..., :, W - 1 - p:W - 1] += g[..., :, p + W:].flip(-1)         # right strip mirrors columns W-1-p..W-2
        out = gx[..., p:p + H, :].clone()
        out[..., 1:p + 1, :] += gx[..., :p, :].flip(-2)
        out[..., H - 1 - p:H - 1, :] += gx[..., p + H:, :].flip(-2)
        return out, None


def _stem_layers(seq: nn.Sequential):
    """(norm, conv) pairs of a branch after its first convolution (convolutions.py:52-61: norm1 -> SiLU -> conv1, norm2 -> ...)."""
    out = []
    for blk in list(seq)[1:]:
        out += [(blk.norm1, blk.conv1), (blk.norm2, blk.conv2)]
    return out


class _HipStem(torch.autograd.Function):
    """Both branches of the conv stem (convolutions.py:67-92) as ONE differentiable op on the HIP kernels: the forward is the
    inference stem (naf_stem_conv0_fwd / naf_stem_conv_fwd, bf16 activations, fp32 accumulation, fp64 GroupNorm sums) with
    every layer's input kept; the backward walks the layers down with
      data gradient    naf_stem_conv_fwd in plain mode on the flipped / transposed weights (3x3: over the output gradient in a
                       2-pixel zero border, i.e. on the reflect-PADDED domain),
      norm + SiLU      naf_stem_act_bwd (folds the padded border back on load, returns the GroupNorm affine gradients),
      weight gradient  naf_stem_wgrad: a GEMM contracted over pixels (transposing LDS reads feed both MFMA operands), with
                       a = SiLU(GroupNorm(x)) recomputed in its loader.
    bf16 roundings of stored activations / gradients are treated as identities (as torch.autocast does for bf16 convolutions:
    this is the reference's use_bf16 training mode, train.py:120).  Every width the forward stem serves (round 6: hidden widths that
    are multiples of 16 up to 256 -- the reference's denoising models, denoising.py:209-220 -- through stem_generic.hip's plain
    convolution, stem_generic_bwd.hip's weight gradient and the width-general norm / first-convolution kernels of stem_bwd.hip)."""

    @staticmethod
    def forward(ctx, enc, image, *params):
        B, _, H, W = image.shape
        dev = image.device
        branches = (enc.encoder, enc.sem_encoder)
        hid = enc.encoder[0].out_channels
        nlayer = len(_stem_layers(enc.encoder))
        stats = ops.new_stats(B, dev, lead=(2, nlayer + 1))
        cat = torch.empty((B, H, W, 2 * hid), dtype=torch.bfloat16, device=dev)
        img = image.detach()
        if img.dtype not in (torch.float32, torch.bfloat16):
            img = img.float()
        saved = []
        for br, seq in enumerate(branches):
            conv0 = seq[0]
            ys = [torch.empty((B, H, W, hid), dtype=torch.bfloat16, device=dev) for _ in range(max(nlayer, 1))]
            dst = ys[0] if nlayer else cat[..., br * hid:(br + 1) * hid]
            ops.stem_conv0(img, conv0.weight.detach().float().contiguous(), conv0.bias.detach().float(), dst, stats[br, 0])
            for li, (norm, conv) in enumerate(_stem_layers(seq)):
                last = li == nlayer - 1
                dst = cat[..., br * hid:(br + 1) * hid] if last else ys[li + 1]
                ops.stem_conv(ys[li], stats[br, li], norm.weight.detach().float(), norm.bias.detach().float(), norm.eps,
                              enc._packed(conv), conv.bias.detach().float(), dst, None if last else stats[br, li + 1])
            saved.append(ys)
        # saved through autograd's own slots (version-counter checks, freed with the graph); the module is only consulted for its
        # layer structure and current parameter values
        ctx.save_for_backward(image, stats, *[y for ys in saved for y in ys])
        ctx.enc, ctx.nsaved, ctx.nparams = enc, [len(ys) for ys in saved], len(params)
        return cat.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        enc = ctx.enc
        image, stats, *flat = ctx.saved_tensors
        saved, pos = [], 0
        for n in ctx.nsaved:
            saved.append(flat[pos:pos + n])
            pos += n
        B, _, H, W = image.shape
        dev = g.device
        hid = enc.encoder[0].out_channels
        gcl = g.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()          # [B, H, W, 2 hid]; a no-op for a channels-last gradient
        grads = []
        dimage = None
        need_img = ctx.needs_input_grad[1]
        # every accumulator of the step -- weight / bias gradients (fp32 atomics) and the norm layers' sums (fp64 atomics) -- lives in ONE zeroed
        # buffer per dtype, and the sums are reduced over the batch once at the end (a memset, a reduction and two casts per LAYER before)
        branches = (enc.encoder, enc.sem_encoder)
        sizes = []
        for seq in branches:
            lay = _stem_layers(seq)
            kk, k0 = (lay[0][1].kernel_size[0] if lay else 1), seq[0].kernel_size[0]
            sizes.append([(3 * k0 * k0 + 1) * hid] + [kk * kk * hid * hid + hid] * len(lay))
        acc32 = torch.zeros((sum(sum(z) for z in sizes),), dtype=torch.float32, device=dev)
        nl_max = max(len(z) - 1 for z in sizes)
        acc64 = torch.zeros((2, max(nl_max, 1), B, hid, 2), dtype=torch.float64, device=dev)
        pos32 = 0
        for br, seq in enumerate(branches):
            ys = saved[br]
            layers = _stem_layers(seq)
            k = layers[0][1].kernel_size[0] if layers else 1
            out0 = acc32[pos32:pos32 + sizes[br][0]]
            pos32 += sizes[br][0]
            outs = []
            for z in sizes[br][1:]:
                outs.append(acc32[pos32:pos32 + z])
                pos32 += z
            # 3x3 branch: a layer's output gradient lives in the interior of a buffer with a 2-pixel ZERO border (what the
            # data-gradient convolution of the padded domain reads); naf_stem_act_bwd writes the next one straight into
            # the other buffer's interior, so only the branch's incoming gradient is ever copied
            ext = [torch.zeros((B, H + 4, W + 4, hid), dtype=torch.bfloat16, device=dev) for _ in range(2)] if k == 3 else None
            if k == 3:
                gl = ext[0][:, 2:H + 2, 2:W + 2]
                gl.copy_(gcl[..., br * hid:(br + 1) * hid])
            else:
                gl = gcl[..., br * hid:(br + 1) * hid]
            bgrads = []
            for li in range(len(layers) - 1, -1, -1):
                norm, conv = layers[li]
                w = conv.weight.detach()
                gw, gb = norm.weight.detach().float(), norm.bias.detach().float()
                # weight / bias gradient: naf_stem_wgrad (pixel-contraction GEMM; a = SiLU(GroupNorm(x)) recomputed in its loader)
                dw, db = ops.stem_wgrad(gl, ys[li], stats[br, li], gw, gb, norm.eps, k, with_bias=True, out=outs[li])
                # data gradient: the same conv kernel, plain, on the flipped / transposed weights
                wt = ops.pack_conv_weight(w.flip(2, 3).transpose(0, 1))
                if k == 3:
                    cur = (len(layers) - 1 - li) & 1
                    full = torch.empty_like(ext[cur])
                    ops.stem_conv_plain(ext[cur], wt, full)
                    dx = ext[cur ^ 1][:, 2:H + 2, 2:W + 2]
                    ops.stem_act_bwd(full[:, 1:H + 3, 1:W + 3], ys[li], stats[br, li], gw, gb, norm.eps, dx, fold=True, sums=acc64[br, li])
                    del full
                else:
                    da = torch.empty((B, H, W, hid), dtype=torch.bfloat16, device=dev)
                    ops.stem_conv_plain(gl, wt, da)
                    dx = torch.empty((B, H, W, hid), dtype=torch.bfloat16, device=dev)
                    ops.stem_act_bwd(da, ys[li], stats[br, li], gw, gb, norm.eps, dx, fold=False, sums=acc64[br, li])
                    del da
                bgrads.append((li, norm, dw.to(conv.weight.dtype), db.to(conv.bias.dtype)))
                gl = dx
            # first convolution (3 -> hid on the image): naf_stem_conv0_wgrad for the parameters and, when the image wants a
            # gradient, naf_stem_conv0_dgrad (round 6: no ATen / MIOpen convolution is left on the training path)
            conv0 = seq[0]
            dw0, db0 = ops.stem_conv0_wgrad(gl, image.detach(), conv0.kernel_size[0], out=out0)
            grads.append((br, dw0.to(conv0.weight.dtype), db0.to(conv0.bias.dtype), bgrads[::-1]))
            if need_img:
                if dimage is None:
                    dimage = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
                    ops.stem_conv0_dgrad(gl, conv0.weight.detach().float().contiguous(), dimage, accumulate=False)
                else:
                    ops.stem_conv0_dgrad(gl, conv0.weight.detach().float().contiguous(), dimage, accumulate=True)
        s32 = acc64.sum(2).float()      # [branch, layer, hid, {d bias, d weight}]: one reduction over the batch for every norm layer
        flat = []
        for br, dw0, db0, per_layer in grads:          # the order of _hip_stem_params
            flat += [dw0, db0]
            for li, norm, dw, db in per_layer:
                flat += [s32[br, li, :, 1].to(norm.weight.dtype), s32[br, li, :, 0].to(norm.bias.dtype), dw, db]
        grads = flat
        assert len(grads) == ctx.nparams
        return (None, dimage.to(image.dtype) if dimage is not None else None, *grads)


def _hip_stem_params(enc):
    """Parameters in the order _HipStem.backward returns their gradients."""
    out = []
    for seq in (enc.encoder, enc.sem_encoder):
        out += [seq[0].weight, seq[0].bias]
        for norm, conv in _stem_layers(seq):
            out += [norm.weight, norm.bias, conv.weight, conv.bias]
    return out


class ImageEncoder(nn.Module):
    """Guidance encoder (naf.py:11-52).  Both conv branches run through the library's fused HIP stem
    (naf_stem_conv0_fwd / naf_stem_conv_fwd: GroupNorm+SiLU+conv in one MFMA pass per layer): the hand-scheduled
    weight-stationary kernels at the default width (dim 256 -> 128 hidden channels), the general kernels of
    stem_generic.hip at any other width that is a multiple of 16 up to 256 (the reference's denoising models, dim 96 ... 512).
    ``stem_impl = "torch"`` (MIOpen ops in ``stem_dtype``) is an explicit A/B switch, never a silent fallback.
    RoPE is applied by the caller's fused rope+pool kernel."""

    def __init__(self, in_channels=3, out_channels=256, heads_rope=1, use_encoder=True, rope_base=None,
                 rope_rescale=None, img_layers=2):
        super().__init__()
        self.use_encoder = use_encoder
        self.out_channels = out_channels
        self.encoder = make_branch(in_channels, out_channels // 2, 1, 1, img_layers)
        self.sem_encoder = make_branch(in_channels, out_channels // 2, 3, 3, img_layers)
        self.rope = RoPE(out_channels, num_heads=heads_rope, base=rope_base, rescale_coords=rope_rescale)
        self.stem_dtype = torch.bfloat16
        self.stem_impl = "hip"      # "hip": fused HIP stem; "torch": MIOpen ops (A/B only)
        self.fuse_conv0 = True      # 1x1 branch: first block layer recomputes conv0 instead of reading it

    @staticmethod
    def _conv(x, conv: nn.Conv2d, dt):
        pad = conv.kernel_size[0] // 2
        if pad:
            x = F.pad(x, (pad, pad, pad, pad), mode="reflect")
        return F.conv2d(x, conv.weight.to(dt), None if conv.bias is None else conv.bias.to(dt))

    def _branch(self, x, seq: nn.Sequential, dt):
        x = self._conv(x, seq[0], dt)
        for blk in list(seq)[1:]:
            # (_GroupNormTrain: ATen's group_norm forward runs its statistics on B * groups workgroups, see its docstring)
            x = F.silu(_GroupNormTrain.apply(x, blk.norm1.weight, blk.norm1.bias, blk.norm1.num_groups, blk.norm1.eps))
            x = self._conv(x, blk.conv1, dt)
            x = F.silu(_GroupNormTrain.apply(x, blk.norm2.weight, blk.norm2.bias, blk.norm2.num_groups, blk.norm2.eps))
            x = self._conv(x, blk.conv2, dt)
        return x

    # ---- differentiable torch stem of forward_train ---------------------------------------------------
    # Same math as _branch (convolutions.py:52-92) with the three ops whose ATen ROCm kernels dominate a training
    # step at batch 1 replaced by equivalent compositions (profiles/r01_train_step.txt): GroupNorm statistics
    # (ATen launches one workgroup per (sample, group) = 8 workgroups: 2.1 ms per layer at 448^2), the reflect-pad
    # backward (0.85 ms per layer) and -- in forward_train -- the adaptive-average-pool backward (atomics, 2.6 ms).
    @staticmethod
    def _group_norm_train(x, norm: nn.GroupNorm):
        return _GroupNormTrain.apply(x, norm.weight, norm.bias, norm.num_groups, norm.eps)

    def _conv_train(self, x, conv: nn.Conv2d):
        pad = conv.kernel_size[0] // 2
        if pad:
            x = _ReflectPad.apply(x, pad)
        return F.conv2d(x, conv.weight, conv.bias)

    def _branch_train(self, x, seq: nn.Sequential):
        x = self._conv_train(x, seq[0])
        for blk in list(seq)[1:]:
            x = self._conv_train(F.silu(self._group_norm_train(x, blk.norm1)), blk.conv1)
            x = self._conv_train(F.silu(self._group_norm_train(x, blk.norm2)), blk.conv2)
        return x

    # ---- fused HIP stem (hidden width a multiple of 16 up to 256, GroupNorm(8)) --------------------
    def _hip_stem_ok(self) -> bool:
        c0 = self.encoder[0]
        return (self.use_encoder and c0.out_channels % 16 == 0 and 16 <= c0.out_channels <= 256 and c0.in_channels == 3
                and all(b.norm1.num_groups == 8 for b in list(self.encoder)[1:]))

    def _hip_stem_default_width(self) -> bool:
        return self._hip_stem_ok() and self.encoder[0].out_channels == 128

    def _hip_train_stem_ok(self) -> bool:
        """Widths ``_HipStem`` (forward with saved activations + HIP backward kernels) serves: all the forward stem does."""
        return self._hip_stem_ok()

    def _packed(self, conv: nn.Conv2d) -> torch.Tensor:
        """``ops.pack_conv_weight`` of a conv weight (bf16, the order naf_stem_conv_fwd reads), cached until the parameter changes."""
        cache = self.__dict__.setdefault("_wcache", {})
        w = conv.weight
        key = (w.data_ptr(), w._version, str(w.device))
        hit = cache.get(id(conv))
        if hit is None or hit[0] != key:
            k = w.shape[-1]
            hit = (key, ops.pack_conv_weight(w))
            cache[id(conv)] = hit
        return hit[1]

    def _stem_hip(self, image: torch.Tensor) -> torch.Tensor:
        """Both conv branches through naf_stem_conv0_fwd / naf_stem_conv_fwd; returns the concatenated
        guidance as a logical [B, 256, H, W] view of a channels-last bf16 buffer (naf.py:31-33)."""
        B, _, H, W = image.shape
        dev = image.device
        branches = (self.encoder, self.sem_encoder)
        hid = self.encoder[0].out_channels
        nstage = 1 + 2 * (len(self.encoder) - 1)
        stats = ops.new_stats(B, dev, lead=(2, nstage))      # one memset for all sums
        cat = torch.empty((B, H, W, 2 * hid), dtype=torch.bfloat16, device=dev)
        bufs = [torch.empty((B, H, W, hid), dtype=torch.bfloat16, device=dev) for _ in range(2)]
        for br, seq in enumerate(branches):
            conv0 = seq[0]
            w0, b0 = conv0.weight.detach().float().contiguous(), conv0.bias.detach().float()
            # 1x1 branch: the conv0 activation is never stored -- one statistics-only pass, then the first
            # GroupNorm/SiLU/conv layer recomputes it from the image (bit-identical, 0.5 GB less traffic)
            recompute = (self.fuse_conv0 and hid == 128 and conv0.kernel_size[0] == 1 and nstage > 1
                         and seq[1].conv1.kernel_size[0] == 1)
            last = nstage == 1
            dst = cat[..., br * hid:(br + 1) * hid] if last else bufs[0]
            ops.stem_conv0(image, w0, b0, None if recompute else dst, stats[br, 0])
            cur, st = dst, 0
            for blk in list(seq)[1:]:
                for norm, conv in ((blk.norm1, blk.conv1), (blk.norm2, blk.conv2)):
                    st += 1
                    last = st == nstage - 1
                    dst = cat[..., br * hid:(br + 1) * hid] if last else bufs[st % 2]
                    ops.stem_conv(None if (recompute and st == 1) else cur, stats[br, st - 1], norm.weight.detach().float(),
                                  norm.bias.detach().float(), norm.eps, self._packed(conv), conv.bias.detach().float(), dst,
                                  None if last else stats[br, st], first=(image, w0, b0) if (recompute and st == 1) else None)
                    cur = dst
        return cat.permute(0, 3, 1, 2)

    # ``guidance`` in three steps, so that a ``Guidance`` can keep what each one returns: the stem's input (the image, or its pre-shrunk
    # copy), the stem, the pooling to the output size.
    @staticmethod
    def stem_input_size(image_size, output_size) -> Tuple[int, int]:
        """The size the stem runs at for this output size: the image's own, or the pre-shrunk one of naf.py:39-48."""
        H, W = int(image_size[0]), int(image_size[1])
        ho, wo = output_size
        if H > 4 * ho or W > 4 * wo:
            return (min(H, 4 * ho, 4 * wo), min(W, 4 * wo, 4 * ho))
        return (H, W)

    def stem_input(self, image: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
        """``image`` at ``stem_input_size``: itself, or its bilinear pre-shrink."""
        x = image
        if tuple(x.shape[-2:]) != tuple(size):
            if x.is_cuda and x.dim() == 4 and x.shape[1] == 3 and x.dtype in (torch.float32, torch.bfloat16):
                x = ops.preshrink_image(x, size)                               # the kernel naf_forward uses as well
            else:
                x = F.interpolate(x.float(), size=size, mode="bilinear", align_corners=False)
        return x

    def guidance(self, image: torch.Tensor, output_size: Tuple[int, int]) -> torch.Tensor:
        """Pre-RoPE guidance features, logical [B, dim, Ho, Wo] (naf.py:37-49 + :31-35)."""
        x = self.stem_input(image, self.stem_input_size(image.shape[-2:], output_size))
        return self.pool(self.stem(x), output_size)

    def stem(self, x: torch.Tensor) -> torch.Tensor:
        """Both conv branches on the stem's input (naf.py:31-33): logical [B, dim, Hs, Ws]."""
        if self.use_encoder and self.stem_impl == "hip":
            if not self._hip_stem_ok():
                raise RuntimeError(f"naf_amd: the HIP conv stem serves hidden widths that are multiples of 16 up to 256 with "
                                   f"GroupNorm(8) (got {self.encoder[0].out_channels}); there is no silent torch fallback -- set "
                                   f"image_encoder.stem_impl = 'torch' explicitly to run MIOpen ops")
            x = self._stem_hip(x)
        elif self.use_encoder:
            dt = self.stem_dtype
            x = x.to(dt).contiguous(memory_format=torch.channels_last)
            x = torch.cat([self._branch(x, self.encoder, dt), self._branch(x, self.sem_encoder, dt)], dim=1)
        return x

    def pool(self, x: torch.Tensor, output_size: Tuple[int, int]) -> torch.Tensor:
        """The stem's output at the output size (naf.py:34), channels-last; the tensor itself when it is both already."""
        ho, wo = output_size
        if x.shape[-2:] != (ho, wo):                                           # naf.py:34
            if (x.dtype == torch.bfloat16 and x.is_cuda and x.shape[1] % 8 == 0
                    and x.is_contiguous(memory_format=torch.channels_last)):
                x = ops.pool_guidance(x, (ho, wo))                             # the kernel naf_forward uses as well
            else:
                x = F.adaptive_avg_pool2d(x, output_size=(ho, wo))
        return x.contiguous(memory_format=torch.channels_last)


class QueryEncoder(nn.Module):
    """Identity (naf.py:55-60)."""

    def forward(self, x):
        return x


class KeyEncoder(nn.Module):
    """``adaptive_avg_pool2d`` of the RoPE'd guidance to the feature grid (naf.py:63-69).  ``NAF.forward`` never calls it
    -- the pooling is fused into naf_rope_pool_fwd / naf_forward -- but callers that use the sub-module directly (as the
    reference allows) get the same result: HIP pooling kernel for channels-last bf16 device tensors, ATen otherwise."""

    def forward(self, x, features):
        size = tuple(int(v) for v in features.shape[-2:])
        if (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[1] % 8 == 0
                and x.is_contiguous(memory_format=torch.channels_last)):
            return ops.pool_guidance(x, size)
        return F.adaptive_avg_pool2d(x, output_size=size)


class CrossAttention(nn.Module):
    """Cross-scale neighbourhood attention (attentions.py:32-75) on naf_xna_fwd."""

    def __init__(self, dim, num_heads, kernel_size=(9, 9), **kwargs):
        super().__init__()
        assert dim % num_heads == 0, "dim must be divisible by num_heads"
        self.num_heads = num_heads
        self.kernel_size = tuple(kernel_size)
        self.scale = (dim // num_heads) ** -0.5
        self.dilation = None

    def forward(self, q5, k5, values, return_weights=False, path="auto", rope_tables=None):
        """q5/k5: 5-D bf16 views from ops.rope_pool; values: [B, C, h, w] features.  With ``rope_tables`` q5 is
        the un-rotated guidance and the attention kernel rotates it on load."""
        B, C = values.shape[:2]
        if C % self.num_heads:
            raise ValueError(f"feature channels {C} not divisible by {self.num_heads} heads")   # einops error in the reference
        Ho, Wo = q5.shape[2:4]
        h, w = values.shape[-2:]
        self.dilation = (Ho // h, Wo // w)                                     # attentions.py:56-57
        vp = ops.pack_values(values)
        v5 = vp.view(B, h, w, self.num_heads, C // self.num_heads).permute(0, 3, 1, 2, 4)
        # bf16 / float16 features leave in their own dtype (float16: half values on the f16 matrix instruction, nothing is rounded
        # to bf16 and no fp32 map exists); everything else is computed from bf16 values into fp32
        out_dtype = values.dtype if values.dtype in (torch.bfloat16, torch.float16) else torch.float32
        res = ops.xna_forward(q5, k5, v5, self.kernel_size, out_dtype=out_dtype, return_logits=return_weights,
                              path=path, scale=self.scale, rope_tables=rope_tables)
        out5, logits = res if return_weights else (res, None)
        # [B, heads, Ho, Wo, Dv] view of a channels-last buffer -> logical [B, C, Ho, Wo]
        out = out5.permute(0, 2, 3, 1, 4).reshape(B, Ho, Wo, C).permute(0, 3, 1, 2)
        if values.dtype not in (torch.bfloat16, torch.float16, torch.float32):
            out = out.to(values.dtype)      # float64
        return (out, logits) if return_weights else out


def _walk_parameters(module: nn.Module):
    """Every parameter below ``module``, read fresh from the module tree (a re-assigned parameter or a replaced sub-module is seen),
    without ``Module.parameters()``'s names and de-duplication: the plan-cache key of every forward call (100 -> 25 us of host time)."""
    for p in module._parameters.values():
        if p is not None:
            yield p
    for child in module._modules.values():
        if child is not None:
            yield from _walk_parameters(child)


class GraphedForward:
    """One NAF forward captured in a hipGraph (``torch.cuda.CUDAGraph``) and replayed: the ~13 kernel launches of a
    forward become one graph launch, which removes the host-side launch gaps (0.06 ms of a 2.5 ms G1 step, 10 % of
    a 448^2 step).  Shapes are frozen at capture; ``__call__`` copies new inputs into the captured buffers (or, with no
    arguments, replays on whatever ``.image`` / ``.features`` hold -- write into them in place to skip the copies).
    The returned tensor is the graph's own output buffer: it is overwritten by the next replay."""

    def __init__(self, model: "NAF", image: torch.Tensor, features: torch.Tensor, output_size, warmup: int = 2,
                 capture_error_mode: str = "global"):
        if isinstance(image, Guidance):
            raise TypeError("capture() takes the image, not a Guidance: the captured forward is the one-call plan, which encodes the image itself")
        if not (image.is_cuda and features.is_cuda):
            raise RuntimeError("GraphedForward needs device tensors")
        self.model, self.output_size = model, (int(output_size[0]), int(output_size[1]))
        self.image, self.features = image.clone(), features.clone()
        cur = torch.cuda.current_stream(image.device)
        side = torch.cuda.Stream(device=image.device)
        side.wait_stream(cur)
        # Always the fused inference forward, whatever mode the module is in: ``hubconf.naf()`` hands out a train-mode
        # module like the reference, and ``model(...)`` would then dispatch to ``forward_train`` (torch stem with saved
        # activations, a random RoPE jitter draw and an output with a grad_fn frozen into the graph).
        with torch.no_grad():
            with torch.cuda.stream(side):                   # warm-up outside the capture: caches, lazy module init
                for _ in range(max(1, warmup)):
                    model._forward_inference(self.image, self.features, self.output_size)
            cur.wait_stream(side)
            # the warm-up's workspace (1 GB at 1024^2) belonged to the throw-away stream: drop it before the capture allocates the
            # graph's own, instead of leaving it in the plan's pool until four other streams evict it
            side.synchronize()
            warm_plan = (model.__dict__.get("_plan_cache") or (None, None))[1]
            if warm_plan is not None:
                warm_plan.release_stream(image.device.index, int(side.cuda_stream))   # also drops the plan's "last used" reference to it
            # the capture runs on a stream of ours, and the second stream the forward forks onto (ops.forward_aux: the host lends
            # it to naf_forward_ex) is created BEFORE the capture begins
            cap = torch.cuda.Stream(device=image.device)
            ops.forward_aux(image.device, cap)
            self.graph = torch.cuda.CUDAGraph()
            # capture_error_mode="thread_local": other host threads may keep issuing (and synchronising with) eager work while this
            # one captures -- e.g. forwards of another module on another stream; their second streams are their own (ops.forward_aux)
            with torch.cuda.graph(self.graph, stream=cap, capture_error_mode=capture_error_mode):
                self.out = model._forward_inference(self.image, self.features, self.output_size)
        # The captured launches dereference device memory the graph does not own: the forward plan's workspace and
        # argument block, the RoPE tables, the packed bf16 weights.  They live in single-slot caches of the model that a
        # later eager call with other shapes (or a parameter update) replaces; hold them here so that a replay never
        # reads freed or recycled memory.
        enc = model.image_encoder
        plan_slot = model.__dict__.get("_plan_cache")
        plan = plan_slot[1] if plan_slot else None
        self._keep = [plan_slot, plan, getattr(plan, "_ws", None), getattr(plan, "_keep", None), enc.rope._tables,
                      dict(enc.__dict__.get("_wcache", {}))]

    def __call__(self, image: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None) -> torch.Tensor:
        if image is not None:
            self.image.copy_(image)
        if features is not None:
            self.features.copy_(features)
        self.graph.replay()
        return self.out


def _scores_mode(return_weights):
    """``ops.XnaFunction``'s seventh argument for a ``return_weights`` value: "differentiable", or whether the scores are returned at all."""
    if isinstance(return_weights, str):
        if return_weights != "differentiable":
            raise ValueError(f"return_weights must be a bool or 'differentiable', got {return_weights!r}")
        return "differentiable"
    return bool(return_weights)

_HEAD_FORMS = "an nn.Conv2d with a 1x1 kernel, an nn.Linear, or a (weight, bias_or_None) pair with weight [N, C] or [N, C, 1, 1]"


def _linear_head(head, channels: int):
    """(weight [N, C], bias [N] or None) of a linear head on ``channels`` features; TypeError for anything that is not one of the accepted
    forms, ValueError for an accepted form that is not a plain linear map of those channels.  Host-side checks only."""
    if isinstance(head, nn.Conv2d):
        pad = head.padding
        pad_ok = pad in ("valid", "same") if isinstance(pad, str) else all(int(v) == 0 for v in pad)
        if tuple(head.kernel_size) != (1, 1) or tuple(head.stride) != (1, 1) or head.groups != 1 or tuple(head.dilation) != (1, 1) or not pad_ok:
            raise ValueError(f"head: the convolution must be a plain 1x1 one (kernel 1, stride 1, no padding, dilation 1, groups 1), got {head}")
        weight, bias = head.weight[:, :, 0, 0], head.bias
    elif isinstance(head, nn.Linear):
        weight, bias = head.weight, head.bias
    elif isinstance(head, (tuple, list)) and len(head) == 2 and isinstance(head[0], torch.Tensor) and (head[1] is None or isinstance(head[1], torch.Tensor)):
        weight, bias = head
        if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
            weight = weight[:, :, 0, 0]
        if weight.dim() != 2:
            raise ValueError(f"head: weight must be [N, C] or [N, C, 1, 1], got {tuple(weight.shape)}")
    else:
        raise TypeError(f"head must be {_HEAD_FORMS}; got {type(head).__name__}")
    if weight.shape[1] != channels:
        raise ValueError(f"head: it reads {weight.shape[1]} channels, the features have {channels}")
    if weight.shape[0] < 1:
        raise ValueError("head: no output channels")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"head: bias must be [{weight.shape[0]}], got {tuple(bias.shape)}")
    if weight.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"head: weight must be float32 or bfloat16, got {weight.dtype}")
    return weight, bias


def _apply_head(head, x: torch.Tensor) -> torch.Tensor:
    """``head(x)`` for the accepted forms of ``head`` on [B, C, H, W] features (the unfused composition)."""
    if isinstance(head, nn.Conv2d):
        return head(x.to(head.weight.dtype))
    if isinstance(head, nn.Linear):
        return head(x.to(head.weight.dtype).permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
    weight, bias = head
    if weight.dim() == 2:
        weight = weight[:, :, None, None]
    return F.conv2d(x.to(weight.dtype), weight, None if bias is None else bias.to(weight.dtype))


def _cosine_head(head, channels: int) -> torch.Tensor:
    """The embedding matrix [N, C] of a ``cosine=True`` call: a tensor, a ``(weight, None)`` pair, or the weight of a bias-free ``nn.Linear`` /
    plain 1x1 ``nn.Conv2d``; any float dtype.  TypeError for other forms, ValueError for a bias or a shape that does not fit."""
    if isinstance(head, torch.Tensor):
        weight, bias = head, None
    elif isinstance(head, (nn.Conv2d, nn.Linear)):
        weight, bias = head.weight, head.bias
        if isinstance(head, nn.Conv2d):
            pad = head.padding
            pad_ok = pad in ("valid", "same") if isinstance(pad, str) else all(int(v) == 0 for v in pad)
            if tuple(head.kernel_size) != (1, 1) or tuple(head.stride) != (1, 1) or head.groups != 1 or tuple(head.dilation) != (1, 1) or not pad_ok:
                raise ValueError(f"head: the convolution must be a plain 1x1 one (kernel 1, stride 1, no padding, dilation 1, groups 1), got {head}")
    elif isinstance(head, (tuple, list)) and len(head) == 2 and isinstance(head[0], torch.Tensor) and (head[1] is None or isinstance(head[1], torch.Tensor)):
        weight, bias = head
    else:
        raise TypeError(f"cosine=True: head must be an [N, C] tensor, a (weight, None) pair, or a bias-free nn.Linear / 1x1 nn.Conv2d; got {type(head).__name__}")
    if bias is not None:
        raise ValueError("cosine=True: the head must have no bias (a cosine is taken against the rows of its weight)")
    if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight[:, :, 0, 0]
    if weight.dim() != 2 or not weight.is_floating_point():
        raise ValueError(f"cosine=True: the embeddings must be a floating-point [N, C] or [N, C, 1, 1] tensor, got {tuple(weight.shape)} {weight.dtype}")
    if weight.shape[1] != channels or weight.shape[0] < 1:
        raise ValueError(f"cosine=True: the embeddings are {tuple(weight.shape)}, the features have {channels} channels")
    return weight


Peaks = collections.namedtuple("Peaks", ["scores", "y", "x", "cell_scores", "cell_index"])
Peaks.__doc__ = """Result of ``NAF.locate``: ``scores`` [B, N, k] fp32, the k best cells' maxima of the scaled cosine in descending order (ties: the
lower flat index first); ``y``, ``x`` [B, N, k] int64, their pixels in output coordinates; ``cell_scores`` [B, N, h, w] fp32 and ``cell_index``
[B, N, h, w] int32, every low-res cell's maximum and its flat index ``y * Wo + x``."""

Match = collections.namedtuple("Match", ["scores", "y", "x", "distance"])
Match.__doc__ = """Result of ``NAF.match``: per source point its k best locations in the destination image, ``scores`` [P, k] fp32, ``y``, ``x`` [P, k]
int64; ``distance`` [P] fp32 with ``mutual=True`` (the pixel distance between the point and where its best match leads back to), else None."""


class KMeans(collections.namedtuple("KMeans", ["labels", "centroids", "counts", "shift"])):
    """Result of ``NAF.kmeans``: ``labels`` int64 [B, Ho, Wo], every pixel's cluster under the returned centroids; ``centroids`` fp32 [B, K, C]
    ([K, C] with ``per_image=False``); ``counts`` fp32 [B, K], the pixels per cluster (exact integers); ``shift`` fp32 [iters, B], the largest
    centroid movement ``max_k |c_new - c|`` of every iteration: the caller's convergence record."""
    __slots__ = ()

    def head(self, b: int = 0):
        """``(weight [K, C], bias [K])`` of image ``b``'s centroids as a linear head: ``naf(g, feats, size, head=r.head(), predict=True)``
        labels the pixels of other images by their nearest centroid (``argmax_k c_k . f - |c_k|^2 / 2``); on the clustered batch itself
        row ``b`` of that call is ``labels[b]``, bit for bit (``NAF.kmeans`` makes its final assignment this way)."""
        return _kmeans_head(self.centroids if self.centroids.dim() == 2 else self.centroids[b])


def _kmeans_head(c: torch.Tensor):
    """Centroids [K, C] as a linear head: ``argmax_k c_k . f - |c_k|^2 / 2`` is the nearest centroid."""
    return c, -0.5 * (c * c).sum(dim=1)


def _lib_last_error() -> str:
    return ops._lib.last_error()


def _rocm_only(**where) -> RuntimeError:
    """The error of a call with an operand off the ROCm device; ``where`` (name=tensor) is listed as "got <name> on <device>, ..."."""
    got = ", ".join(f"{n} on {t.device}" for n, t in where.items())
    return RuntimeError("naf_amd.NAF runs only on a ROCm device (HIP kernels, no CPU fallback)" + (f"; got {got}" if got else ""))


PointQuery = collections.namedtuple("PointQuery", ["features", "logits", "probs", "window_y", "window_x"])
PointQuery.__doc__ = """Result of ``NAF.query``: ``features`` [N, C] fp32 or None, ``logits`` / ``probs`` [N, heads, ky*kx] fp32 or None,
``window_y`` [N, ky] / ``window_x`` [N, kx] int32: the low-res rows / columns each point attends to (-1 for a point outside the grid)."""


class Guidance:
    """The image-side state of a ``NAF`` call, encoded once (``NAF.guide``) and accepted wherever ``NAF.forward`` takes an image on an
    inference call: nothing in the guidance depends on the feature map but the size of its grid, so other backbones, other grids, other
    dtypes and other output sizes for the same image skip the stem and -- where the keys are cached too -- the RoPE pass
    (notebooks/inference.ipynb cells 16 and 19 of the reference upsample five backbones / five sizes for one image).

    Four caches, filled on demand under ``torch.no_grad()``:
      stem output      per stem-input size (the image's, or a pre-shrunk one)   [B, dim, Hs, Ws] channels-last bf16
      pooled guidance  per (Ho, Wo)                                             un-rotated guidance at the output size
      rotated queries  per (Ho, Wo)                                             only once a call could not rotate on load
      keys             per (Ho, Wo, h, w)                                       pooled RoPE'd keys
    (and the RoPE tables per (Ho, Wo)).  ``nbytes``: bytes the caches hold; ``clear()`` drops them.

    It records (data_ptr, _version) of every parameter, of ``rope.periods`` and of the image: a call after an in-place change of any of them
    raises RuntimeError (stale).  Towards ``NAF``'s argument checks it answers like the image it stands for (``shape``, ``dim()``,
    ``is_cuda``, ``device``, ``dtype``, ``requires_grad``)."""

    def __init__(self, model: "NAF", image: torch.Tensor):
        if not isinstance(image, torch.Tensor) or image.dim() != 4:
            raise ValueError(f"guide: expected an image [B, 3, H, W], got "
                             + (f"{tuple(image.shape)}" if isinstance(image, torch.Tensor) else type(image).__name__))
        if not image.is_cuda:
            raise _rocm_only(image=image)
        self.model, self.image = model, image
        self._stamp = self._stamp_now()
        self._stem, self._pooled, self._queries, self._keys, self._tables = {}, {}, {}, {}, {}

    # ---- what NAF's argument checks read of an image ----
    shape = property(lambda self: self.image.shape)
    device = property(lambda self: self.image.device)
    dtype = property(lambda self: self.image.dtype)
    is_cuda = property(lambda self: self.image.is_cuda)
    requires_grad = property(lambda self: self.image.requires_grad)

    def dim(self) -> int:
        return self.image.dim()

    def _stamp_now(self):
        m, per = self.model, self.model.image_encoder.rope.periods
        return (tuple((p.data_ptr(), p._version) for p in _walk_parameters(m)), (per.data_ptr(), per._version),
                (self.image.data_ptr(), self.image._version))

    def check(self, model: "NAF") -> None:
        """RuntimeError unless this is ``model``'s guidance and neither its parameters nor the image changed since it was made."""
        if model is not self.model:
            raise RuntimeError("Guidance: made by another NAF module; call guide() on the module that uses it")
        prm, per, img = self._stamp_now()
        if img != self._stamp[2]:
            raise RuntimeError("Guidance is stale: the image was modified in place after guide(); call guide() again")
        if prm != self._stamp[0] or per != self._stamp[1]:
            raise RuntimeError("Guidance is stale: a parameter of the module (or rope.periods) changed after guide(); call guide() again")

    def _cached(self):
        for d in (self._stem, self._pooled, self._queries, self._keys):
            yield from d.values()
        for ty, tx in self._tables.values():
            yield ty
            yield tx

    @property
    def nbytes(self) -> int:
        """Bytes of device memory the caches hold (a stem output that is also a pooled level counts once)."""
        seen = {}
        for t in self._cached():
            st = t.untyped_storage()
            seen[st.data_ptr()] = st.nbytes()
        return sum(seen.values())

    def clear(self) -> None:
        for d in (self._stem, self._pooled, self._queries, self._keys, self._tables):
            d.clear()

    def tables(self, ho: int, wo: int):
        t = self._tables.get((ho, wo))
        if t is None:
            t = self._tables[(ho, wo)] = self.model.image_encoder.rope.tables(ho, wo)
        return t

    def pooled(self, ho: int, wo: int) -> torch.Tensor:
        """``image_encoder.guidance(image, (ho, wo))``, from the caches."""
        x = self._pooled.get((ho, wo))
        if x is None:
            enc = self.model.image_encoder
            with torch.no_grad(), ops._Timed("stem"):
                size = enc.stem_input_size(self.image.shape[-2:], (ho, wo))
                s = self._stem.get(size)
                if s is None:
                    s = self._stem[size] = enc.stem(enc.stem_input(self.image, size))
                x = self._pooled[(ho, wo)] = enc.pool(s, (ho, wo))
        return x

    def queries_keys(self, ho: int, wo: int, lr_size, heads_rope: int, q_layout: str, need_q: bool):
        """(rotated queries or None, keys) of ``ops.rope_pool`` for this output size and feature grid: cached ones where there are, else
        ONE launch -- queries and keys together when the queries are needed for the first time, keys only otherwise."""
        h, w = int(lr_size[0]), int(lr_size[1])
        q, k = self._queries.get((ho, wo)), self._keys.get((ho, wo, h, w))
        if k is None or (need_q and q is None):
            x = self.pooled(ho, wo)
            tab_y, tab_x = self.tables(ho, wo)
            with torch.no_grad():
                if need_q and q is None:
                    q, k = ops.rope_pool(x, tab_y, tab_x, heads_rope, (h, w), q_layout=q_layout)
                    self._queries[(ho, wo)] = q
                else:
                    _, k = ops.rope_pool(x, tab_y, tab_x, heads_rope, (h, w), write_q=False)
            self._keys[(ho, wo, h, w)] = k
        return (q if need_q else None), k


class NAF(nn.Module):
    """Drop-in for the reference's ``NAF`` (naf.py:72-116): same constructor, same ``state_dict``."""

    def __init__(self, dim=256, heads_attn=4, heads_rope=4, kernel_size=9, use_encoder=True, rope_base=100.0,
                 rope_rescale=2.0, img_layers=2, **kwargs):
        super().__init__()
        self.image_encoder = ImageEncoder(in_channels=3, out_channels=dim, heads_rope=heads_rope,
                                          use_encoder=use_encoder, rope_base=rope_base, img_layers=img_layers,
                                          rope_rescale=rope_rescale)
        self.query_encoder = QueryEncoder()
        self.key_encoder = KeyEncoder()
        self.upsampler = CrossAttention(dim=dim, num_heads=heads_attn, kernel_size=(kernel_size, kernel_size))
        self.xna_path = "auto"
        self.fuse_rope = True      # rotate queries inside the attention kernel when the shapes allow it
        self.single_call = True    # issue the whole forward through naf_forward (one foreign call) when possible

    def guidance_qk(self, image, lr_size, output_size, fuse_for=None, fusable=None):
        """bf16 queries and pooled RoPE'd keys (5-D views) for ``image``.  Returns (q5, k5, rope_tables):
        rope_tables is None when q5 is already rotated, or the (tab_y, tab_x) pair when q5 is the un-rotated
        guidance that the attention kernel rotates on load (``fuse_for`` = (Dv, out_dtype) of the attention call
        asks for that; it is granted when the shapes allow it, see ops.xna_rope_fusable).  ``fusable``: a predicate
        ``(q5, (tab_y, tab_x)) -> bool`` that decides it instead (the head-summed attention asks its own kernel, ``ops.xna_head_select``).
        ``image`` may be a ``Guidance``: the guidance, the tables, rotated queries and keys then come from its caches (``Guidance.queries_keys``:
        at most one ``ops.rope_pool`` launch, none when this size and grid were seen); the choice between the two query forms is the same."""
        ho, wo = int(output_size[0]), int(output_size[1])
        enc = self.image_encoder
        g = image if isinstance(image, Guidance) else None
        if g is not None:
            x = g.pooled(ho, wo)
            tab_y, tab_x = g.tables(ho, wo)
        else:
            with ops._Timed("stem"):
                x = enc.guidance(image, (ho, wo))
            tab_y, tab_x = enc.rope.tables(ho, wo)
        heads_rope, heads_attn = enc.rope.num_heads, self.upsampler.num_heads
        same = heads_attn == heads_rope
        if (fuse_for is not None or fusable is not None) and self.fuse_rope and same and x.dtype == torch.bfloat16:
            B, Cq = x.shape[:2]
            xq = x.permute(0, 2, 3, 1)                                            # [B, Ho, Wo, C] view
            if xq.stride(3) == 1:
                q5 = xq.unflatten(3, (heads_rope, Cq // heads_rope)).permute(0, 3, 1, 2, 4)
                if fusable is not None:
                    ok = fusable(q5, (tab_y, tab_x))
                else:
                    ok = ops.xna_rope_fusable(q5, lr_size, fuse_for[0], self.upsampler.kernel_size, (tab_y, tab_x),
                                              out_dtype=fuse_for[1], path=self.xna_path)
                if ok:
                    if g is not None:
                        _, k5 = g.queries_keys(ho, wo, lr_size, heads_rope, "head_major", need_q=False)
                    else:
                        _, k5 = ops.rope_pool(x, tab_y, tab_x, heads_rope, lr_size, write_q=False)
                    return q5, k5, (tab_y, tab_x)
        q_layout = "head_major" if same else "channels_last"
        if g is not None:
            q5, k5 = g.queries_keys(ho, wo, lr_size, heads_rope, q_layout, need_q=True)
        else:
            q5, k5 = ops.rope_pool(x, tab_y, tab_x, heads_rope, lr_size, q_layout=q_layout)
        if not same:        # re-split the channel axis for attention: pure views of channels-last buffers
            B, _, Ho, Wo, _ = q5.shape
            dim = enc.out_channels
            q5 = q5.permute(0, 2, 3, 1, 4).reshape(B, Ho, Wo, heads_attn, dim // heads_attn).permute(0, 3, 1, 2, 4)
            h, w = k5.shape[2:4]
            k5 = k5.permute(0, 2, 3, 1, 4).reshape(B, h, w, heads_attn, dim // heads_attn).permute(0, 3, 1, 2, 4)
        return q5, k5, None

    def _forward_plan(self, image, features, output_size):
        """``ops.ForwardPlan`` (one ``naf_forward`` call per forward) when the configuration allows it, else None:
        default width through the fused stem (any image / output / feature sizes, either head split, return_weights).
        Cached until a parameter, the shapes, strides or dtypes change."""
        enc = self.image_encoder
        ho, wo = int(output_size[0]), int(output_size[1])
        if not (enc.use_encoder and enc.stem_impl == "hip" and enc._hip_stem_default_width() and enc.fuse_conv0 and self.fuse_rope):
            return None
        if image.shape[1] != 3 or self.xna_path != "auto":
            return None
        if features.dtype not in (torch.bfloat16, torch.float16, torch.float32):
            return None
        if image.dtype not in (torch.bfloat16, torch.float32) or features.shape[1] % self.upsampler.num_heads:
            return None
        if self.upsampler.kernel_size[0] != self.upsampler.kernel_size[1]:
            return None
        prm_key = tuple((p.data_ptr(), p._version) for p in _walk_parameters(self)) + (enc.rope.periods.data_ptr(), enc.rope.periods._version)
        key = (prm_key, tuple(image.shape), tuple(image.stride()), image.dtype, tuple(features.shape), tuple(features.stride()),
               features.dtype, str(image.device), (ho, wo))
        hit = self.__dict__.get("_plan_cache")
        if hit is not None and hit[0] == key:
            return hit[1]
        branches = []
        for seq in (enc.encoder, enc.sem_encoder):
            c0 = seq[0]
            layers = [(n.weight.detach().float().contiguous(), n.bias.detach().float().contiguous(), enc._packed(c),
                       c.bias.detach().float().contiguous())
                      for blk in list(seq)[1:] for n, c in ((blk.norm1, blk.conv1), (blk.norm2, blk.conv2))]
            if len(layers) > 8 or any(c.kernel_size[0] != seq[1].conv1.kernel_size[0] for blk in list(seq)[1:] for c in (blk.conv1, blk.conv2)):
                return None
            branches.append((c0.weight.detach().float().contiguous(), c0.bias.detach().float().contiguous(), c0.kernel_size[0],
                             seq[1].conv1.kernel_size[0] if len(seq) > 1 else 1, layers))
        if not branches[0][4]:
            return None
        eps = enc.encoder[1].norm1.eps
        plan = ops.ForwardPlan(branches, len(branches[0][4]), eps, enc.rope.tables(ho, wo), image, features,
                               self.upsampler.num_heads, self.upsampler.kernel_size[0],
                               features.dtype if features.dtype in (torch.bfloat16, torch.float16) else torch.float32, self.upsampler.scale,
                               output_size=(ho, wo), heads_rope=enc.rope.num_heads)
        plan = plan if plan.supported else None
        self.__dict__["_plan_cache"] = (key, plan)
        return plan

    def capture(self, image, features, output_size, capture_error_mode: str = "global") -> GraphedForward:
        """Capture this forward for the given shapes in a hipGraph; see ``GraphedForward``."""
        return GraphedForward(self, image, features, output_size, capture_error_mode=capture_error_mode)

    def forward_train(self, image, features, output_size, amp="auto", return_weights=False, regress=None, regress_path="auto"):
        """Differentiable forward for training (train.py:127-137): gradients reach the encoder parameters, the image
        and the features.  The attention and its backward are the HIP kernels (naf_xna_fwd / naf_xna_bwd through
        ``ops.XnaFunction``); the conv stem runs as ``_HipStem`` (HIP forward and backward kernels) or, as the A/B arm, as torch ops
        (``amp`` below); RoPE and key pooling run as HIP kernels with their own backward (``ops.RopePoolFunction``) where the stem is
        ``_HipStem`` and the RoPE heads are the attention heads with a head dim that is a multiple of 32, as torch ops otherwise.  On that
        branch the pooling of a guidance image larger than the output (naf.py:34; the reference trains at 4x, train.py:126-127) is
        ``ops.pool_guidance`` with its backward ``naf_pool_guidance_bwd`` (bf16 channels-last in both directions, no fp32 copy of the
        full-resolution guidance), and with ``_HipStem`` the pre-shrink of an image more than 4x the output (naf.py:39-48) is
        ``ops.preshrink_image`` with ``naf_preshrink_image_bwd`` (a gather, bit-reproducible); the torch arms keep ATen's ops.  In ``.train()`` mode the RoPE coordinates get the
        reference's random rescale (rope.py:107-124, NAF's rope_rescale); in ``.eval()`` mode they are deterministic.  Every geometry
        has a backward kernel (``ops.xna_backward_select``): the MFMA cell kernel (integer ratio, Wo/w a multiple of 16, window <= 13
        with K/V windows inside the LDS), the row-streaming matrix-core kernel (every other integer ratio: the reference's own training
        geometry 16^2 -> 32^2, patch-14 backbones, the denoising call), the table-driven scalar kernel for the rest.
        ``return_weights``: also returns the scaled pre-softmax scores [B, heads, Ho, Wo, k*k] of the q / k this step used, fp32.  True:
        without a gradient (its callers only display them).  "differentiable": with a gradient that reaches q and k -- and through them the
        stem, RoPE and the image -- as the reference's scores have one (legacy_attention, attentions.py:16-29): a loss on them (attention-map
        regularisers, attention distillation) trains the encoder.  The backward then runs naf_xna_bwd_scores (C ABI 0.4.3).
        ``amp="auto"`` (the default, and what ``model(image, feats, size)`` uses when a gradient is wanted; round 6) trains through the
        library's own differentiable stem ``_HipStem`` whenever ``image_encoder.stem_impl == "hip"`` and the width has HIP training
        kernels -- with or without ``torch.autocast``: its contract (bf16 activations between layers, fp32 accumulation, fp64 GroupNorm
        sums) is what the inference forward computes, so training and inference see the same function.  The torch stem stays as the
        explicit A/B arm: ``amp=False`` = fp32 MIOpen convolutions, ``amp=True`` = the reference's ``use_bf16`` mode (bf16 stem
        convolutions under ``torch.autocast``, train.py:120, denoising.py:209; GroupNorm statistics, RoPE and pooling fp32);
        ``stem_impl = "torch"`` makes "auto" choose between those two by the ambient autocast state.  ``amp="hip"`` insists on
        ``_HipStem`` (raises when the width is not served).
        ``regress`` / ``regress_path``: the objective of ``forward(..., regress=...)`` -- the call returns the 0-dim fp32 mean squared error
        against ``regress`` instead of the feature map.  On the HIP branch (``_HipStem`` + ``ops.RopePoolFunction``), where
        ``ops.xna_mse_auto`` says so (or ``regress_path="fused"`` insists), ``ops.XnaMSEFunction`` stands in place of ``ops.XnaFunction``:
        the attention kernel's epilogue computes the loss and leaves its gradient for naf_xna_bwd, and nothing of the step between the
        attention forward and backward is a torch op.  Otherwise: ``F.mse_loss`` on the map this method computes."""
        if regress is not None and return_weights:
            raise ValueError("forward_train(regress=...) returns the loss alone: the scores belong to the features' call")
        if regress_path not in ("auto", "fused", "composed"):
            raise ValueError(f"regress_path must be 'auto', 'fused' or 'composed', got {regress_path!r}")
        if not (image.is_cuda and features.is_cuda):
            raise _rocm_only()
        enc = self.image_encoder
        ho, wo = int(output_size[0]), int(output_size[1])
        h, w = features.shape[-2:]
        heads_rope, heads = enc.rope.num_heads, self.upsampler.num_heads
        x = image
        if amp == "auto":
            if enc.use_encoder and enc.stem_impl == "hip" and enc._hip_train_stem_ok():
                amp = "hip"
            else:
                amp = bool(torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16)
        if x.shape[-2] > 4 * ho or x.shape[-1] > 4 * wo:                       # naf.py:39-48
            size = (min(x.shape[-2], 4 * ho, 4 * wo), min(x.shape[-1], 4 * wo, 4 * ho))
            if enc.use_encoder and amp == "hip" and x.dim() == 4 and x.shape[1] == 3:
                # naf_preshrink_image, and naf_preshrink_image_bwd when the image wants a gradient (a gather: no atomic scatter)
                x = ops.preshrink_image(x if x.dtype in (torch.float32, torch.bfloat16) else x.float(), size)
            else:
                x = F.interpolate(x.float(), size=size, mode="bilinear", align_corners=False)

        def rope_tabs():    # [Ho, 2, P], [Wo, 2, P]; in training mode with the reference's coordinate augmentation (rope.py:107-124)
            if enc.rope.training and enc.rope.cache_train_coords:
                if (ho, wo) not in enc.rope._train_tables:
                    enc.rope._train_tables[(ho, wo)] = _rope_train_tables(enc.rope, ho, wo)
                return enc.rope._train_tables[(ho, wo)]
            return _rope_train_tables(enc.rope, ho, wo) if enc.rope.training else enc.rope.tables(ho, wo)

        tabs = None
        if enc.use_encoder and amp == "hip":
            if not enc._hip_train_stem_ok():
                raise RuntimeError("forward_train(amp='hip'): the differentiable HIP stem serves hidden widths that are multiples of 16 "
                                   f"up to 256 with GroupNorm(8) (got {enc.encoder[0].out_channels})")
            rope_hip = heads_rope == heads and (2 * enc.encoder[0].out_channels // heads_rope) % 32 == 0
            if rope_hip:
                # before the stem: its last layer, the pooling and naf_rope_pool_fwd then follow one another on the stream
                tabs = tuple(t.contiguous() for t in rope_tabs())
            x = _HipStem.apply(enc, x, *_hip_stem_params(enc))
            if x.shape[-2:] != (ho, wo):
                if rope_hip:
                    # naf.py:34 as naf_pool_guidance / naf_pool_guidance_bwd: bf16 channels-last from the stem's last layer into
                    # RopePoolFunction below, and the gradient the same way back (no fp32 copy of the full-resolution guidance)
                    x = ops.pool_guidance(x, (ho, wo))
                else:
                    x = x.float()
        elif enc.use_encoder:
            x = x.float().contiguous(memory_format=torch.channels_last)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(amp)):
                x = torch.cat([enc._branch_train(x, enc.encoder), enc._branch_train(x, enc.sem_encoder)], dim=1)
            x = x.float()
        if x.shape[-2:] != (ho, wo):
            x = F.adaptive_avg_pool2d(x, output_size=(ho, wo))                 # naf.py:34

        if amp == "hip" and heads_rope == heads and (x.shape[1] // heads_rope) % 32 == 0:
            # RoPE, key pooling and their backward as HIP kernels too (naf_rope_pool_fwd / naf_rope_pool_bwd): the guidance stays
            # bf16 channels-last from the stem's last layer to the attention kernel, and so does its gradient on the way back
            tab_y, tab_x = tabs if tabs is not None else rope_tabs()
            xcl = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            q5, k5 = ops.RopePoolFunction.apply(xcl, tab_y.contiguous(), tab_x.contiguous(), heads_rope, (h, w))
            B, C = features.shape[:2]
            v5 = features.reshape(B, heads, C // heads, h, w).permute(0, 1, 3, 4, 2).to(torch.bfloat16).contiguous()
            out_dtype = torch.bfloat16 if features.dtype == torch.bfloat16 else torch.float32
            if regress is not None and regress_path != "composed" and C % heads == 0:
                ksz = self.upsampler.kernel_size
                if regress_path == "fused":
                    fused = ops.xna_mse_supported(q5, k5, v5, regress, ksz)
                    if not fused:
                        raise ops._lib.NafHipError(f"naf(..., regress_path='fused'): {ops._lib.last_error()}")
                else:
                    fused = ops.xna_mse_auto(B, heads, q5.shape[-1], C // heads, (h, w), (ho, wo), ksz, out_dtype, regress) \
                        and ops.xna_mse_supported(q5, k5, v5, regress, ksz)
                if fused:
                    with ops._Timed("attention"):
                        return ops.XnaMSEFunction.apply(q5, k5, v5, regress, ksz, self.upsampler.scale)
            res = ops.XnaFunction.apply(q5, k5, v5, self.upsampler.kernel_size, self.upsampler.scale, out_dtype, _scores_mode(return_weights))
            out5, logits = res if return_weights else (res, None)
            # [B, heads, Ho, Wo, Dv] is a view of a [B, Ho, Wo, heads * Dv] buffer: hand it out as a logical NCHW view of that
            # (channels-last memory, no transpose copy of the largest tensor of the step)
            out = out5.permute(0, 2, 3, 1, 4).reshape(B, ho, wo, C).permute(0, 3, 1, 2)
            if regress is not None:
                return F.mse_loss(out.float(), regress.float())
            return (out, logits) if return_weights else out
        if regress is not None and regress_path == "fused":
            raise ops._lib.NafHipError("naf(..., regress_path='fused'): the fused objective follows the HIP stem and ops.RopePoolFunction; this "
                                       "configuration trains through torch ops there (regress_path='auto' composes the loss)")
        # RoPE (rope.py:15-34,139-153) from the cached tables: angle index t < D/4 -> row, else column
        tab_y, tab_x = rope_tabs()
        B, Cq = x.shape[:2]
        D = Cq // heads_rope
        cos = torch.cat([tab_y[:, 0, None, :].expand(ho, wo, -1), tab_x[None, :, 0, :].expand(ho, wo, -1)], dim=-1)
        sin = torch.cat([tab_y[:, 1, None, :].expand(ho, wo, -1), tab_x[None, :, 1, :].expand(ho, wo, -1)], dim=-1)
        xh = x.reshape(B, heads_rope, D, ho, wo).permute(0, 1, 3, 4, 2)        # [B, n, Ho, Wo, D]
        x1, x2 = xh[..., : D // 2], xh[..., D // 2:]
        xr = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
        xr = xr.permute(0, 1, 4, 2, 3).reshape(B, Cq, ho, wo)
        if ho % h == 0 and wo % w == 0:                                        # naf.py:63-69 (pooled AFTER RoPE); box mean as a
            k = xr.reshape(B, Cq, h, ho // h, w, wo // w).mean(dim=(3, 5))    # reshape: its backward is a broadcast, not atomics
        else:
            k = F.adaptive_avg_pool2d(xr, output_size=(h, w))
        Dq, C = Cq // heads, features.shape[1]
        to5 = lambda t, d: t.reshape(B, heads, d, *t.shape[-2:]).permute(0, 1, 3, 4, 2).to(torch.bfloat16).contiguous()
        q5, k5, v5 = to5(xr, Dq), to5(k, Dq), to5(features, C // heads)
        out_dtype = torch.bfloat16 if features.dtype == torch.bfloat16 else torch.float32
        res = ops.XnaFunction.apply(q5, k5, v5, self.upsampler.kernel_size, self.upsampler.scale, out_dtype, _scores_mode(return_weights))
        out5, logits = res if return_weights else (res, None)
        out = out5.permute(0, 1, 4, 2, 3).reshape(B, C, ho, wo)
        if regress is not None:
            return F.mse_loss(out.float(), regress.float())
        return (out, logits) if return_weights else out

    def forward(self, image, features, output_size, return_weights=False, *args, head=None, target=None, ignore_index=-100,
                reduction="mean", predict=False, confusion=None, regress=None, regress_path="auto", cosine=False, logit_scale=1.0,
                return_norms=False, cosine_path="auto", loss=None, masks=None, mask_reduce="mean", mask_path="auto",
                return_attention=False, dense_target=None, dense_loss="l1", beta=1.0, valid=None, errors=None, clamp=None, **kwargs):
        """``naf(image, lr_features, target_size)`` (naf.py:104-116).  ``return_weights``: False, True (``(out, scores)``, the scores
        without a gradient) or "differentiable" (``(out, scores)`` with scores that carry a gradient to q and k on a gradient-enabled call,
        as the reference's always do; see ``forward_train``).  Outside a gradient-enabled call "differentiable" is the same as True.  The reference's forward is always differentiable;
        here the fused inference kernels run unless a gradient is actually wanted: autograd enabled AND (an input requires
        grad, or the module is in ``.train()`` mode with trainable parameters) -- then the call is ``forward_train``
        (train.py:127-137, denoising.py:213 work unchanged).  README usage (``naf.eval()`` then ``naf(...)``) and any call
        under ``torch.no_grad()`` take the inference path; that path always uses the deterministic eval-mode RoPE
        coordinates (the reference's train-mode coordinate jitter only exists on the differentiable path here).

        ``image`` may be a ``Guidance`` (``self.guide(image)``) on every inference call described here -- the plain call with bf16 / fp16 /
        fp32 features, ``return_weights=True``, ``head=`` with or without ``target`` / ``predict``, ``confusion=``: the stem, the pooling
        and, for a size and grid seen before, the RoPE pass are not run again, and the result is what the image call computes through the
        same operators (``single_call = False``).  Gradients with respect to the head keep working.  Refused: ``regress=`` and
        ``return_weights="differentiable"`` (ValueError: both train the encoder), a call that would take the training path (RuntimeError),
        a stale ``Guidance`` (RuntimeError).  ``self.query(guidance, points, ...)`` is the attention at N pixels.

        ``head`` (keyword only): a linear probe on the upsampled features -- an ``nn.Conv2d`` with a 1x1 kernel, an ``nn.Linear`` or a
        ``(weight, bias_or_None)`` pair (weight [N, C] or [N, C, 1, 1]) -- what evaluation/eval_seg_probing.py:56,104-111 puts on
        ``model(image, feats, (H, W))``.  The call then returns the logits ``head(naf(image, features, size))`` as a logical
        [B, N, Ho, Wo] tensor in the head weight's dtype (float32 / bfloat16) whose memory is a dense channels-last [B, Ho, Wo, N] buffer
        (strides (Ho*Wo*N, 1, Wo*N, N)), WITHOUT forming the [B, C, Ho, Wo] features: the attention is linear in the values and its
        weights sum to one, so the head is applied on the low-res grid (``ops.project_head_values``) and the head-summed attention
        kernel (``ops.xna_head_forward``) writes N channels per pixel.  With a frozen upsampler (``torch.no_grad()``, or no trainable
        upsampler parameter in ``.train()`` mode and no input that requires grad) the call is differentiable WITH RESPECT TO THE HEAD when
        its parameters require grad (probe training): the stem, RoPE and key pooling run on the inference kernels without a graph, only
        the projection and ``ops.XnaHeadFunction`` are recorded.  A call that wants a gradient for the upsampler, the image or the
        features runs the unfused composition ``head(self.forward_train(...))`` -- correct, not fused.  ``return_weights`` together with
        ``head`` is rejected (ValueError): the scores belong to the features' call.  Anything that is not one of the three forms raises
        TypeError; a 3x3 / strided / grouped / dilated convolution or a channel mismatch raises ValueError (no silent fallback).
        ``head=None`` is the call above, untouched.

        ``target``, ``ignore_index``, ``reduction``, ``predict`` (keyword only, with ``head``): the probe's objective instead of its logits --
        what the reference's probing loop does with them (evaluation/eval_seg_probing.py:94-135).  ``target`` (integer class indices
        [B, Ho, Wo] on the features' device; other integer dtypes are converted to int64, resizing a mismatching target stays the caller's
        business) returns ``F.cross_entropy(head(naf(...)).float(), target, ignore_index=ignore_index, reduction=reduction)``: a 0-dim fp32
        tensor, or [B, Ho, Wo] fp32 for ``reduction="none"``; ``predict=True`` returns ``head(naf(...)).argmax(1)`` as int64 [B, Ho, Wo];
        both return ``(loss, labels)`` from one launch.  The logits tensor is not written: the head-summed kernel's epilogue
        (``ops.xna_head_objective``) takes the softmax over the classes in registers.  ``ignore_index`` defaults to torch's -100 (the
        reference passes 255).  One difference from torch: a target outside [0, N) that is not ``ignore_index`` is IGNORED (no loss, no
        gradient, not counted) where ``F.cross_entropy`` raises a device-side assert.  ``reduction="mean"`` without a valid pixel is nan,
        as in torch.  The gradient modes are those of the logits call: frozen upsampler and a probe that requires grad -- fused and
        differentiable with respect to the probe (``ops.XnaHeadCEFunction``); no gradient wanted -- the kernel with rotate-on-load; a
        gradient for the upsampler, the image or the features -- the unfused ``F.cross_entropy(head(self.forward_train(...)).float(), ...)``.

        ``confusion`` (keyword only, with ``head`` and ``target``): the probe's EVALUATION -- what the reference's ``evaluate()``
        (evaluation/eval_seg_probing.py:221-257) accumulates for its accuracy and Jaccard index.  ``confusion=True`` returns a fresh int64
        [N, N] matrix of this call, ``cm[t, p]`` = number of pixels with target ``t`` and predicted label ``p`` (row = target, column =
        prediction) over the pixels that are not ignored (``target != ignore_index`` and ``0 <= target < N``); an int64 [N, N] tensor on
        the features' device (columns contiguous) is ACCUMULATED into in place and returned, so an evaluation loop passes the same
        tensor for every batch and never synchronises with the host; ``naf_amd.confusion_metrics(cm)`` turns it into accuracy and IoU,
        ``naf_amd.dist.reduce_confusion(cm)`` sums it over ranks.  The call returns the matrix IN PLACE OF the loss -- no cross-entropy is
        computed (``reduction`` is not used) -- or ``(matrix, labels)`` with ``predict=True``.  The head-summed kernel's epilogue counts
        (``naf_xna_head_cm_fwd``: aggregated per wave, integer atomics, bit-reproducible); no label map is written unless asked for.  It
        is never differentiable and runs the inference kernels (rotate-on-load where the geometry allows) whatever the gradient mode.
        Geometries or class counts the kernel does not serve count the labels of the composed path, same contract.  An empty batch leaves
        the matrix as it was.  Loss and matrix from ONE launch stay available one level down: ``ops.xna_head_objective(..., want_loss=True,
        confusion=cm)``.
        Not offered: class weights, label smoothing, soft targets, ``capture()`` of this call.

        ``regress``, ``regress_path`` (keyword only): the objective of the reference's own training step (train.py:127-132,
        ``loss = mse(model(img, lr_feats, size).float(), hr_feats.float())``) instead of the feature map.  ``regress`` is a float32 /
        bfloat16 tensor [B, C, Ho, Wo] on the features' device (any strides: a ViT wrapper's ``b (h w) c -> b c h w`` view is read
        with vector loads), without a gradient of its own; the call returns the 0-dim fp32 value
        ``F.mse_loss(naf(image, features, size).float(), regress.float())``.  ``regress_path="auto"`` takes that value from the attention
        kernel's epilogue (``ops.xna_mse_forward``: the kernel subtracts the target from its fp32 accumulators, writes the loss's gradient
        in bf16 where it would write the features, and sums the squared error -- the prediction, its fp32 copy and the fp32 gradient never
        exist) wherever the plain forward of these shapes runs the table-driven MFMA kernel (``naf_xna_select`` says NAF_XNA_UNION: the
        reference's training geometry 16^2 -> 32^2, non-integer ratios, ratio 1, small integer ratios; head dim 64, C / heads a multiple
        of 16) and the stem is the HIP stem; everywhere else it is the composed expression above.  ``"fused"`` insists (NafHipError where
        ``naf_xna_mse_supported`` refuses, or where the torch stem arms run); ``"composed"`` is the A/B arm.  On a gradient-enabled call
        (as defined above) this is ``forward_train`` with ``ops.XnaMSEFunction`` in place of ``ops.XnaFunction``: ``loss.backward()`` trains
        the encoder as today's step does, from a ``dout`` that carries one bf16 rounding instead of two.  Without a gradient the inference stem
        and materialised queries feed the loss-only launch (nothing but the loss is written).  ``regress`` together with ``head``,
        ``target``, ``predict``, ``confusion`` or ``return_weights`` raises ValueError; shape, dtype and device mismatches raise before any
        device work.  Not offered: other losses, the reference's unused ``normalize=True``, ``capture()`` of this call.

        ``cosine``, ``logit_scale``, ``return_norms``, ``cosine_path`` (keyword only, with ``head``): open-vocabulary logits and
        similarity heat maps.  ``head`` is then an embedding matrix ``E`` [N, C] of any float dtype -- a tensor, a ``(weight, None)`` pair,
        or an ``nn.Linear`` / 1x1 ``nn.Conv2d`` WITHOUT bias whose weight it is -- and the call returns, in fp32 [B, N, Ho, Wo],
            ``logit_scale * einsum("nc,bchw->bnhw", F.normalize(E.float(), dim=1), F.normalize(naf(image, features, size).float(), dim=1))``
        (eps 1e-12 in both: a pixel whose upsampled feature is zero gets exactly 0, never NaN); with ``return_norms=True``
        ``(cos, norms)``, ``norms`` [B, Ho, Wo] fp32 = the feature's unclamped 2-norm.  ``cosine_path="auto"`` takes it from the attention
        kernel (``ops.xna_cos_forward``: the [B, C, Ho, Wo] features, their fp32 copy and the normalised copy never exist) for bf16 features
        on the geometries ``head=`` is fused for (windows 13 and 15 up to 64 embeddings), and is the expression above in torch ops on the
        plain forward everywhere else: fp16 / fp32 features, non-integer ratios, ratio 1, and whenever a gradient is enabled and ``E``
        requires one (that route is differentiable with respect to ``E``; the fused one is inference-only without ``loss=``).  ``"fused"`` insists
        (NafHipError with the library's reason); ``"composed"`` is the A/B arm.  ``cosine=True`` with ``predict=True`` or with ``target=`` and
        ``confusion=`` runs those calls with ``head=(F.normalize(E.float(), dim=1), None)``: the argmax does not see the per-pixel positive
        scale.  ValueError: a head with a bias, ``target=`` without ``confusion=`` or ``loss=`` (the loss is ``loss="ce"``, below), ``regress=``, ``return_weights``,
        ``return_norms`` with ``predict`` / ``confusion``.  Not offered: ``capture()`` of this call.

        ``loss="ce"`` (keyword only, with ``cosine=True`` and ``target``): TRAINING against the cosines -- a cosine classifier as a dense
        probe, prompt / embedding tuning, a learnable temperature.  The call returns
            ``F.cross_entropy(cos.float(), target, ignore_index=ignore_index, reduction=reduction)``
        on the scaled cosines ``cos`` defined above (a 0-dim fp32 tensor, [B, Ho, Wo] for ``reduction="none"``; targets outside [0, N) are
        ignored as for ``head=probe``), or ``(loss, pred)`` with ``predict=True`` (``pred`` int64 [B, Ho, Wo], from the same launch).
        ``logit_scale`` is a float or a 1-element fp32 tensor; a tensor is read on the device (no host synchronisation) and receives a
        gradient when it requires one, as do the embeddings.  ``cosine_path="auto"`` takes loss, labels and both gradients from the
        attention kernel's epilogue (``ops.XnaCosCEFunction`` / ``ops.xna_cos_objective``: one forward launch, and for the embeddings one
        launch of the attention backward; the [B, C, Ho, Wo] features, their copies and the [B, N, Ho, Wo] cosines never exist) where
        ``naf_xna_cos_ce_select`` grants the geometry, the features are bf16 and no gradient is wanted for the upsampler or its inputs;
        everything else is the expression above in torch ops on the plain forward (``forward_train`` when the upsampler wants a
        gradient).  ``"fused"`` insists (NafHipError with the reason); ``"composed"`` is the A/B arm.  ``image`` may be a ``Guidance``.
        ValueError, before any device work: ``loss`` other than None / "ce"; ``loss`` without ``cosine=True``, without ``target``, with
        ``return_norms`` or with ``confusion``; a float ``logit_scale <= 0`` with ``predict``.  Not offered: a gradient for the upsampler
        through the fused route, class weights, label smoothing, soft targets, fp16 / fp32 features on the fused route.

        ``masks``, ``mask_reduce``, ``mask_path``, ``return_attention`` (keyword only): MASKED AVERAGE POOLING -- region embeddings for mask
        proposals, prototypes for few-shot and reference-guided segmentation ("scribble a mask, see what looks like it":
        ``E = naf(image, feats, size, masks=M)``, then ``naf(image, feats, size, head=E[b], cosine=True)``).  ``masks`` is [B, K, Ho, Wo], dtype
        bool, uint8, bfloat16, float16 or float32, on the features' device, without a gradient; the call returns fp32 [B, K, C]:
            ``einsum("bkhw,bchw->bkc", masks.float(), naf(image, features, size).float())``
        divided by ``mass[b, k] = masks[b, k].sum()`` for ``mask_reduce="mean"``, undivided for ``"sum"``.  A mask of zero mass gives a row of
        exact zeros, never NaN (the convention of the cosine head for a zero feature).  ``return_attention=True`` returns ``(pooled, A,
        mass)`` with ``A`` fp32 [B, heads, K, h, w], the attention summed under each mask on the low-res grid, and ``mass`` fp32 [B, K].
        ``mask_path="auto"`` takes ``A`` and ``mass`` from the mask-pooling kernel (``ops.xna_mask_pool``: it never reads the features, and the
        [B, C, Ho, Wo] tensor and its fp32 copy never exist) and contracts them with the features on the low-res grid
        (``ops.mask_pool_apply``) where ``naf_xna_maskpool_select`` grants the geometry (those of ``head=``) and the features are bf16;
        everything else is the expression above in torch ops on the plain forward: non-integer ratios, ratio 1, fp16 / fp32 features, or a
        call that wants a gradient for the upsampler or the features (``forward_train``).  ``"fused"`` insists (NafHipError with the
        library's reason); ``"composed"`` is the A/B arm.  float16 / float32 masks are rounded once to bfloat16 on the fused route; more than
        64 masks run in chunks of 64.  ``image`` may be a ``Guidance``.  ValueError, before any device work: ``masks`` together with ``head``,
        ``target``, ``predict``, ``confusion``, ``regress``, ``return_weights`` or ``cosine``; a wrong shape or device; ``mask_reduce`` outside
        the two values.  Not offered: integer label maps (pass ``labels[:, None] == torch.arange(K, device=labels.device)[None, :, None, None]``),
        a gradient through the fused route, ``capture()`` of this call.

        ``dense_target``, ``dense_loss``, ``beta``, ``valid``, ``errors``, ``clamp`` (keyword only, with ``head``): DENSE REGRESSION with the
        probe -- the other dense probing protocol: a 1x1 ``Conv2d(C, N)`` trained on depth (N = 1) or flow, normals, colour (N = 2, 3)
        under a validity mask, and for depth scored with RMSE, abs-rel and delta < 1.25^k.  ``dense_target`` is a float tensor
        [B, N, Ho, Wo] on the features' device (any strides; other float dtypes are converted to float32), ``valid`` a bool / uint8
        [B, Ho, Wo] mask or None (a pixel is valid for all N channels alike; what lies under an invalid pixel, NaN included, reaches
        nothing).  With ``sel`` = ``valid`` broadcast over the channels the call returns, for ``reduction`` "mean" / "sum",
            ``F.l1_loss(head(naf(...)).float()[sel], dense_target.float()[sel], reduction=reduction)``        (``dense_loss="l1"``)
        or ``F.mse_loss`` (``"mse"``) or ``F.smooth_l1_loss(..., beta=beta)`` (``"smooth_l1"``): a 0-dim fp32 tensor; ``reduction="none"`` returns
        the [B, Ho, Wo] map of the channel sums of the elementwise loss, 0 where invalid; ``"mean"`` without a valid pixel is nan.
        ``predict=True`` additionally returns the prediction ``head(naf(...))`` as fp32 [B, N, Ho, Wo] from the same launch:
        ``(loss, prediction)``.  For N <= 32 the loss map, its gradient and the prediction come from the head-summed kernel's epilogue
        (``ops.xna_head_regression``: the fp32 logits, the boolean gather and the loss's autograd graph never exist); more outputs, or a
        geometry the kernel does not serve, compose the logits call with the same expressions.  ``errors`` (N = 1): the probe's
        EVALUATION.  ``errors=True`` returns a fresh float64 [10] tensor of this call's error sums, ``errors=acc`` ADDS them to the
        float64 [10] tensor ``acc`` and returns it, so a validation loop passes one accumulator for every batch and never synchronises
        with the host: over the pixels that are valid, have ``dense_target > 0`` and a finite target and prediction, with
        ``p = clamp(prediction, *clamp)`` (default ``clamp=(1e-3, inf)``; it applies to these statistics only) and ``d = ln p - ln t``:
        ``n, sum |p - t|, sum (p - t)^2, sum |p - t| / t, sum (p - t)^2 / t, sum d, sum d^2`` and the counts of
        ``max(p / t, t / p) < 1.25^k``, k = 1, 2, 3.  ``naf_amd.depth_metrics(acc)`` turns them into MAE, RMSE, abs-rel, sq-rel, RMSE-log,
        SILog and delta_1..3, ``naf_amd.dist.reduce_errors(acc)`` sums them over ranks.  The call returns the sums IN PLACE OF the loss
        (``(sums, prediction)`` with ``predict=True``), is never differentiable, adds without float atomics (bit-reproducible) and
        runs the inference kernels whatever the gradient mode.  The gradient modes of the loss are those of ``target=``: frozen upsampler
        and a probe that requires grad -- fused and differentiable with respect to the probe (``ops.XnaHeadRegFunction``); no gradient
        wanted -- the kernel with rotate-on-load; a gradient for the upsampler, the image or the features -- the unfused composition on
        ``forward_train``.  ``image`` may be a ``Guidance``.  ValueError, before any device work: ``dense_target`` without ``head`` or together
        with ``target``, ``confusion``, ``regress``, ``cosine``, ``masks`` or ``return_weights``; ``valid``, ``errors`` or ``clamp`` without
        ``dense_target``; a wrong shape or device; ``dense_loss`` outside the three values; ``beta <= 0``; ``errors`` with N != 1.
        Not offered: scale-invariant log loss as a training loss (it is not separable per pixel), per-element masks, ``capture()`` of this call."""
        if dense_target is not None:
            if head is None:
                raise ValueError("naf(..., dense_target=...) is the regression objective of a probe: pass head=probe as well")
            if (target is not None or (confusion is not None and confusion is not False) or regress is not None or cosine or masks is not None
                    or return_weights or loss is not None):
                raise ValueError("naf(..., dense_target=...) does not combine with target / confusion / regress / cosine / masks / return_weights")
            return self._forward_head_regression(image, features, output_size, head, dense_target, dense_loss, beta, valid, errors, clamp,
                                                 reduction, bool(predict))
        if valid is not None or (errors is not None and errors is not False) or clamp is not None:
            raise ValueError("naf(..., valid= / errors= / clamp=) belong to the dense regression objective: pass head=probe and dense_target=... as well")
        if masks is not None:
            if (head is not None or target is not None or predict or (confusion is not None and confusion is not False) or regress is not None
                    or return_weights or cosine or loss is not None):
                raise ValueError("naf(..., masks=...) pools the features themselves: it does not combine with head / target / predict / confusion / "
                                 "regress / return_weights / cosine")
            return self._forward_masks(image, features, output_size, masks, mask_reduce, mask_path, bool(return_attention))
        if return_attention:
            raise ValueError("naf(..., return_attention=True) goes with masks=...")
        if loss is not None:
            if loss != "ce":
                raise ValueError(f"loss must be None or 'ce', got {loss!r}")
            if not cosine:
                raise ValueError("naf(..., loss='ce') is the objective of the cosine head: pass head=E and cosine=True as well "
                                 "(a linear probe's cross-entropy is head=probe, target=...)")
        if cosine:
            return self._forward_cosine(image, features, output_size, return_weights, head, target, ignore_index, reduction, predict, confusion,
                                        regress, logit_scale, return_norms, cosine_path, loss)
        if isinstance(image, Guidance):
            self._check_guidance_call(image, features, return_weights, regress, confusion)
        if regress is not None:
            if head is not None or target is not None or predict or (confusion is not None and confusion is not False) or return_weights:
                raise ValueError("naf(..., regress=...) is the regression objective of the features themselves: it does not combine with "
                                 "head / target / predict / confusion / return_weights")
            return self._forward_regress(image, features, output_size, regress, regress_path)
        if confusion is not None and confusion is not False:
            if head is None or target is None:
                raise ValueError("naf(..., confusion=...) is the evaluation of a probe against a target: pass head=probe and target=... as well")
            return self._forward_head_confusion(image, features, output_size, return_weights, head, target, ignore_index, reduction, bool(predict), confusion)
        if target is not None or predict:
            if head is None:
                raise ValueError("naf(..., target=... / predict=True) is the objective of a probe: pass head=probe as well")
            return self._forward_head_objective(image, features, output_size, return_weights, head, target, ignore_index, reduction, bool(predict))
        if head is not None:
            return self._forward_head(image, features, output_size, return_weights, head)
        if self._wants_grad(image, features):
            # the library's own differentiable stem whenever it serves the width, with or without torch.autocast (round 6: the
            # bf16-activation contract is what the inference path computes); else the torch stem in the ambient precision.
            # return_weights (attentions.py:64-67 under autograd): (out, scores); True: scores without a gradient, "differentiable": with one
            return self.forward_train(image, features, output_size, amp="auto", return_weights=return_weights)
        with torch.no_grad():
            return self._forward_inference(image, features, output_size, return_weights)

    def _forward_masks(self, image, features, output_size, masks, reduce, path, return_attention):
        """``forward(..., masks=M)``: see ``forward``.  Every refusal comes before anything touches the device.  On the composed route
        ``A`` of ``return_attention`` comes from the materialised scores (``return_weights=True``, ``ops.mask_attention_from_scores``),
        without a gradient."""
        if reduce not in ops._MASK_REDUCE:
            raise ValueError(f"mask_reduce must be one of {ops._MASK_REDUCE}, got {reduce!r}")
        if path not in ops._HEAD_PATHS:
            raise ValueError(f"mask_path must be one of {ops._HEAD_PATHS}, got {path!r}")
        if not isinstance(features, torch.Tensor) or features.dim() != 4 or image.dim() != 4 or image.shape[0] != features.shape[0]:
            raise ValueError(f"expected image [B,3,H,W] and features [B,C,h,w], got {tuple(image.shape)} / {tuple(getattr(features, 'shape', ()))}")
        ho, wo = int(output_size[0]), int(output_size[1])
        B, C = features.shape[0], features.shape[1]
        ops.check_masks("naf(..., masks=...)", masks, (B, None, ho, wo), features.device)
        if not (image.is_cuda and features.is_cuda):
            raise _rocm_only(image=image, features=features)
        if isinstance(image, Guidance):
            self._check_guidance_call(image, features, False, None, None)
        K = int(masks.shape[1])
        heads, ksz, enc = self.upsampler.num_heads, self.upsampler.kernel_size, self.image_encoder
        lr = features.shape[-2:]
        reason = None       # why the fused kernel does not take the call
        if B == 0:
            reason = "an empty batch"
        elif self._wants_grad(image, features):
            reason = "the fused mask-pooling kernel is inference-only and the call wants a gradient for the upsampler or its inputs"
        elif features.dtype != torch.bfloat16:
            reason = f"the fused mask-pooling route reads bfloat16 features, got {features.dtype}"
        elif C % heads or enc.out_channels % heads:
            reason = f"feature channels {C} / guidance channels {enc.out_channels} not divisible by {heads} heads"
        else:
            probe = torch.empty((B, ho, wo, heads, enc.out_channels // heads), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
            if ops.xna_mask_pool_select(probe, lr, min(K, ops.MASK_POOL_CHUNK), ksz) != "fused":
                reason = _lib_last_error() or "naf_xna_maskpool_select refuses the geometry"
        if path == "fused" and reason is not None:
            raise ops._lib.NafHipError(f"naf(..., masks=..., mask_path='fused'): {reason}")
        if path == "composed" or reason is not None:
            with ops._Timed("mask_pool_composed"):
                A = None
                if B == 0:
                    f = torch.empty((0, C, ho, wo), dtype=features.dtype, device=features.device)
                    A = torch.empty((0, heads, K, *lr), dtype=torch.float32, device=features.device)
                elif return_attention:
                    f, scores = self.forward(image, features, output_size, return_weights=True)
                    with torch.no_grad():
                        A = ops.mask_attention_from_scores(scores, masks, lr, ksz)
                else:
                    f = self.forward(image, features, output_size)
                pooled, mass = ops.mask_pool_from_features(f, masks, reduce, return_mass=True)
            return (pooled, A, mass) if return_attention else pooled
        with torch.no_grad():
            kc = min(K, ops.MASK_POOL_CHUNK)
            fusable = lambda q5, tabs: ops.xna_mask_pool_select(q5, lr, kc, ksz, rope_tables=tabs) == "fused"
            q5, k5, tabs = self.guidance_qk(image, lr, (ho, wo), fusable=fusable)
            with ops._Timed("attention"):
                A, mass = ops.xna_mask_pool(q5, k5, masks, ksz, scale=self.upsampler.scale, rope_tables=tabs)
                pooled = ops.mask_pool_apply(A, features, mass, reduce)
        return (pooled, A, mass) if return_attention else pooled

    def _wants_grad(self, *inputs) -> bool:
        """This call wants a gradient for the upsampler or its ``inputs`` (image or ``Guidance``, features): gradient mode with an input
        that requires one, or ``.train()`` with trainable parameters.  Such calls take the training path."""
        return torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or
                                            (self.training and any(p.requires_grad for p in self.parameters())))

    # ---- encode the image once ------------------------------------------------------------------------------------------------
    def guide(self, image: torch.Tensor, output_size=None) -> Guidance:
        """The image-side state of a call, for reuse: ``g = naf.guide(image)``, then ``naf(g, feats, size)`` for any number of feature
        maps, grids, dtypes, sizes and modes (see ``Guidance`` and ``forward``).  ``output_size``: build that level now (stem and
        pooling) instead of on the first call.  Always the inference encoder (bf16 stem, deterministic RoPE coordinates)."""
        g = Guidance(self, image)
        if output_size is not None:
            g.pooled(int(output_size[0]), int(output_size[1]))
        return g

    def _check_guidance_call(self, g: Guidance, features, return_weights, regress, confusion) -> None:
        """What ``forward`` refuses of a call whose image is a ``Guidance``, each with its reason."""
        if regress is not None:
            raise ValueError("naf(guidance, ..., regress=...): the regression objective trains the encoder, a Guidance holds the frozen "
                             "encoder's output; pass the image")
        if isinstance(return_weights, str) and _scores_mode(return_weights) == "differentiable":
            raise ValueError("naf(guidance, ..., return_weights='differentiable'): the scores' gradient reaches the encoder, a Guidance holds "
                             "the frozen encoder's output; pass the image (return_weights=True works)")
        g.check(self)
        evaluation = confusion is not None and confusion is not False        # never differentiable, whatever the gradient mode
        if not evaluation and self._wants_grad(g, *([features] if isinstance(features, torch.Tensor) else [])):
            raise RuntimeError("naf(guidance, ...): this call wants a gradient for the upsampler, the image or the features (gradient mode with an "
                               "input that requires grad, or .train() with trainable parameters) and would take the training path; a Guidance "
                               "serves inference calls -- use torch.no_grad() / .eval() / requires_grad_(False), or pass the image")

    def query(self, guidance, points, features=None, output_size=None, weights="logits", lr_size=None) -> PointQuery:
        """The attention at N pixels: ``naf.query(g, points, features=feats, output_size=(Ho, Wo), weights="logits")``.

        ``guidance``: a ``Guidance`` (or an image, encoded for this call).  ``points``: an integer tensor [N, 3] of (b, y, x) in output
        coordinates -- [N, 2] of (y, x) when the batch is 1 -- on any device.  ``weights``: "logits" (the scaled pre-softmax scores: the
        rows of what ``return_weights=True`` returns), "softmax", "both" or None.  ``features`` [B, C, h, w]: also the upsampled feature
        vectors of the points; without them pass ``lr_size=(h, w)``, the grid the keys are pooled to.  Returns ``PointQuery(features [N, C]
        fp32 or None, logits, probs [N, heads, k*k] fp32 or None, window_y [N, k], window_x [N, k] int32)``: the windows are the low-res
        rows / columns each point attends to (duplicates included), taken from the index tables on the device.  A point outside the grid
        gets NaN rows and -1 windows.  No dense score tensor or feature map is formed (``ops.xna_points``); where the RoPE heads are the
        attention heads and no rotated queries are cached the kernel rotates the N vectors it reads, so no query tensor is written either.
        Keys come from the ``Guidance``'s cache; values go through ``ops.pack_values`` (fp32 features are read as bf16, as everywhere).
        Nothing synchronises with the host."""
        if weights not in ("logits", "softmax", "both", None):
            raise ValueError(f"query: weights must be 'logits', 'softmax', 'both' or None, got {weights!r}")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] not in (2, 3):
            raise ValueError("query: points must be an integer tensor [N, 3] of (b, y, x), or [N, 2] of (y, x) for a batch of 1; got "
                             + (f"{tuple(points.shape)}" if isinstance(points, torch.Tensor) else type(points).__name__))
        if points.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise TypeError(f"query: points must be an integer tensor, got {points.dtype}")
        if output_size is None:
            raise ValueError("query: output_size=(Ho, Wo) is required: the points are in its coordinates")
        ho, wo = int(output_size[0]), int(output_size[1])
        if features is not None:
            if not isinstance(features, torch.Tensor) or features.dim() != 4:
                raise ValueError("query: features must be [B, C, h, w]")
            if lr_size is not None and (int(lr_size[0]), int(lr_size[1])) != tuple(features.shape[-2:]):
                raise ValueError(f"query: lr_size {tuple(lr_size)} contradicts the features' grid {tuple(features.shape[-2:])}")
            if features.shape[1] % self.upsampler.num_heads:
                raise ValueError(f"feature channels {features.shape[1]} not divisible by {self.upsampler.num_heads} heads")
            h, w = int(features.shape[-2]), int(features.shape[-1])
        elif lr_size is None:
            raise ValueError("query: without features pass lr_size=(h, w), the grid the keys are pooled to")
        else:
            h, w = int(lr_size[0]), int(lr_size[1])
        if features is None and weights is None:
            raise ValueError("query: nothing asked for: no features and weights=None")
        g = guidance if isinstance(guidance, Guidance) else self.guide(guidance)
        g.check(self)
        B = g.shape[0]
        if features is not None and (features.shape[0] != B or not features.is_cuda):
            if features.shape[0] != B:
                raise ValueError(f"query: features of batch {features.shape[0]}, image of batch {B}")
            raise _rocm_only(features=features)
        if points.shape[1] == 2 and B != 1:
            raise ValueError(f"query: [N, 2] points name no image; the batch is {B}, pass [N, 3] of (b, y, x)")
        dev = g.device
        with torch.no_grad():
            pts = points.to(device=dev, dtype=torch.int32)
            if pts.shape[1] == 2:
                pts = torch.cat([torch.zeros_like(pts[:, :1]), pts], dim=1)
            pts = pts.contiguous()
            enc, heads, ksz = self.image_encoder, self.upsampler.num_heads, self.upsampler.kernel_size
            heads_rope = enc.rope.num_heads
            same = heads == heads_rope
            tabs = None
            q5 = None
            if same and self.fuse_rope and (ho, wo) not in g._queries:
                x = g.pooled(ho, wo)
                xq = x.permute(0, 2, 3, 1)
                if x.dtype == torch.bfloat16 and xq.stride(3) == 1:     # the un-rotated guidance: the kernel rotates the vectors it reads
                    q5 = xq.unflatten(3, (heads_rope, x.shape[1] // heads_rope)).permute(0, 3, 1, 2, 4)
                    tabs = g.tables(ho, wo)
                    _, k5 = g.queries_keys(ho, wo, (h, w), heads_rope, "head_major", need_q=False)
            if q5 is None:
                q5, k5, _ = self.guidance_qk(g, (h, w), (ho, wo))
            v5 = None
            if features is not None:
                C_ = features.shape[1]
                v5 = ops.pack_values(features).view(B, h, w, heads, C_ // heads).permute(0, 3, 1, 2, 4)
            with ops._Timed("attention"):
                out, logits, probs = ops.xna_points(q5, k5, v5, pts, ksz, want_logits=weights in ("logits", "both"),
                                                    want_probs=weights in ("softmax", "both"), scale=self.upsampler.scale, rope_tables=tabs)
            iy = ops.device_index_table(ho, h, ksz[0], dev)
            ix = ops.device_index_table(wo, w, ksz[1], dev)
            py, px = pts[:, 1].long(), pts[:, 2].long()
            ok = ((pts[:, 0] >= 0) & (pts[:, 0] < B) & (py >= 0) & (py < ho) & (px >= 0) & (px < wo))[:, None]
            win_y = torch.where(ok, iy[py.clamp(0, ho - 1)], -1)
            win_x = torch.where(ok, ix[px.clamp(0, wo - 1)], -1)
        return PointQuery(out, logits, probs, win_y, win_x)

    def locate(self, image, features, output_size, embeddings, *, topk=1, logit_scale=1.0, path="auto") -> Peaks:
        """Where in the upsampled map each of N vectors matches best: ``naf.locate(image_or_guidance, feats, (Ho, Wo), E, topk=k)``.

        With ``cos`` what ``naf(image, feats, size, head=E, cosine=True, logit_scale=s)`` returns, every low-res cell (the ``Ho / h`` x
        ``Wo / w`` block of pixels it is upsampled to; the ratio must be an integer, ValueError otherwise) yields the maximum of ``cos[b, n]``
        over its pixels and the lowest flat index ``y * Wo + x`` among the pixels that attain it; the ``topk`` best cells per (b, n), by value
        descending, then by index ascending, are returned as a ``Peaks``.  One candidate per cell: a non-maximum suppression at the cell
        grid, not the k best pixels; ``topk=1`` is the global maximum with the lowest flat index among ties.  A pixel whose feature is zero
        has cosine 0 and takes part like any other.  ``embeddings`` takes the forms ``cosine=True`` takes; ``image`` may be a ``Guidance``.
        Inference only: runs under ``no_grad`` whatever the mode.  ``path="auto"``: the peak epilogue of the cosine kernel
        (``ops.xna_cos_peaks``: the [B, N, Ho, Wo] map is never allocated; more than 256 vectors run in chunks of 256) wherever
        ``naf_xna_cos_peaks_select`` grants it, else the composition (the cosine call, then torch reductions with the same tie rule): fp16 /
        fp32 features, windows 13 / 15 with more than 64 vectors.  ``"fused"`` insists (NafHipError with the library's reason),
        ``"composed"`` is the A/B arm.  1 <= topk <= min(h * w, 64).  Every refusal comes before any device work."""
        if path not in ("auto", "fused", "composed"):
            raise ValueError(f"locate: path must be 'auto', 'fused' or 'composed', got {path!r}")
        if not isinstance(features, torch.Tensor) or features.dim() != 4 or image.dim() != 4 or image.shape[0] != features.shape[0]:
            raise ValueError(f"expected image [B,3,H,W] and features [B,C,h,w], got {tuple(image.shape)} / {tuple(getattr(features, 'shape', ()))}")
        weight = _cosine_head(embeddings, features.shape[1])
        if not math.isfinite(float(logit_scale)):
            raise ValueError(f"logit_scale must be finite, got {logit_scale}")
        ho, wo = int(output_size[0]), int(output_size[1])
        B, C, N = features.shape[0], features.shape[1], weight.shape[0]
        h, w = int(features.shape[-2]), int(features.shape[-1])
        if ho % h or wo % w:
            raise ValueError(f"locate: {ho}x{wo} pixels over {h}x{w} cells is not an integer ratio: there are no cells")
        if ho * wo >= 2 ** 31:
            raise ValueError(f"locate: {ho}x{wo} pixels do not fit an int32 flat index")
        k = int(topk)
        if k != topk or not 1 <= k <= min(h * w, 64):
            raise ValueError(f"locate: topk must be an integer in 1 .. min(h * w, 64) = {min(h * w, 64)}, got {topk!r}")
        if not (image.is_cuda and features.is_cuda and weight.is_cuda):
            raise _rocm_only(image=image, features=features, embeddings=weight)
        if isinstance(image, Guidance):
            image.check(self)
        dev = features.device
        if B == 0 or N == 0:
            z = lambda *sh, dt=torch.float32: torch.empty(sh, dtype=dt, device=dev)
            return Peaks(z(B, N, k), z(B, N, k, dt=torch.int64), z(B, N, k, dt=torch.int64), z(B, N, h, w), z(B, N, h, w, dt=torch.int32))
        heads, ksz, enc = self.upsampler.num_heads, self.upsampler.kernel_size, self.image_encoder
        chunks = sorted({min(N, 256), N % 256 or min(N, 256)})      # the sizes ops.xna_cos_peaks launches
        with torch.no_grad():
            reason = None       # why the fused kernel does not take the call
            if features.dtype != torch.bfloat16:
                reason = f"the fused kernel reads bfloat16 features, got {features.dtype}"
            elif C % heads or enc.out_channels % heads:
                reason = f"feature channels {C} / guidance channels {enc.out_channels} not divisible by {heads} heads"
            else:
                probe = torch.empty((B, ho, wo, heads, enc.out_channels // heads), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
                for n in chunks:
                    if reason is None and ops.xna_cos_peaks_select(probe, (h, w), C // heads, n, ksz) != "fused":
                        reason = _lib_last_error() or f"naf_xna_cos_peaks_select refuses {n} embeddings"
            if path == "fused" and reason is not None:
                raise ops._lib.NafHipError(f"naf.locate(..., path='fused'): {reason}")
            if path == "composed" or reason is not None:
                with ops._Timed("locate_composed"):
                    cos = self.forward(image, features, (ho, wo), head=weight, cosine=True, logit_scale=logit_scale)
                    peak, where = ops.peaks_from_cosines(cos, (h, w))
                    del cos
            else:
                fusable = lambda q5, tabs: all(ops.xna_cos_peaks_select(q5, (h, w), C // heads, n, ksz, rope_tables=tabs) == "fused" for n in chunks)
                q5, k5, tabs = self.guidance_qk(image, (h, w), (ho, wo), fusable=fusable)
                v5 = ops.pack_values(features).view(B, h, w, heads, C // heads).permute(0, 3, 1, 2, 4)
                with ops._Timed("attention"):
                    peak, where, _ = ops.xna_cos_peaks(q5, k5, v5, weight, ksz, logit_scale=logit_scale, path="fused", scale=self.upsampler.scale,
                                                       rope_tables=tabs)
            scores, index = ops.peaks_topk(peak, where, k)
            index = index.long()
            return Peaks(scores, index // wo, index % wo, peak, where)

    def match(self, src, src_features, points, dst, dst_features, output_size, *, topk=1, mutual=False) -> Match:
        """Keypoint transfer: find the pixels of ``points`` of one image in another.  ``src`` and ``dst`` are ``Guidance`` objects of the same
        batch size, ``points`` as for ``query`` ([P, 3] of (b, y, x), [P, 2] for a batch of 1; inside the grid -- a point outside has a NaN
        vector and no match).  The call is ``query(src, points, features=src_features, output_size=output_size).features`` followed by
        ``locate(dst, dst_features, output_size, those, topk=topk)``, read for every point in the destination image of the point's batch
        index.  ``mutual=True`` also goes the way back -- ``query`` at the best locations in ``dst``, ``locate`` in ``src`` -- and reports
        the round-trip pixel distance per point, the usual cycle-consistency filter (0 is not guaranteed for a perfect match: another
        pixel may tie within the arithmetic's error).  Returns a ``Match``.  Pure host glue over the two calls."""
        if not isinstance(src, Guidance) or not isinstance(dst, Guidance):
            raise TypeError(f"match: src and dst must be Guidance objects (naf.guide(image)), got {type(src).__name__} / {type(dst).__name__}")
        if src.shape[0] != dst.shape[0]:
            raise ValueError(f"match: src holds {src.shape[0]} images, dst {dst.shape[0]}")
        with torch.no_grad():
            vec = self.query(src, points, features=src_features, output_size=output_size, weights=None).features
            dev = vec.device
            pts = points.to(device=dev, dtype=torch.int64)
            bidx = pts[:, 0] if pts.shape[1] == 3 else torch.zeros(pts.shape[0], dtype=torch.int64, device=dev)
            bsel = bidx.clamp(0, dst.shape[0] - 1)
            rows = torch.arange(pts.shape[0], device=dev)
            there = self.locate(dst, dst_features, output_size, vec, topk=topk)
            scores, y, x = there.scores[bsel, rows], there.y[bsel, rows], there.x[bsel, rows]
            distance = None
            if mutual:
                found = torch.stack([bsel, y[:, 0], x[:, 0]], dim=1)
                back = self.locate(src, src_features, output_size, self.query(dst, found, features=dst_features, output_size=output_size,
                                                                              weights=None).features, topk=1)
                by, bx = back.y[bsel, rows, 0], back.x[bsel, rows, 0]
                distance = ((by - pts[:, -2]).float().square() + (bx - pts[:, -1]).float().square()).sqrt()
        return Match(scores, y, x, distance)

    # ---- k-means on the upsampled features ---------------------------------------------------------------------------------------
    def kmeans_path(self, features, output_size, k: int) -> str:
        """The route ``kmeans(..., path="auto")`` takes for these features, output size and cluster count: "fused" or "composed".  A
        host-side query (``ops.xna_kmeans_select``); the reason for "composed" is the second element of ``_kmeans_reason``."""
        return "composed" if self._kmeans_reason(features, (int(output_size[0]), int(output_size[1])), int(k)) is not None else "fused"

    def _kmeans_reason(self, features, size, K: int):
        """Why the one-launch step does not take the call, or None."""
        heads, ksz, enc = self.upsampler.num_heads, self.upsampler.kernel_size, self.image_encoder
        B, C = features.shape[0], features.shape[1]
        if K > ops.KMEANS_FUSED_MAX:
            return f"the fused k-means step takes at most {ops.KMEANS_FUSED_MAX} clusters, got {K}"
        if features.dtype != torch.bfloat16:
            return f"the fused k-means route reads bfloat16 features, got {features.dtype}"
        if C % heads or enc.out_channels % heads:
            return f"feature channels {C} / guidance channels {enc.out_channels} not divisible by {heads} heads"
        probe = torch.empty((max(B, 1), size[0], size[1], heads, enc.out_channels // heads), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
        if ops.xna_kmeans_select(probe, features.shape[-2:], K, ksz) != "fused":
            return _lib_last_error() or "naf_xna_kmeans_select refuses the geometry"
        return None

    def kmeans(self, image, features, output_size, k, *, iters=10, init="points", generator=None, per_image=True, path="auto") -> KMeans:
        """K-means (Lloyd) over the upsampled features of one call, without writing them: ``r = naf.kmeans(image_or_guidance, feats, (Ho, Wo), k)``
        returns ``KMeans(labels, centroids, counts, shift)`` -- an unsupervised segmentation, the companion picture of the PCA view.

        One iteration is, with ``c`` the centroids [B, K, C] fp32,

            pv5, bias, _ = ops.project_kmeans_values(c, feats, heads)               # centred: argmax_k c_k . f - |c_k|^2 / 2
            labels       = the head kernel's argmax of (pv5[b], bias[b]) per image  # the lowest index among equal maxima
            A, mass      = ops.xna_mask_pool(q, k, labels == arange(K))             # the attention summed under the one-hot masks
            sums         = ops.mask_pool_apply(A, feats, None, "sum")
            c_new        = where(mass > 0, sums / mass, c)                          # an empty cluster keeps its centroid
            shift[i]     = max_k |c_new - c|

        which is also the ``path="composed"`` arm.  ``path="auto"`` runs labels and accumulation of an iteration in ONE launch
        (``ops.xna_kmeans_step``; no label map, no one-hot tensor) where ``naf_xna_kmeans_select`` grants the geometry, k <= 64 and the
        features are bf16 -- bit for bit the same labels, centroids, counts and shift -- and the composition otherwise: 64 < k <= 256,
        fp16 / fp32 features, geometries the head route composes (those materialise the feature map).  ``"fused"`` insists (NafHipError
        with the library's reason).  After ``iters`` updates one more labels-only launch per image assigns the pixels to the final
        centroids through ``r.head(b)`` -- the centroids as a plain linear head, the call ``naf(g, feats, size, head=r.head(b),
        predict=True)`` makes, so that call returns ``r.labels[b]`` bit for bit: the returned ``labels``; ``counts`` are their masses.  ``iters`` is fixed: there is no tolerance and no early stop (it would
        synchronise with the host); ``shift`` is the record to read afterwards.  ``init="points"`` draws k distinct pixels per image with
        ``torch.randperm`` on the host from ``generator`` (default: a fixed seed) and takes their features (``query``); ``init`` may also
        be a tensor [K, C] or [B, K, C].  ``per_image=False`` shares one set of centroids: sums and masses are added over the batch before
        the division.  The image is encoded once for all iterations; a ``Guidance`` is accepted.  Inference only (``no_grad``).
        k > 256, k < 1 and iters < 0 raise ValueError before any device work.
        Not offered: a gradient, cosine / spherical k-means, k-means++ seeding, ``capture()``."""
        who = "kmeans"
        if path not in ("auto", "fused", "composed"):
            raise ValueError(f"{who}: path must be 'auto', 'fused' or 'composed', got {path!r}")
        K, iters_ = int(k), int(iters)
        if K != k or K < 1 or K > ops.KMEANS_MAX:
            raise ValueError(f"{who}: k must be an integer in 1 .. {ops.KMEANS_MAX}, got {k!r}")
        if iters_ != iters or iters_ < 0:
            raise ValueError(f"{who}: iters must be a non-negative integer, got {iters!r}")
        if not isinstance(features, torch.Tensor) or features.dim() != 4 or image.dim() != 4 or image.shape[0] != features.shape[0]:
            raise ValueError(f"expected image [B,3,H,W] and features [B,C,h,w], got {tuple(image.shape)} / {tuple(getattr(features, 'shape', ()))}")
        ho, wo = int(output_size[0]), int(output_size[1])
        B, C = int(features.shape[0]), int(features.shape[1])
        heads, ksz = self.upsampler.num_heads, self.upsampler.kernel_size
        if B < 1:
            raise ValueError(f"{who}: an empty batch has nothing to cluster")
        if C % heads:
            raise ValueError(f"feature channels {C} not divisible by {heads} heads")
        if isinstance(init, torch.Tensor):
            if tuple(init.shape) not in ((K, C), (B, K, C)) or not init.is_floating_point():
                raise ValueError(f"{who}: init must be 'points' or a floating-point tensor [K, C] = ({K}, {C}) or [B, K, C], got {tuple(init.shape)} {init.dtype}")
            if not per_image and init.dim() == 3:
                raise ValueError(f"{who}: per_image=False shares one set of centroids: init must be [K, C]")
        elif init != "points":
            raise ValueError(f"{who}: init must be 'points' or a tensor, got {init!r}")
        elif K > ho * wo:
            raise ValueError(f"{who}: cannot draw {K} distinct pixels from {ho}x{wo}")
        if features.dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise TypeError(f"{who}: features must be bfloat16, float16 or float32, got {features.dtype}")
        if not (image.is_cuda and features.is_cuda) or (isinstance(init, torch.Tensor) and not init.is_cuda):
            raise _rocm_only(image=image, features=features, **({"init": init} if isinstance(init, torch.Tensor) else {}))
        reason = self._kmeans_reason(features, (ho, wo), K)
        if path == "fused" and reason is not None:
            raise ops._lib.NafHipError(f"naf.kmeans(..., path='fused'): {reason}")
        fused = path != "composed" and reason is None
        dev, lr = features.device, tuple(features.shape[-2:])
        with torch.no_grad():
            g = image if isinstance(image, Guidance) else self.guide(image)
            g.check(self)
            if isinstance(init, torch.Tensor):
                c = init.to(device=dev, dtype=torch.float32)
                c = (c[None].expand(B, K, C) if c.dim() == 2 else c).contiguous()
            else:
                gen = generator if generator is not None else torch.Generator().manual_seed(0)
                nb = B if per_image else 1
                flat = torch.stack([torch.randperm(ho * wo, generator=gen)[:K] for _ in range(nb)])          # host
                pts = torch.stack([torch.arange(nb)[:, None].expand(nb, K), flat // wo, flat % wo], dim=2).reshape(nb * K, 3)
                c = self.query(g, pts, features=features, output_size=(ho, wo), weights=None).features.reshape(nb, K, C)
                c = c.expand(B, K, C).contiguous()
            # can the (un-rotated guidance, tables) form serve every launch of the route?
            if fused:
                fusable = lambda q5, tabs: ops.xna_kmeans_select(q5, lr, K, ksz, rope_tables=tabs) == "fused" and \
                    ops.xna_head_select(q5[:1], lr, K, ksz, rope_tables=tabs) == "fused"
            else:
                fusable = lambda q5, tabs: ops.xna_head_select(q5[:1], lr, K, ksz, rope_tables=tabs) == "fused" and \
                    ops.xna_mask_pool_select(q5, lr, min(K, ops.MASK_POOL_CHUNK), ksz, rope_tables=tabs) == "fused"
            q5, k5, tabs = self.guidance_qk(g, lr, (ho, wo), fusable=fusable)
            pooled_ok = fused or ops.xna_mask_pool_select(q5, lr, min(K, ops.MASK_POOL_CHUNK), ksz, rope_tables=tabs) == "fused"
            fmap = None if pooled_ok else self.forward(g, features, (ho, wo)).float()      # geometries the head route composes
            scale = self.upsampler.scale
            arange = torch.arange(K, device=dev)

            def assign(pv5, bias):
                """The head kernel's labels per image (each image has its own bias row)."""
                return torch.cat([ops.xna_head_objective(q5[b:b + 1], k5[b:b + 1], pv5[b:b + 1], bias[b], ksz, n_out=K, want_labels=True,
                                                         scale=scale, rope_tables=tabs)[1] for b in range(B)])

            def sums_of(A):
                if features.dtype == torch.bfloat16:
                    return ops.mask_pool_apply(A, features, None, "sum")
                return torch.einsum("bgkj,bgdj->bkgd", A.flatten(3), features.float().reshape(B, heads, C // heads, -1)).reshape(B, K, C)

            shift = torch.empty((iters_, B), dtype=torch.float32, device=dev)
            for it in range(iters_):
                pv5, bias, _ = ops.project_kmeans_values(c, features, heads)
                with ops._Timed("attention"):
                    if fused:
                        _, A, mass = ops.xna_kmeans_step(q5, k5, pv5, bias, ksz, scale=scale, rope_tables=tabs)
                        sums = sums_of(A)
                    else:
                        onehot = assign(pv5, bias)[:, None] == arange[None, :, None, None]
                        if pooled_ok:
                            A, mass = ops.xna_mask_pool(q5, k5, onehot, ksz, scale=scale, rope_tables=tabs)
                            sums = sums_of(A)
                        else:
                            sums, mass = ops.mask_pool_from_features(fmap, onehot, "sum", return_mass=True)
                        del onehot
                if not per_image:
                    sums, mass = sums.sum(dim=0, keepdim=True).expand(B, K, C), mass.sum(dim=0, keepdim=True).expand(B, K)
                c_new = torch.where(mass[..., None] > 0, sums / mass[..., None], c)
                shift[it] = (c_new - c).norm(dim=2).amax(dim=1)
                c = c_new
            # the final assignment is the call ``KMeans.head`` documents -- the centroids as a plain linear head on the features as they
            # are -- so that ``naf(g, feats, size, head=r.head(b), predict=True)[b]`` IS ``r.labels[b]``, bit for bit
            cents = c if per_image else c[:1]
            labels = []
            for b in range(cents.shape[0]):
                pvh, bh = ops.project_head_values(*_kmeans_head(cents[b]), features, heads)
                sl = slice(b, b + 1) if per_image else slice(None)
                labels.append(ops.xna_head_objective(q5[sl], k5[sl], pvh[sl], bh, ksz, n_out=K, want_labels=True, scale=scale, rope_tables=tabs)[1])
            labels = torch.cat(labels)
            counts = torch.zeros((B, 256), dtype=torch.float32, device=dev)
            counts.scatter_add_(1, labels.reshape(B, -1).long(), torch.ones((B, ho * wo), dtype=torch.float32, device=dev))
            return KMeans(labels.long(), c if per_image else c[0].clone(), counts[:, :K].contiguous(), shift)

    def _forward_regress(self, image, features, output_size, regress, regress_path):
        """``forward(..., regress=regress)``: see ``forward``."""
        if regress_path not in ("auto", "fused", "composed"):
            raise ValueError(f"regress_path must be 'auto', 'fused' or 'composed', got {regress_path!r}")
        if features.dim() != 4 or image.dim() != 4 or image.shape[0] != features.shape[0]:
            raise ValueError(f"expected image [B,3,H,W] and features [B,C,h,w], got {tuple(image.shape)} / {tuple(features.shape)}")
        ho, wo = int(output_size[0]), int(output_size[1])
        B, C = features.shape[:2]
        ops._check_regress_target("naf(..., regress=...)", regress, (B, C, ho, wo), features.device)
        if not (image.is_cuda and features.is_cuda):
            raise _rocm_only(image=image, features=features)
        composed = lambda: F.mse_loss(self.forward(image, features, output_size).float(), regress.float())
        if regress_path == "composed" or (B == 0 and regress_path == "auto"):
            return composed()
        if self._wants_grad(image, features):
            return self.forward_train(image, features, output_size, amp="auto", regress=regress, regress_path=regress_path)
        enc, heads, ksz = self.image_encoder, self.upsampler.num_heads, self.upsampler.kernel_size
        hip_stem = enc.use_encoder and enc.stem_impl == "hip" and enc._hip_stem_ok() and enc.rope.num_heads == heads
        if regress_path == "auto":
            out_dtype = torch.bfloat16 if features.dtype == torch.bfloat16 else torch.float32
            if not (hip_stem and C % heads == 0 and B > 0 and
                    ops.xna_mse_auto(B, heads, enc.out_channels // heads, C // heads, features.shape[-2:], (ho, wo), ksz, out_dtype, regress)):
                return composed()
        elif C % heads:
            raise ValueError(f"feature channels {C} not divisible by {heads} heads")
        with torch.no_grad():
            q5, k5, _ = self.guidance_qk(image, features.shape[-2:], (ho, wo))       # materialised queries: the union kernel takes no rotate-on-load
            h, w = features.shape[-2:]
            # (the objective's kernel takes bf16 values: float16 features are packed to bf16 through fp32, as they always were)
            v5 = ops.pack_values(features.float() if features.dtype == torch.float16 else features).view(B, h, w, heads, C // heads).permute(0, 3, 1, 2, 4)
            with ops._Timed("attention"):
                loss, _ = ops.xna_mse_forward(q5, k5, v5, regress, ksz, scale=self.upsampler.scale, grad=False)
        return loss

    def _forward_cosine(self, image, features, output_size, return_weights, head, target, ignore_index, reduction, predict, confusion,
                        regress, logit_scale, return_norms, path, loss=None):
        """``forward(..., head=E, cosine=True)``: see ``forward``.  Every refusal comes before anything touches the device."""
        if path not in ("auto", "fused", "composed"):
            raise ValueError(f"cosine_path must be 'auto', 'fused' or 'composed', got {path!r}")
        if regress is not None or return_weights:
            raise ValueError("naf(..., cosine=True) returns cosines against the rows of head=E: it does not combine with regress / return_weights")
        if head is None:
            raise ValueError("naf(..., cosine=True) needs the embeddings: pass head=E ([N, C] tensor, or a bias-free nn.Linear / 1x1 nn.Conv2d)")
        if not isinstance(features, torch.Tensor) or features.dim() != 4 or image.dim() != 4 or image.shape[0] != features.shape[0]:
            raise ValueError(f"expected image [B,3,H,W] and features [B,C,h,w], got {tuple(image.shape)} / {tuple(getattr(features, 'shape', ()))}")
        weight = _cosine_head(head, features.shape[1])
        evaluation = confusion is not None and confusion is not False
        if loss is not None:
            return self._forward_cosine_objective(image, features, output_size, weight, target, ignore_index, reduction, predict, evaluation,
                                                  logit_scale, return_norms, path)
        if target is not None and not evaluation:
            raise ValueError("naf(..., cosine=True, target=...) without confusion=: the cross-entropy on the scaled cosines is loss='ce' "
                             "(labels: predict=True; evaluation: confusion=)")
        if not math.isfinite(float(logit_scale)):
            raise ValueError(f"logit_scale must be finite, got {logit_scale}")
        if predict or evaluation:
            if return_norms:
                raise ValueError("naf(..., cosine=True, return_norms=True) goes with the cosines, not with predict / confusion")
            # the argmax over n of logit_scale * cos is that of E^ . f for logit_scale > 0: the existing labels / confusion launches
            if float(logit_scale) <= 0:
                raise ValueError(f"naf(..., cosine=True, predict / confusion) needs logit_scale > 0 (the labels are the argmax), got {logit_scale}")
            with torch.no_grad():
                e_hat = ops.normalize_embeddings(weight)
            return self.forward(image, features, output_size, head=(e_hat, None), target=target, ignore_index=ignore_index, reduction=reduction,
                                predict=predict, confusion=confusion)
        if not (image.is_cuda and features.is_cuda and weight.is_cuda):
            raise _rocm_only(image=image, features=features, head=weight)
        if isinstance(image, Guidance):
            self._check_guidance_call(image, features, False, None, None)
        ho, wo = int(output_size[0]), int(output_size[1])
        B, C, N = features.shape[0], features.shape[1], weight.shape[0]
        if B == 0:
            cos = torch.empty((0, ho, wo, N), dtype=torch.float32, device=features.device).permute(0, 3, 1, 2)
            return (cos, torch.empty((0, ho, wo), dtype=torch.float32, device=features.device)) if return_norms else cos
        heads, ksz, enc = self.upsampler.num_heads, self.upsampler.kernel_size, self.image_encoder
        grad = torch.is_grad_enabled()
        reason = None       # why the fused kernel does not take the call
        if grad and weight.requires_grad:
            reason = "the fused cosine kernel is inference-only and the embeddings require a gradient"
        elif self._wants_grad(image, features):
            reason = "the fused cosine kernel is inference-only and the call wants a gradient for the upsampler or its inputs"
        elif features.dtype != torch.bfloat16:
            reason = f"the fused cosine kernel reads bfloat16 features, got {features.dtype}"
        elif C % heads or enc.out_channels % heads:
            reason = f"feature channels {C} / guidance channels {enc.out_channels} not divisible by {heads} heads"
        else:
            probe = torch.empty((B, ho, wo, heads, enc.out_channels // heads), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
            if ops.xna_cos_select(probe, features.shape[-2:], C // heads, N, ksz) != "fused":
                reason = _lib_last_error() or f"naf_xna_cos_select refuses {N} embeddings"
        if path == "fused" and reason is not None:
            raise ops._lib.NafHipError(f"naf(..., cosine=True, cosine_path='fused'): {reason}")
        if path == "composed" or reason is not None:
            with ops._Timed("cosine_composed"):
                return ops.cosine_from_features(self.forward(image, features, output_size), ops.normalize_embeddings(weight), logit_scale, return_norms)
        with torch.no_grad():
            lr = features.shape[-2:]
            fusable = lambda q5, tabs: ops.xna_cos_select(q5, lr, C // heads, N, ksz, rope_tables=tabs) == "fused"
            q5, k5, tabs = self.guidance_qk(image, lr, (ho, wo), fusable=fusable)
            v5 = ops.pack_values(features).view(B, lr[0], lr[1], heads, C // heads).permute(0, 3, 1, 2, 4)
            with ops._Timed("attention"):
                return ops.xna_cos_forward(q5, k5, v5, weight, ksz, logit_scale=logit_scale, return_norms=return_norms, path="fused",
                                           scale=self.upsampler.scale, rope_tables=tabs)

    def _forward_cosine_objective(self, image, features, output_size, weight, target, ignore_index, reduction, predict, evaluation,
                                  logit_scale, return_norms, path):
        """``forward(..., head=E, cosine=True, target=t, loss="ce")``: see ``forward``.  Every refusal comes before anything touches the device."""
        if target is None:
            raise ValueError("naf(..., cosine=True, loss='ce') needs target=...: integer class indices [B, Ho, Wo]")
        if return_norms:
            raise ValueError("naf(..., cosine=True, loss='ce') returns the loss: return_norms goes with the cosines")
        if evaluation:
            raise ValueError("naf(..., cosine=True, loss='ce') does not combine with confusion= (the evaluation is a call of its own)")
        if reduction not in ops._REDUCTIONS:
            raise ValueError(f"reduction must be one of {ops._REDUCTIONS}, got {reduction!r}")
        learnable = isinstance(logit_scale, torch.Tensor)
        if learnable:
            if logit_scale.numel() != 1 or logit_scale.dtype != torch.float32:
                raise ValueError(f"logit_scale must be a float or a 1-element float32 tensor, got {tuple(logit_scale.shape)} {logit_scale.dtype}")
        else:
            if not math.isfinite(float(logit_scale)):
                raise ValueError(f"logit_scale must be finite, got {logit_scale}")
            if predict and float(logit_scale) <= 0:
                raise ValueError(f"naf(..., cosine=True, loss='ce', predict=True) needs logit_scale > 0 (the labels are the argmax), got {logit_scale}")
        ho, wo = int(output_size[0]), int(output_size[1])
        B, C, N = features.shape[0], features.shape[1], weight.shape[0]
        ignore_index = int(ignore_index)
        target = ops._check_target(target, (B, ho, wo), features.device, "naf(..., loss='ce')")
        if not (image.is_cuda and features.is_cuda and weight.is_cuda and (not learnable or logit_scale.is_cuda)):
            raise _rocm_only(image=image, features=features, head=weight)
        if isinstance(image, Guidance):
            self._check_guidance_call(image, features, False, None, None)
        pack = lambda loss, labels: (loss, labels) if predict else loss
        heads, ksz, enc = self.upsampler.num_heads, self.upsampler.kernel_size, self.image_encoder
        head_grad = torch.is_grad_enabled() and (weight.requires_grad or (learnable and logit_scale.requires_grad))
        reason = None       # why the fused kernel does not take the call
        if B == 0:
            reason = "an empty batch"
        elif self._wants_grad(image, features):
            reason = "the call wants a gradient for the upsampler or its inputs, which the fused route does not carry"
        elif features.dtype != torch.bfloat16:
            reason = f"the fused cosine kernel reads bfloat16 features, got {features.dtype}"
        elif C % heads or enc.out_channels % heads:
            reason = f"feature channels {C} / guidance channels {enc.out_channels} not divisible by {heads} heads"
        else:
            probe = torch.empty((B, ho, wo, heads, enc.out_channels // heads), dtype=torch.bfloat16, device="meta").permute(0, 3, 1, 2, 4)
            if ops.xna_cos_ce_select(probe, features.shape[-2:], C // heads, N, ksz) != "fused":
                reason = _lib_last_error() or f"naf_xna_cos_ce_select refuses {N} embeddings"
        if path == "fused" and reason is not None:
            raise ops._lib.NafHipError(f"naf(..., cosine=True, loss='ce', cosine_path='fused'): {reason}")
        if path == "composed" or reason is not None:
            with ops._Timed("cosine_objective_composed"):
                if B == 0:
                    z = torch.empty((0, N, ho, wo), dtype=torch.float32, device=features.device)
                else:
                    z = ops.cosine_from_features(self.forward(image, features, output_size), ops.normalize_embeddings(weight), 1.0) * logit_scale
                val = F.cross_entropy(z.float(), ops.head_sanitized_target(target, ignore_index, N), ignore_index=ignore_index, reduction=reduction)
                return pack(val, z.detach().argmax(1) if predict else None)
        lr = features.shape[-2:]
        with torch.no_grad():
            # a recorded graph reads materialised (rotated) queries: the backward kernels have no rotate-on-load
            fusable = None if head_grad else (lambda q5, tabs: ops.xna_cos_ce_select(q5, lr, C // heads, N, ksz, rope_tables=tabs) == "fused")
            q5, k5, tabs = self.guidance_qk(image, lr, (ho, wo), fusable=fusable)
            v5 = ops.pack_values(features).view(B, lr[0], lr[1], heads, C // heads).permute(0, 3, 1, 2, 4)
        with ops._Timed("attention"):
            if head_grad:
                pv5 = ops.project_cosine_values(weight, v5)       # with the graph on: the embeddings' gradient enters autograd here
                res = ops.XnaCosCEFunction.apply(q5, k5, pv5, v5, weight, logit_scale, target, ksz, ignore_index, reduction, bool(predict), "fused",
                                                 self.upsampler.scale)
                val, labels = res if predict else (res, None)
            else:
                with torch.no_grad():
                    loss_map, labels, _, _ = ops.xna_cos_objective(q5, k5, v5, weight, ksz, target=target, ignore_index=ignore_index,
                                                                   logit_scale=logit_scale, want_loss=True, want_labels=bool(predict), path="fused",
                                                                   scale=self.upsampler.scale, rope_tables=tabs)
                    val = ops.reduce_head_loss(loss_map, target, ignore_index, N, reduction)
        return pack(val, None if labels is None else labels.long())

    def _head_call(self, image, features, output_size, return_weights, head, reduction="mean", target=None, confusion=None, more=None):
        """Host-side validation the ``head=`` entries share, in the order they raise (nothing has touched the device yet):
        -> (weight, bias, (ho, wo), target as int64).  ``target`` / ``confusion``: checked where the entry has one; the logits entry has no ``reduction``, the default passes.
        ``more(weight, ho, wo)``: an entry's further checks, run before CPU tensors are sent away."""
        if features.dim() != 4 or image.dim() != 4 or image.shape[0] != features.shape[0]:
            raise ValueError(f"expected image [B,3,H,W] and features [B,C,h,w], got {tuple(image.shape)} / {tuple(features.shape)}")
        weight, bias = _linear_head(head, features.shape[1])
        if return_weights:
            raise ValueError("naf(..., head=...) does not return attention scores: call naf(image, features, size, return_weights=True) for them")
        if reduction not in ops._REDUCTIONS:
            raise ValueError(f"reduction must be one of {ops._REDUCTIONS}, got {reduction!r}")
        ho, wo = int(output_size[0]), int(output_size[1])
        if target is not None:
            target = ops._check_target(target, (image.shape[0], ho, wo), features.device, "naf(..., target=...)")
        if confusion is not None and confusion is not True:
            if not isinstance(confusion, torch.Tensor):
                raise TypeError(f"confusion must be True or an int64 [N, N] tensor, got {type(confusion).__name__}")
            ops._check_confusion(confusion, weight.shape[0], features.device, "naf(..., confusion=...)")
        if more is not None:
            more(weight, ho, wo)
        if not (image.is_cuda and features.is_cuda and weight.is_cuda):
            raise _rocm_only(image=image, features=features, head=weight)
        return weight, bias, (ho, wo), target

    def _head_operands(self, image, features, weight, bias, out_size, head_grad, out_dtype=torch.float32):
        """The attention's operands of a ``head=`` call: (q5, k5, rope tables or None, pv5, fp32 bias or None).  ``head_grad``: the call
        records a graph for the head, so the queries are materialised -- rotate-on-load only without a graph: the backward kernels read
        rotated queries.  Otherwise the geometry decides (``out_dtype``: the logits'), not the outputs asked for."""
        heads = self.upsampler.num_heads
        if features.shape[1] % heads:
            raise ValueError(f"feature channels {features.shape[1]} not divisible by {heads} heads")
        ksz, lr, N = self.upsampler.kernel_size, features.shape[-2:], weight.shape[0]
        with torch.no_grad():
            fusable = None if head_grad else (lambda q5, tabs: ops.xna_head_select(q5, lr, N, ksz, out_dtype=out_dtype, rope_tables=tabs) == "fused")
            q5, k5, tabs = self.guidance_qk(image, lr, out_size, fusable=fusable)
        return (q5, k5, tabs) + ops.project_head_values(weight, bias, features, heads)

    def _forward_head(self, image, features, output_size, return_weights, head):
        """``forward(..., head=head)``: see ``forward``."""
        weight, bias, (ho, wo), _ = self._head_call(image, features, output_size, return_weights, head)
        N = weight.shape[0]
        if image.shape[0] == 0:
            return torch.empty((0, ho, wo, N), dtype=weight.dtype, device=features.device).permute(0, 3, 1, 2)
        grad = torch.is_grad_enabled()
        if self._wants_grad(image, features):
            # a gradient for the upsampler or its inputs: today's differentiable forward, then the head (unfused)
            return _apply_head(head, self.forward_train(image, features, output_size, amp="auto"))
        head_grad = grad and (weight.requires_grad or (bias is not None and bias.requires_grad))
        q5, k5, tabs, pv5, b32 = self._head_operands(image, features, weight, bias, (ho, wo), head_grad, weight.dtype)
        ksz = self.upsampler.kernel_size
        with ops._Timed("attention"):
            if head_grad:
                return ops.XnaHeadFunction.apply(q5, k5, pv5, b32, ksz, N, weight.dtype, "auto", self.upsampler.scale)
            with torch.no_grad():
                return ops.xna_head_forward(q5, k5, pv5, b32, ksz, n_out=N, out_dtype=weight.dtype, scale=self.upsampler.scale, rope_tables=tabs)

    def _forward_head_objective(self, image, features, output_size, return_weights, head, target, ignore_index, reduction, predict):
        """``forward(..., head=head, target=... / predict=True)``: see ``forward``."""
        weight, bias, (ho, wo), target = self._head_call(image, features, output_size, return_weights, head, reduction, target)
        B, N = image.shape[0], weight.shape[0]
        ignore_index = int(ignore_index)
        pack = lambda loss, labels: (loss, labels) if (target is not None and predict) else (loss if target is not None else labels)
        grad = torch.is_grad_enabled()
        if B == 0 or self._wants_grad(image, features):
            # an empty batch (what torch returns for empty inputs of these shapes), or a gradient for the upsampler or its inputs: the
            # logits call (unfused there), then the objective as torch ops
            logits = self._forward_head(image, features, output_size, False, head).float()
            loss = None
            if target is not None:      # torch's own cross-entropy, with this call's contract for targets outside the classes
                loss = F.cross_entropy(logits, ops.head_sanitized_target(target, ignore_index, N), ignore_index=ignore_index, reduction=reduction)
            return pack(loss, logits.detach().argmax(1) if predict else None)
        head_grad = grad and target is not None and (weight.requires_grad or (bias is not None and bias.requires_grad))
        q5, k5, tabs, pv5, b32 = self._head_operands(image, features, weight, bias, (ho, wo), head_grad)
        ksz = self.upsampler.kernel_size
        with ops._Timed("attention"):
            if head_grad:
                res = ops.XnaHeadCEFunction.apply(q5, k5, pv5, b32, target, ksz, N, ignore_index, reduction, predict, "auto", self.upsampler.scale)
                loss, labels = res if predict else (res, None)
            else:
                with torch.no_grad():
                    loss_map, labels, _, _ = ops.xna_head_objective(q5, k5, pv5, b32, ksz, n_out=N, target=target, ignore_index=ignore_index,
                                                                    want_loss=target is not None, want_labels=predict,
                                                                    scale=self.upsampler.scale, rope_tables=tabs)
                    loss = None if target is None else ops.reduce_head_loss(loss_map, target, ignore_index, N, reduction)
        return pack(loss, None if labels is None else labels.long())       # the kernel writes uint8; widened so that it drops into pred == target

    def _forward_head_confusion(self, image, features, output_size, return_weights, head, target, ignore_index, reduction, predict, confusion):
        """``forward(..., head=head, target=..., confusion=True / matrix)``: see ``forward``."""
        weight, bias, (ho, wo), target = self._head_call(image, features, output_size, return_weights, head, reduction, target, confusion)
        N = weight.shape[0]
        if features.shape[1] % self.upsampler.num_heads:      # this entry refuses it for an empty batch too
            raise ValueError(f"feature channels {features.shape[1]} not divisible by {self.upsampler.num_heads} heads")
        with torch.no_grad():
            cm = torch.zeros((N, N), dtype=torch.int64, device=features.device) if confusion is True else confusion
            if image.shape[0] == 0:
                return (cm, torch.empty((0, ho, wo), dtype=torch.int64, device=features.device)) if predict else cm
            q5, k5, tabs, pv5, b32 = self._head_operands(image, features, weight, bias, (ho, wo), False)
            with ops._Timed("attention"):
                _, labels, _, _ = ops.xna_head_objective(q5, k5, pv5, b32, self.upsampler.kernel_size, n_out=N, target=target, ignore_index=int(ignore_index),
                                                         want_labels=predict, scale=self.upsampler.scale, rope_tables=tabs, confusion=cm)
            return (cm, labels.long()) if predict else cm

    def _forward_head_regression(self, image, features, output_size, head, dense_target, kind, beta, valid, errors, clamp, reduction, predict):
        """``forward(..., head=head, dense_target=t)``: see ``forward``.  Every refusal comes before anything touches the device."""
        who = "naf(..., dense_target=...)"
        evaluation = errors is not None and errors is not False

        def more(weight, ho, wo):
            B, N, dev = image.shape[0], weight.shape[0], features.device
            ops._check_reg_kind(who, kind, beta)
            ops._check_dense_target(who, dense_target, (B, N, ho, wo), dev)
            if valid is not None:
                ops._check_valid_mask(who, valid, (B, ho, wo), dev)
            ops._check_clamp(who, clamp)
            if evaluation:
                if N != 1:
                    raise ValueError(f"naf(..., errors=...): the error statistics are defined for a head with one output, this one has {N}")
                if errors is not True:
                    ops._check_errors("naf(..., errors=...)", errors, dev)

        weight, bias, (ho, wo), _ = self._head_call(image, features, output_size, False, head, reduction, more=more)
        if isinstance(image, Guidance):
            self._check_guidance_call(image, features, False, None, True if evaluation else None)
        B, N = image.shape[0], weight.shape[0]
        if features.shape[1] % self.upsampler.num_heads:
            raise ValueError(f"feature channels {features.shape[1]} not divisible by {self.upsampler.num_heads} heads")
        beta = float(beta)
        if evaluation:
            with torch.no_grad():
                acc = torch.zeros(ops._lib.HEAD_REG_STATS, dtype=torch.float64, device=features.device) if errors is True else errors
                if B == 0:
                    return (acc, torch.empty((0, N, ho, wo), dtype=torch.float32, device=features.device)) if predict else acc
                q5, k5, tabs, pv5, b32 = self._head_operands(image, features, weight, bias, (ho, wo), False)
                with ops._Timed("attention"):
                    _, _, pred = ops.xna_head_regression(q5, k5, pv5, b32, self.upsampler.kernel_size, n_out=N, target=dense_target, valid=valid,
                                                         return_logits=predict, errors=acc, clamp=clamp, scale=self.upsampler.scale, rope_tables=tabs)
                return (acc, pred) if predict else acc
        grad = torch.is_grad_enabled()
        if B == 0 or self._wants_grad(image, features):
            # an empty batch, or a gradient for the upsampler or its inputs: the logits call (unfused there), then the objective as torch ops
            logits = self._forward_head(image, features, output_size, False, head).float()
            loss_map, _ = ops.head_regression_from_logits(logits, dense_target, valid, kind, beta, want_loss=True)
            val = ops.reduce_regression_loss(loss_map, valid, N, reduction)
            return (val, logits.detach()) if predict else val
        head_grad = grad and (weight.requires_grad or (bias is not None and bias.requires_grad))
        q5, k5, tabs, pv5, b32 = self._head_operands(image, features, weight, bias, (ho, wo), head_grad)
        ksz = self.upsampler.kernel_size
        with ops._Timed("attention"):
            if head_grad:
                res = ops.XnaHeadRegFunction.apply(q5, k5, pv5, b32, dense_target, valid, ksz, N, kind, beta, reduction, predict, "auto",
                                                   self.upsampler.scale)
                return res
            with torch.no_grad():
                loss_map, _, pred = ops.xna_head_regression(q5, k5, pv5, b32, ksz, n_out=N, target=dense_target, valid=valid, kind=kind, beta=beta,
                                                            want_loss=True, return_logits=predict, scale=self.upsampler.scale, rope_tables=tabs)
                val = ops.reduce_regression_loss(loss_map, valid, N, reduction)
        return (val, pred) if predict else val

    def _forward_inference(self, image, features, output_size, return_weights=False):
        if not (image.is_cuda and features.is_cuda):
            raise _rocm_only(image=image, features=features)
        if image.dim() != 4 or features.dim() != 4 or image.shape[0] != features.shape[0]:
            raise ValueError(f"expected image [B,3,H,W] and features [B,C,h,w], got {tuple(image.shape)} / {tuple(features.shape)}")
        if image.shape[0] == 0:
            # an empty batch flows through the reference's torch ops as empty tensors; there is nothing to launch here
            ho, wo = int(output_size[0]), int(output_size[1])
            odt = features.dtype if features.dtype in (torch.bfloat16, torch.float16, torch.float32) else torch.float32
            out = torch.empty((0, ho, wo, features.shape[1]), dtype=odt, device=features.device).permute(0, 3, 1, 2)
            if out.dtype != features.dtype:
                out = out.to(features.dtype)
            if return_weights:
                k = self.upsampler.kernel_size
                return out, torch.empty((0, self.upsampler.num_heads, ho, wo, k[0] * k[1]), dtype=torch.float32, device=features.device)
            return out
        if self.single_call and not isinstance(image, Guidance):       # (the one-call plan runs the whole forward: nothing of it is reusable)
            plan = self._forward_plan(image, features, output_size)
            if plan is not None:
                timer = ops.KERNEL_TIMER
                ev = pe = None
                if timer is not None and getattr(timer, "enabled", False):
                    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    for e in ev:
                        e.record()          # creates the underlying hipEvent_t; naf_forward re-records it around the kernel
                    timer.pairs.setdefault("xna_mfma", []).append(ev)
                    every = int(getattr(timer, "phases", 1) or 0)       # 0 / False: none; n: every n-th call (an event record
                    timer._calls = getattr(timer, "_calls", -1) + 1       # between two kernels costs ~5 us of device time)
                    if every > 0 and timer._calls % every == 0:
                        # the phases of the ONE call (naf_forward_args.phase_events, version >= 105: the branches' layers alternate):
                        # the whole stem, both first convolutions, ONE launch of each block-layer kernel (stage 1), the RoPE /
                        # key-pooling pre-pass, the attention
                        pe = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
                        for e in pe:
                            e.record()
                        # under the A/B knob NAF_STEM_ORDER=0 (one branch after the other) the library never records [7] and [1] / [2] / [3]
                        # mean other things (include/naf_hip.h): only the boundaries both orders share are registered then
                        knobs = os.environ.get("NAF_HIP_KNOBS") == "1"
                        sequential = knobs and os.environ.get("NAF_STEM_ORDER") == "0"
                        one_stream = plan.planned_streams() == 1     # the library's plan for these shapes (naf_forward_streams)
                        pairs = (("stem", 0, 4), ("rope_pool", 4, 5), ("attention", 5, 6))
                        if sequential:
                            pass
                        elif one_stream:      # round 3: the branches' layers alternate on one stream
                            pairs += (("stem_first_convs", 0, 1), ("stem_layer_1x1", 2, 3), ("stem_layer_3x3", 3, 7))
                        else:                 # two streams (the host lends the second: ops.forward_aux); [2] .. [7] bracket one 3x3 launch (the 1x1 launches run beside it)
                            pairs += (("stem_first_convs", 0, 1), ("stem_layer_3x3", 2, 7))
                        for name, i, j in pairs:
                            timer.pairs.setdefault(name, []).append((pe[i], pe[j]))
                return plan.run(image, features, ev, return_logits=bool(return_weights), phase_events=pe)
        fuse_for = None
        if features.shape[1] % self.upsampler.num_heads == 0:
            fuse_for = (features.shape[1] // self.upsampler.num_heads,
                        features.dtype if features.dtype in (torch.bfloat16, torch.float16) else torch.float32)
        q5, k5, tabs = self.guidance_qk(image, features.shape[-2:], output_size, fuse_for=fuse_for)
        with ops._Timed("attention"):
            return self.upsampler(q5, k5, features, return_weights=return_weights, path=self.xna_path, rope_tables=tabs)

"""Stable Diffusion 2.1 UNet (diffusers ``UNet2DConditionModel`` architecture), NHWC.

Reference workload: ``StableDiffusionPipeline`` UNet that app/run-sd.py:104-135
runs (cuDNN/Inductor on GPU, NEFF on Inferentia).  MI355X-first design:

* Every 3x3/1x1 conv is the implicit-GEMM MFMA kernel; the time-embedding bias
  and the residual/skip add are fused into the conv epilogue, Upsample2D's
  nearest-2x is fused into the gather.  A ResNet's GroupNorm+SiLU takes its
  statistics from the producer's epilogue partials; one vectorised apply pass
  writes the normalised input and the tuned conv reads it (the default).  The
  halo-tiled conv (csrc/kernels/conv_halo.hip, ``ops.set_halo_conv``) applies
  the norm once per staged element in LDS instead; it is opt-in, measured
  slower at the SD2.1 shapes.
* Transformer blocks: fused QKV GEMM -> flash attention reading strided views
  -> out-proj GEMM with the residual in its epilogue; GEGLU fused into the FF
  GEMM epilogue.
* Cross-attention K/V depend only on the text context: computed once per
  request (:meth:`UNet2DConditionModel.context_kv`) and reused for all steps.
* All 22 ResNet time-embedding projections run as ONE batched GEMM per step.
* Classifier-free guidance (``forward(..., cfg_pairs=True)``): rows i and B + i
  of the batch enter identical and stay so until the first cross-attention, so
  the first ResNet and the first transformer up to its cross-attention Q run on
  B rows; the kernels that join them with the 2B contexts read the B-row
  operand in place (``q_batch_mod`` / ``residual_rows``).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from .. import ops
from .attention import CrossAttention, FusedSelfAttention, merge_linear_keys
from .layers import Conv2d, GLULinear, GroupNorm, LayerNorm, Linear, _wkey, timestep_embedding

# the last transformer block's FF down projection merged into proj_out (Transformer2DModel._merged_out)
MERGE_PROJ_OUT = os.environ.get("SHAI_MERGE_PROJ_OUT", "1") != "0"
# the Transformer2D input GroupNorm folded into proj_in's weight per image (Transformer2DModel._proj_in_gn_folded)
GN_FOLD_PROJ_IN = os.environ.get("SHAI_GN_FOLD_PROJ_IN", "1") != "0"

# GroupNorm partials / LayerNorm moments handed from the producing GEMM epilogue to the next norm (and LayerNorms
# folded into their consumer projections); SHAI_NORM_HANDOFF=0 restores the standalone norm passes (A/B)
NORM_HANDOFF = os.environ.get("SHAI_NORM_HANDOFF", "1") != "0"
# ResNet GroupNorm + SiLU applied by the consuming 3x3 conv (ops.conv2d(norm=...): the halo-tiled conv normalises each
# staged input element once in LDS); SHAI_FUSED_GN_CONV=0 restores the separate apply pass (A/B)
FUSED_GN_CONV = os.environ.get("SHAI_FUSED_GN_CONV", "1") != "0"
# cfg_pairs forwards run the layers both guidance halves share once (UNet2DConditionModel.forward);
# SHAI_CFG_SHARED=0 restores the full-batch path (A/B)
CFG_SHARED = os.environ.get("SHAI_CFG_SHARED", "1") != "0"
# fewest activation rows per guidance half (B H W at the first level) at which the prefix is shared.  One 512^2 image
# (4096 rows) stays unshared: halving its already small, split-K-bound kernels measured no gain (batch-1 p50 350.7 /
# 351.3 ms shared against 350.7 / 350.6 ms unshared, profiles/cfg_shared_prefix.md); batch 32 gains 2.7 %.  The gate
# rests on those two points alone: batches 2 to 16 were not measured
CFG_SHARED_MIN_ROWS = int(os.environ.get("SHAI_CFG_SHARED_MIN_ROWS", "8192"))


@dataclass
class UNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    layers_per_block: int = 2
    attention_heads: Tuple[int, ...] = (5, 10, 20, 20)  # diffusers "attention_head_dim" for SD2 = head counts
    cross_attention_dim: int = 1024
    down_attn: Tuple[bool, ...] = (True, True, True, False)
    norm_num_groups: int = 32
    norm_eps: float = 1e-5
    time_embed_dim: int = 1280
    flip_sin_to_cos: bool = True
    freq_shift: float = 0.0

    @staticmethod
    def sd21():
        return UNetConfig()

    @staticmethod
    def tiny():
        return UNetConfig(block_out_channels=(64, 128), layers_per_block=1, attention_heads=(1, 2),
                          cross_attention_dim=64, down_attn=(True, False), time_embed_dim=128)


class ResnetBlock2D(nn.Module):
    def __init__(self, cin: int, cout: int, temb: Optional[int], groups: int, eps: float):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.norm1 = GroupNorm(groups, cin, eps)
        self.conv1 = Conv2d(cin, cout, 3, padding=1)
        self.time_emb_proj = Linear(temb, cout) if temb else None
        self.norm2 = GroupNorm(groups, cout, eps)
        self.conv2 = Conv2d(cout, cout, 3, padding=1)
        self.conv_shortcut = Conv2d(cin, cout, 1) if cin != cout else None

    def forward(self, x, temb_proj=None, x2=None):
        """``x2``: up-block skip tensor -- the block's input is cat([x, x2], -1), read from the two
        sources by GroupNorm and by the 1x1 shortcut conv (fused concat), never materialised."""
        return self.forward_parts(x, temb_proj, x2)[0]

    def forward_parts(self, x, temb_proj=None, x2=None, xp=None, x2p=None, stats: bool = False):
        """forward with the GroupNorm hand-off: ``xp`` / ``x2p`` are GroupNorm partials of x / x2 written by their
        producers' epilogues (they replace the statistics pass of norm1); with ``stats`` conv1 and conv2 write
        the partials of their outputs (norm2's input, and the next norm's).  Returns (out, partials or None)."""
        st = {"stats": "gn"} if stats else {}
        if FUSED_GN_CONV and x.shape[-1] % 8 == 0 and (x2 is None or x2.shape[-1] % 8 == 0):
            # GroupNorm + SiLU as the convs' prologue: (scale, shift) from the producers' partials, applied once per
            # staged element inside the halo-tiled conv (one apply pass + the tuned conv where it does not fit)
            sc, sh = self.norm1.scale_shift(x, x2, part=xp, part2=x2p)
            out1 = self.conv1(x, x2=x2, norm=(sc, sh, "silu"), temb=temb_proj, **st)
        else:
            # the separate pass: GroupNorm + SiLU written out, then the conv
            n1 = self.norm1(x, silu=True, x2=x2, part=xp, part2=x2p)
            out1 = self.conv1(n1, temb=temb_proj, **st)
        h, hp = out1 if stats else (out1, None)
        if self.conv_shortcut is not None:
            skip = self.conv_shortcut(x, x2=x2) if x2 is not None else self.conv_shortcut(x)
        else:
            skip = x if x2 is None else torch.cat([x, x2], dim=-1)
        if FUSED_GN_CONV and h.shape[-1] % 8 == 0:
            sc, sh = self.norm2.scale_shift(h, part=hp)
            out = self.conv2(h, norm=(sc, sh, "silu"), residual=skip, **st)
        else:
            out = self.conv2(self.norm2(h, silu=True, part=hp), residual=skip, **st)
        return out if stats else (out, None)


class GEGLU(nn.Module):
    def __init__(self, dim: int, inner: int):
        super().__init__()
        self.proj = GLULinear(dim, inner, act="gelu")


class FeedForward(nn.Module):
    def __init__(self, dim: int, mult: int = 4):
        super().__init__()
        inner = dim * mult
        self.net = nn.ModuleList([GEGLU(dim, inner), nn.Identity(), Linear(inner, dim)])

    def forward(self, x, residual):
        return self.net[2](self.net[0].proj(x), residual=residual)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim: int, heads: int, ctx_dim: int):
        super().__init__()
        self.norm1 = LayerNorm(dim)
        self.attn1 = FusedSelfAttention(dim, heads, qkv_bias=False)
        self.norm2 = LayerNorm(dim)
        self.attn2 = CrossAttention(dim, ctx_dim, heads)
        self.norm3 = LayerNorm(dim)
        self.ff = FeedForward(dim)

    def forward(self, x, ctx_kv, shared: bool = False):
        """``shared``: x holds B images under 2B contexts (``CrossAttention.forward``); the output has 2B images."""
        x = self.attn1(self.norm1(x), residual=x)
        x = self.attn2(self.norm2(x), ctx_kv, residual=x, shared=shared)
        return self.ff(self.norm3(x), residual=x)

    def forward_folded(self, x, ctx_kv, mr, next_eps=None, defer_down: bool = False, shared: bool = False):
        """forward with every LayerNorm folded into the projection that consumes it: ``mr`` = (mean, rstd) [rows, 2]
        of x from its producer; each residual GEMM (attention out-projections, FF down) hands the next norm's
        (mean, rstd) over from its epilogue, so no normalised activation is ever written.  ``next_eps``: the
        following block's norm1 eps (its statistics are returned), None for the last block.  ``defer_down``: return
        (GEGLU output, residual stream) instead of applying the FF down projection (the caller merges it into
        ``proj_out``).  ``shared``: x holds B images under a context of 2B entries -- everything up to the
        cross-attention Q projection runs on B rows; the cross-attention reads Q, and its out-projection the residual
        stream, of image b % B (``q_batch_mod`` / ``residual_rows``), and the rest runs on 2B rows."""
        B, T, C = x.shape
        a1 = self.attn1
        w, b, s = a1.qkv.folded(self.norm1)
        q, k, v = a1.split(ops.linear(x, w, b, row_affine=(mr, s)))
        o = ops.attention(q, k, v)
        a2 = self.attn2
        H, hd = a2.heads, a2.head_dim
        # 320-wide level: the out-projections compute the next LayerNorm in their epilogue (whole rows in one
        # workgroup of the W-stationary kernel), so Q and the GEGLU run plain on the normalised rows; wider levels
        # hand (mean, rstd) over and fold the norm into the consumer
        lnout = x.is_cuda and ops.lnout_supported(B * T, C, a1.heads * a1.head_dim)
        if lnout:
            n2, n3 = self.norm2, self.norm3
            x, xn = ops.linear_lnout(o.view(B, T, a1.heads * a1.head_dim), a1.out.weight, a1.out.bias, x, n2.weight,
                                     n2.bias, n2.eps)
            q = a2.q(xn).view(B, T, H, hd)
        else:
            x, mr = a1.out.forward_stats(o.view(B, T, a1.heads * a1.head_dim), residual=x, stats="ln",
                                         eps=self.norm2.eps)
            w, b, s = a2.q.folded(self.norm2)
            q = ops.linear(x, w, b, row_affine=(mr, s)).view(B, T, H, hd)
        S = ctx_kv.shape[1]
        o = ops.attention(q, ctx_kv[..., : H * hd].view(ctx_kv.shape[0], S, H, hd),
                          ctx_kv[..., H * hd:].view(ctx_kv.shape[0], S, H, hd), q_batch_mod=B if shared else 0)
        rr = B * T if shared else 0  # the residual stream still holds B images
        B = o.shape[0]
        proj = self.ff.net[0].proj
        if lnout:
            x, xn = ops.linear_lnout(o.view(B, T, H * hd), a2.out.weight, a2.out.bias, x, self.norm3.weight,
                                     self.norm3.bias, self.norm3.eps, residual_rows=rr)
            h = ops.linear(xn, proj.weight, proj.bias, act=proj.act, glu=True)
        else:
            x, mr = a2.out.forward_stats(o.view(B, T, H * hd), residual=x, stats="ln", eps=self.norm3.eps,
                                         residual_rows=rr)
            w, b, s = proj.folded(self.norm3)
            h = ops.linear(x, w, b, act=proj.act, glu=True, row_affine=(mr, s))
        if defer_down:
            return h, x
        down = self.ff.net[2]
        if next_eps is None:
            return down(h, residual=x), None
        return down.forward_stats(h, residual=x, stats="ln", eps=next_eps)


class Transformer2DModel(nn.Module):
    def __init__(self, channels: int, heads: int, ctx_dim: int, groups: int):
        super().__init__()
        self.norm = GroupNorm(groups, channels, 1e-6)
        self.proj_in = Conv2d(channels, channels, 1)   # Linear projection as a 1x1 conv (norm fused in gather)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(channels, heads, ctx_dim)])
        self.proj_out = Linear(channels, channels)

    def forward(self, x, ctx_kv, shared: bool = False):
        """``shared``: x holds B images under a context of 2B entries; the first block joins them (its output, and
        this one, have 2B images) and ``proj_out`` adds x of image b % B."""
        B, H, W, C = x.shape
        h = self.proj_in(self.norm(x)).view(B, H * W, C)
        for i, blk in enumerate(self.transformer_blocks):
            h = blk(h, ctx_kv, shared=shared and i == 0)
        return self.proj_out(h, residual=x.view(B, H * W, C),
                             residual_rows=B * H * W if shared else 0).view(h.shape[0], H, W, C)

    def forward_parts(self, x, ctx_kv, xp=None, stats: bool = False, shared: bool = False):
        """forward with the norm hand-offs: GroupNorm partials ``xp`` of x in, LayerNorms folded into the block
        projections (``BasicTransformerBlock.forward_folded``), and with ``stats`` the GroupNorm partials of the
        output out.  Returns (out, partials or None).  ``shared`` as ``forward``."""
        B, H, W, C = x.shape
        rr = B * H * W if shared else 0  # x, the residual of the output projection, still holds B images
        blocks = list(self.transformer_blocks)
        if ops.fold_profitable(B * H * W, C):  # the Q projection (N = C) has the fewest tiles of the consumers
            if self._gn_fold_ok(x):
                h, mr = self._proj_in_gn_folded(x, xp, blocks[0].norm1.eps)
            else:
                h, mr = self.proj_in(self.norm(x, part=xp), stats="ln", eps=blocks[0].norm1.eps)
            h = h.view(B, H * W, C)
            if mr is None:
                mr = ops.row_moments(h, blocks[0].norm1.eps)
            merged = self._merged_out(x.is_cuda)
            for i, blk in enumerate(blocks):
                if i + 1 == len(blocks) and merged is not None:
                    ffh, hx = blk.forward_folded(h, ctx_kv, mr, None, defer_down=True, shared=shared and i == 0)
                    return self._out_merged(ffh, hx, x, merged, stats, rr)
                h, mr = blk.forward_folded(h, ctx_kv, mr, blocks[i + 1].norm1.eps if i + 1 < len(blocks) else None,
                                           shared=shared and i == 0)
        else:
            h = self.proj_in(self.norm(x, part=xp)).view(B, H * W, C)
            for i, blk in enumerate(blocks):
                h = blk(h, ctx_kv, shared=shared and i == 0)
        res = x.view(B, H * W, C)
        B = h.shape[0]
        if stats and ops.stats_supported(B * H * W, C, "gn", H * W):
            out, op = self.proj_out.forward_stats(h, residual=res, stats="gn", residual_rows=rr)
            return out.view(B, H, W, C), op
        return self.proj_out(h, residual=res, residual_rows=rr).view(B, H, W, C), None

    def _gn_fold_ok(self, x) -> bool:
        B, H, W, C = x.shape
        # per-image weights (B C^2) well below the activation the apply pass moves (B H W C); 256-row slices
        return (GN_FOLD_PROJ_IN and (H * W) % 256 == 0 and 2 * C <= H * W and self.proj_in.k == 1
                and self.proj_in.cin_p == C)

    def _proj_in_gn_folded(self, x, xp, eps):
        """proj_in(GroupNorm(x)) without the normalised activation: GroupNorm is x s[n, c] + t[n, c] per image n,
        so proj_in = x (W diag(s_n))^T + (t_n W^T + b): per-image weights (fp32 product, bf16) and a per-image bias,
        ONE GEMM whose 256-row tiles pick their image's weight (``ops.linear_wslices``) -- the GroupNorm apply pass
        (a read and a write of x) goes.  Returns (h [B H W, C], LayerNorm (mean, rstd) of h)."""
        B, H, W, C = x.shape
        sc, sh = self.norm.scale_shift(x, part=xp)
        w, b = self.proj_in.weight, self.proj_in.bias
        ws = (w.float()[None] * sc[:, None, :]).to(w.dtype)
        b2 = ops.linear(sh.to(w.dtype), w, b)  # t_n W^T + b on the GEMM kernels
        return ops.linear_wslices(x.view(B * H * W, C), ws, b2, H * W, stats="ln", eps=eps)

    def _merged_out(self, cuda: bool = True):
        """The last block's FF down projection merged into ``proj_out`` (both linear, adjacent: out = x + b_po +
        (h + b_fo + f W_fo^T) W_po^T = x + b' + [f | h] [W_po W_fo | W_po]^T): ONE GEMM over the GEGLU output f and the
        residual stream h, run as a 1x1 conv over the two sources -- the FF output h + ... is never written or
        re-read.  Weights product and bias in fp32, cached until a weight changes; None when disabled
        (SHAI_MERGE_PROJ_OUT=0) or first needed inside a graph capture."""
        if not MERGE_PROJ_OUT:
            return None
        down, po = self.transformer_blocks[-1].ff.net[2], self.proj_out
        if down.in_features % 64 or po.in_features % 64:
            return None
        key = tuple(_wkey(t) for t in (down.weight, down.bias, po.weight, po.bias))
        cached = getattr(self, "_po_merged", None)
        if cached is None or cached[0] != key:
            if cuda and torch.cuda.is_current_stream_capturing():
                return None
            wpo = po.weight.float()
            w = torch.cat([wpo @ down.weight.float(), wpo], 1).to(po.weight.dtype).contiguous()
            b = po.bias.float() if po.bias is not None else torch.zeros(po.out_features, device=wpo.device)
            if down.bias is not None:
                b = b + wpo @ down.bias.float()
            cached = (key, (w, b.to(po.weight.dtype)))
            self._po_merged = cached
        return cached[1]

    def _out_merged(self, ffh, hx, x, merged, stats, residual_rows: int = 0):
        _, H, W, C = x.shape
        B = hx.shape[0]  # more images than x in the shared mode (residual_rows: x is read per image b % its count)
        w, b = merged
        f = ffh.reshape(B, H, W, ffh.shape[-1])
        kw = {"stats": "gn"} if stats and ops.stats_supported(B * H * W, C, "gn", H * W) else {}
        r = ops.conv2d(f, w, b, 1, 1, x2=hx.reshape(B, H, W, C), residual=x, residual_rows=residual_rows, **kw)
        return r if kw else (r, None)


class Downsample2D(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = Conv2d(ch, ch, 3, stride=2, padding=1)

    def forward(self, x):
        return self.conv(x)

    def forward_parts(self, x, stats: bool = False):
        return self.conv(x, stats="gn") if stats else (self.conv(x), None)


class Upsample2D(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = Conv2d(ch, ch, 3, padding=1)

    def forward(self, x):
        return self.conv(x, upsample=True)

    def forward_parts(self, x, stats: bool = False):
        return self.conv(x, upsample=True, stats="gn") if stats else (self.conv(x, upsample=True), None)


class DownBlock(nn.Module):
    def __init__(self, cin, cout, n, temb, heads, ctx, attn, groups, eps, down):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if i == 0 else cout, cout, temb, groups, eps) for i in range(n)])
        self.attentions = nn.ModuleList([Transformer2DModel(cout, heads, ctx, groups) for _ in range(n)]) if attn else None
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if down else None


class UpBlock(nn.Module):
    def __init__(self, prev, cout, skip_chs, temb, heads, ctx, attn, groups, eps, up):
        super().__init__()
        res = []
        c = prev
        for sc in skip_chs:
            res.append(ResnetBlock2D(c + sc, cout, temb, groups, eps))
            c = cout
        self.resnets = nn.ModuleList(res)
        self.attentions = nn.ModuleList([Transformer2DModel(cout, heads, ctx, groups) for _ in skip_chs]) if attn else None
        self.upsamplers = nn.ModuleList([Upsample2D(cout)]) if up else None


class MidBlock(nn.Module):
    def __init__(self, ch, temb, heads, ctx, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(ch, ch, temb, groups, eps), ResnetBlock2D(ch, ch, temb, groups, eps)])
        self.attentions = nn.ModuleList([Transformer2DModel(ch, heads, ctx, groups)])


class TimestepEmbedding(nn.Module):
    def __init__(self, cin, dim):
        super().__init__()
        self.linear_1 = Linear(cin, dim)
        self.linear_2 = Linear(dim, dim)

    def forward(self, x):
        return self.linear_2(self.linear_1(x, act="silu"))


class UNet2DConditionModel(nn.Module):
    def __init__(self, cfg: UNetConfig = None):
        super().__init__()
        cfg = cfg or UNetConfig()
        self.cfg = cfg
        chs = cfg.block_out_channels
        g, eps, temb, ctx = cfg.norm_num_groups, cfg.norm_eps, cfg.time_embed_dim, cfg.cross_attention_dim
        self.conv_in = Conv2d(cfg.in_channels, chs[0], 3, padding=1)
        self.time_embedding = TimestepEmbedding(chs[0], temb)
        self.down_blocks = nn.ModuleList()
        c = chs[0]
        skips = [c]
        for i, co in enumerate(chs):
            last = i == len(chs) - 1
            blk = DownBlock(c, co, cfg.layers_per_block, temb, cfg.attention_heads[i], ctx, cfg.down_attn[i], g, eps,
                            not last)
            self.down_blocks.append(blk)
            skips += [co] * cfg.layers_per_block
            if not last:
                skips.append(co)
            c = co
        self.mid_block = MidBlock(chs[-1], temb, cfg.attention_heads[-1], ctx, g, eps)
        self.up_blocks = nn.ModuleList()
        rev = list(reversed(chs))
        rev_heads = list(reversed(cfg.attention_heads))
        rev_attn = list(reversed(cfg.down_attn))
        prev = chs[-1]
        for i, co in enumerate(rev):
            n = cfg.layers_per_block + 1
            skip_chs = [skips.pop() for _ in range(n)]
            blk = UpBlock(prev, co, skip_chs, temb, rev_heads[i], ctx, rev_attn[i], g, eps, i < len(rev) - 1)
            self.up_blocks.append(blk)
            prev = co
        self.conv_norm_out = GroupNorm(g, chs[0], eps)
        self.conv_out = Conv2d(chs[0], cfg.out_channels, 3, padding=1)
        self._temb_bank = None

    # ------------------------------------------------------------------ helpers
    def _resnets(self) -> List[ResnetBlock2D]:
        return [m for m in self.modules() if isinstance(m, ResnetBlock2D)]

    def _attn_modules(self) -> List[Transformer2DModel]:
        return [m for m in self.modules() if isinstance(m, Transformer2DModel)]

    def build_temb_bank(self):
        """Concatenate all ResNet time_emb_proj weights -> one GEMM per step."""
        rs = self._resnets()
        w = torch.cat([r.time_emb_proj.weight for r in rs], 0).contiguous()
        b = torch.cat([r.time_emb_proj.bias for r in rs], 0).contiguous()
        offs, o = [], 0
        for r in rs:
            offs.append((o, r.cout))
            o += r.cout
        self._temb_bank = (w, b, offs)

    def context_kv(self, ctx: torch.Tensor) -> List[torch.Tensor]:
        """Cross-attention K/V for every Transformer block (request-constant)."""
        out = []
        for t in self._attn_modules():
            for blk in t.transformer_blocks:
                out.append(blk.attn2.context_kv(ctx))
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, sample: torch.Tensor, timestep: torch.Tensor, ctx_kv: List[torch.Tensor],
                cfg_pairs: bool = False) -> torch.Tensor:
        """sample [B, H, W, 4] NHWC, timestep [B] (float), ctx_kv from :meth:`context_kv`.

        ``cfg_pairs``: the caller asserts that rows i and B / 2 + i of ``sample`` and of ``timestep`` are equal (the
        two guidance halves of ``cat([lat, lat])``; only the contexts differ).  They stay equal until the first
        cross-attention, so the first ResNet of the first down block and its transformer up to the cross-attention Q
        projection run on the first half only (``CFG_SHARED``).  ``conv_in`` still runs on every row: its output is a
        skip tensor the last up block reads per image."""
        cfg = self.cfg
        B = sample.shape[0]
        t = timestep.expand(B) if timestep.numel() == 1 else timestep
        tf = timestep_embedding(t, cfg.block_out_channels[0], cfg.flip_sin_to_cos, cfg.freq_shift)
        emb = self.time_embedding(tf.to(sample.dtype))
        if self._temb_bank is None:
            self.build_temb_bank()
        w, b, offs = self._temb_bank
        # silu(emb) then one GEMM for all ResNets
        semb = ops.bias_act(emb, None, None, "silu")
        tall = ops.linear(semb, w, b)
        tprojs = [tall[:, o:o + n] for (o, n) in offs]  # column views: each conv reads its columns of tall in place
        ti = iter(tprojs)
        kvi = iter(ctx_kv)

        # Norm hand-offs (NORM_HANDOFF): every conv / GEMM whose output feeds a GroupNorm writes that norm's
        # partial sums from its epilogue (no statistics pass over the activation), and the transformer blocks'
        # LayerNorms are folded into the projections that consume them (no normalised activation written).
        st = NORM_HANDOFF
        x, xp = self.conv_in(sample, stats="gn") if st else (self.conv_in(sample), None)
        skips = [(x, xp)]
        share = cfg_pairs and self._cfg_share_ok(x)
        for bi, blk in enumerate(self.down_blocks):
            for i, r in enumerate(blk.resnets):
                if share and bi == 0 and i == 0:
                    # the shared prefix: the first-half views of x, of its GroupNorm partials (128-row blocks, whole
                    # images) and of the time projection; the transformer's cross-attention joins the two contexts
                    hb = B // 2
                    x, xp = r.forward_parts(x[:hb], next(ti)[:hb], xp=None if xp is None else xp[: xp.shape[0] // 2],
                                            stats=st)
                    x, xp = self._attn(blk.attentions[0], x, next(kvi), xp, st, shared=True)
                    skips.append((x, xp))
                    continue
                x, xp = r.forward_parts(x, next(ti), xp=xp, stats=st)
                if blk.attentions is not None:
                    x, xp = self._attn(blk.attentions[i], x, next(kvi), xp, st)
                skips.append((x, xp))
            if blk.downsamplers is not None:
                x, xp = blk.downsamplers[0].forward_parts(x, st)
                skips.append((x, xp))
        x, xp = self.mid_block.resnets[0].forward_parts(x, next(ti), xp=xp, stats=st)
        x, xp = self._attn(self.mid_block.attentions[0], x, next(kvi), xp, st)
        x, xp = self.mid_block.resnets[1].forward_parts(x, next(ti), xp=xp, stats=st)
        for blk in self.up_blocks:
            for i, r in enumerate(blk.resnets):
                s, sp = skips.pop()
                x, xp = r.forward_parts(x, next(ti), x2=s, xp=xp, x2p=sp, stats=st)
                if blk.attentions is not None:
                    x, xp = self._attn(blk.attentions[i], x, next(kvi), xp, st)
            if blk.upsamplers is not None:
                x, xp = blk.upsamplers[0].forward_parts(x, st)
        return self.conv_out(self.conv_norm_out(x, silu=True, part=xp))

    def _cfg_share_ok(self, x) -> bool:
        """Whether a cfg_pairs forward shares the prefix: an even batch whose first down block has attention, with at
        least ``CFG_SHARED_MIN_ROWS`` activation rows per half.  (GroupNorm partials exist only for images of whole
        128-row blocks, so their first half is the first half's partials; where a half is not whole kernel tiles the
        ops expand the shared operand.)"""
        B, H, W, _ = x.shape
        return (CFG_SHARED and B % 2 == 0 and self.down_blocks[0].attentions is not None
                and (B // 2) * H * W >= CFG_SHARED_MIN_ROWS)

    @staticmethod
    def _attn(t: "Transformer2DModel", x, ctx_kv, xp, st: bool, shared: bool = False):
        if st:
            return t.forward_parts(x, ctx_kv, xp=xp, stats=True, shared=shared)
        return t(x, ctx_kv, shared=shared), None

    # ------------------------------------------------------------------ checkpoints
    def convert_hf_state_dict(self, sd: dict) -> dict:
        """diffusers UNet2DConditionModel keys -> ours (merged QKV / KV, 1x1 proj_in)."""
        out = {}
        for k, v in sd.items():
            k2 = k.replace(".to_out.0.", ".out.")
            if ".proj_in.weight" in k2 and v.dim() == 2:
                v = v[:, :, None, None]
            out[k2] = v
        for name, m in self.named_modules():
            if isinstance(m, BasicTransformerBlock):
                merge_linear_keys(out, name + ".attn1.", ["to_q", "to_k", "to_v"], "qkv", bias=False)
                for suf in ("weight", "bias"):
                    kq = f"{name}.attn2.to_q.{suf}"
                    if kq in out:
                        out[f"{name}.attn2.q.{suf}"] = out.pop(kq)
                merge_linear_keys(out, name + ".attn2.", ["to_k", "to_v"], "kv", bias=False)
        return out

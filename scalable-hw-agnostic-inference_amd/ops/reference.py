"""Plain-PyTorch fp32 reference implementations of every native op.

Used (a) as the numerics oracle in tests (HIP kernel vs fp32 torch on the same
inputs) and (b) as the CPU execution path (tests without a GPU, and the CPU
DistilBERT "plumbing" config of BASELINE.json).  They compute in fp32 and
return the input dtype, mirroring the kernels' bf16-in / fp32-math / bf16-out.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_SILU, ACT_GELU, ACT_GELU_TANH, ACT_QUICK_GELU, ACT_RELU = range(6)
ACT_IDS = {"none": ACT_NONE, None: ACT_NONE, "silu": ACT_SILU, "gelu": ACT_GELU, "gelu_tanh": ACT_GELU_TANH,
           "gelu_pytorch_tanh": ACT_GELU_TANH, "gelu_new": ACT_GELU_TANH, "quick_gelu": ACT_QUICK_GELU,
           "relu": ACT_RELU, "swish": ACT_SILU}


def act_id(act) -> int:
    if isinstance(act, int):
        return act
    return ACT_IDS[act]


def apply_act(x: torch.Tensor, act) -> torch.Tensor:
    a = act_id(act)
    if a == ACT_SILU:
        return F.silu(x)
    if a == ACT_GELU:
        return F.gelu(x)
    if a == ACT_GELU_TANH:
        return F.gelu(x, approximate="tanh")
    if a == ACT_QUICK_GELU:
        return x * torch.sigmoid(1.702 * x)
    if a == ACT_RELU:
        return F.relu(x)
    return x


def rmsnorm(x, w, eps, residual=None, w_offset=0.0):
    xf = x.float()
    new_res = None
    if residual is not None:   # the kernels normalise the rounded sum they also return (as Hugging Face and vLLM do)
        new_res = (xf + residual.float()).to(x.dtype)
        xf = new_res.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    if w is not None:
        y = y * (w.float() + w_offset)
    return y.to(x.dtype), new_res


def layernorm(x, w, b, eps, residual=None):
    xf = x.float()
    new_res = None
    if residual is not None:   # the kernels normalise the rounded sum they also return (as Hugging Face and vLLM do)
        new_res = (xf + residual.float()).to(x.dtype)
        xf = new_res.float()
    y = F.layer_norm(xf, (x.shape[-1],), w.float() if w is not None else None, b.float() if b is not None else None,
                     eps)
    return y.to(x.dtype), new_res


def groupnorm_stats(x, gamma, beta, groups, eps):
    """x [N, HW, C] -> (scale, shift) fp32 [N, C] with y = x*scale + shift."""
    N, HW, C = x.shape
    xf = x.float().reshape(N, HW, groups, C // groups)
    mean = xf.mean(dim=(1, 3))  # [N, G]
    var = xf.var(dim=(1, 3), unbiased=False)
    rstd = torch.rsqrt(var + eps)
    g = gamma.float() if gamma is not None else torch.ones(C, device=x.device)
    b = beta.float() if beta is not None else torch.zeros(C, device=x.device)
    rstd_c = rstd.repeat_interleave(C // groups, dim=1)
    mean_c = mean.repeat_interleave(C // groups, dim=1)
    scale = rstd_c * g
    shift = b - mean_c * scale
    return scale, shift


def col_partials(y):
    """[M, N] -> [M / 128, N, 2]: per 128-row block and column (sum, sum of squares) of the bf16 values."""
    M, N = y.shape
    f = y.float().reshape(M // 128, 128, N)
    return torch.stack([f.sum(1), (f * f).sum(1)], -1)


def row_moments(y, eps):
    """[M, N] -> [M, 2] = (mean, rstd) (population variance), the LayerNorm statistics of each row."""
    f = y.float()
    mean = f.mean(-1)
    var = (f * f).mean(-1) - mean * mean
    return torch.stack([mean, torch.rsqrt(var.clamp_min(0) + eps)], -1)


def groupnorm_from_partials(part1, part2, C1, C2, Nimg, HW, gamma, beta, groups, eps):
    """GroupNorm (scale, shift) [Nimg, C1 + C2] from col partials [Nimg * HW / 128, C, 2] of one or two sources."""
    R = HW // 128
    t = part1.double().reshape(Nimg, R, C1, 2).sum(1)
    if part2 is not None:
        t = torch.cat([t, part2.double().reshape(Nimg, R, C2, 2).sum(1)], 1)
    C = C1 + C2
    tg = t.reshape(Nimg, groups, C // groups, 2).sum(2)
    cnt = HW * (C // groups)
    mean = tg[..., 0] / cnt
    var = (tg[..., 1] / cnt - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64, device=part1.device)
    b = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64, device=part1.device)
    rs = rstd.repeat_interleave(C // groups, 1)
    mu = mean.repeat_interleave(C // groups, 1)
    scale = rs * g[None, :]
    shift = b[None, :] - mu * scale
    return scale.float(), shift.float()


def groupnorm_apply(x, scale, shift, silu):
    N = x.shape[0]
    C = x.shape[-1]
    y = x.float() * scale.view(N, *([1] * (x.dim() - 2)), C) + shift.view(N, *([1] * (x.dim() - 2)), C)
    if silu:
        y = F.silu(y)
    return y.to(x.dtype)


def wrap_rows(t, rows, cols):
    """Broadcast operand by index arithmetic: row m of the [rows, cols] result is row m % t_rows of t."""
    t2 = t.reshape(-1, cols)
    assert rows % t2.shape[0] == 0, "the broadcast operand's rows must divide the output rows"
    return t2[torch.arange(rows, device=t.device) % t2.shape[0]]


def linear(x, w, bias=None, act=None, residual=None, glu=False, alpha=1.0, res_alpha=1.0, row_affine=None,
           residual_rows=0):
    """residual_rows > 0: the residual holds that many rows, and output row m adds residual row m % residual_rows."""
    y = torch.matmul(x.float(), w.float().t())
    if row_affine is not None:  # LayerNorm folded in: rstd[m] * (x w'^T - mean[m] * s[n])
        mr, s = row_affine
        mr = mr.float().reshape(-1, 2)
        y2 = y.reshape(-1, y.shape[-1])
        y = (mr[:, 1:2] * (y2 - mr[:, 0:1] * s.float()[None, :])).reshape(y.shape)
    y = y * alpha
    if bias is not None:
        y = y + bias.float()
    if glu:
        val, gate = y[..., 0::2], y[..., 1::2]
        y = val * apply_act(gate, act)
    else:
        y = apply_act(y, act)
    if residual is not None:
        r = residual.float()
        if residual_rows:
            r = wrap_rows(r, y.numel() // y.shape[-1], y.shape[-1]).reshape(y.shape)
        y = y + res_alpha * r
    return y.to(x.dtype)


# ---- MXFP4 (OCP microscaling fp4): e2m1 codes, two per byte (even k in the low nibble), one e8m0 scale byte
# (2^(byte - 127)) per 32 consecutive k of a row.  Logical shapes: codes [N, K / 2], scales [N, K / 32].  The layout the
# kernels stream (csrc/kernels/gemv_fp4.hip) keeps the codes row-major and tiles the scales per 128-wide K step:
# [ceil(K / 128), N, 4] bytes, groups past K / 32 padded with 127 (= 1.0).
MXFP4_GROUP = 32
MXFP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mxfp4_pack(codes: torch.Tensor, scale_bytes: torch.Tensor):
    """Layout helper: packed codes uint8 [N, K / 2] + scale bytes uint8 [N, K / 32] (logical layout) ->
    (wq float4_e2m1fn_x2 [N, K / 2], scales float8_e8m0fnu [ceil(K / 128), N, 4]) as the kernels read them."""
    N, K2 = codes.shape
    G = scale_bytes.shape[1]
    assert codes.dtype == torch.uint8 and scale_bytes.dtype == torch.uint8 and scale_bytes.shape[0] == N
    assert K2 * 2 == G * MXFP4_GROUP, "one scale per 32 codes"
    steps = (G + 3) // 4
    sb = torch.full((N, steps * 4), 127, dtype=torch.uint8, device=codes.device)
    sb[:, :G] = scale_bytes
    tiled = sb.view(N, steps, 4).permute(1, 0, 2).contiguous()
    return codes.contiguous().view(torch.float4_e2m1fn_x2), tiled.view(torch.float8_e8m0fnu)


def mxfp4_unpack(wq: torch.Tensor, scales: torch.Tensor):
    """Inverse of ``mxfp4_pack``: (codes uint8 [N, K / 2], scale bytes uint8 [N, K / 32])."""
    codes = wq.view(torch.uint8)
    N, K2 = codes.shape
    G = K2 * 2 // MXFP4_GROUP
    sb = scales.view(torch.uint8)
    assert sb.dim() == 3 and sb.shape[1] == N and sb.shape[2] == 4 and sb.shape[0] == (G + 3) // 4, \
        f"mxfp4 scales {tuple(sb.shape)} do not belong to codes {tuple(codes.shape)}"
    return codes, sb.permute(1, 0, 2).reshape(N, -1)[:, :G]


def quantize_mxfp4(w: torch.Tensor):
    """OCP MX quantisation of w [N, K] (K % 32 == 0) along K: per group of 32, e = floor(log2(amax)) - 2 clamped so
    that 0.5 * 2^e is a normal bf16, elements / 2^e clamped to +-6 and rounded to the nearest e2m1 value, ties to
    the even mantissa.  A dequantised weight code * 2^e is exact in bf16.  Returns ``mxfp4_pack``'s pair."""
    assert w.dim() == 2 and w.shape[1] % MXFP4_GROUP == 0 and w.shape[1] > 0, "quantize_mxfp4: w must be [N, K], K % 32 == 0"
    N, K = w.shape
    wf = w.float().reshape(N, K // MXFP4_GROUP, MXFP4_GROUP)
    amax = wf.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)                       # amax = m * 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = (ex.to(torch.int32) - 3).clamp(-125, 125)   # an all-zero group: ex = 0, e = -3 (any valid scale), codes 0
    v = torch.ldexp(wf, -e[..., None]).clamp(-6.0, 6.0)
    a = v.abs()
    # nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}; a midpoint goes to the neighbour with the even mantissa (codes 0, 2, 4, 6)
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8)
            + (a >= 1.75).to(torch.uint8) + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
            + (a > 5.0).to(torch.uint8))
    code = code | (((v < 0) & (code > 0)).to(torch.uint8) << 3)
    code = code.reshape(N, K)
    packed = code[:, 0::2] | (code[:, 1::2] << 4)
    return mxfp4_pack(packed, (e + 127).to(torch.uint8))


def dequant_mxfp4(wq: torch.Tensor, scales: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """Table decode of ``quantize_mxfp4``'s pair -> [N, K] (exact in bf16 / fp32)."""
    codes, sb = mxfp4_unpack(wq, scales)
    N, K2 = codes.shape
    table = torch.tensor(MXFP4_VALUES + tuple(-x for x in MXFP4_VALUES), dtype=torch.float32, device=codes.device)
    vals = torch.stack([table[(codes & 15).long()], table[(codes >> 4).long()]], dim=-1).reshape(N, K2 * 2)
    e = sb.to(torch.int32) - 127
    out = torch.ldexp(vals.view(N, -1, MXFP4_GROUP), e[..., None]).reshape(N, K2 * 2)
    return out.to(dtype)


def gate_rows(y, gate, rows_per_gate):
    """y [..., M, N] * gate[(b*M + m) // rows_per_gate] (flattened row index)."""
    N = y.shape[-1]
    y2 = y.reshape(-1, N)
    idx = torch.arange(y2.shape[0], device=y.device) // rows_per_gate
    return (y2 * gate.float()[idx]).reshape(y.shape)


def gemm_into(x, w, out, bias=None, act=None, residual=None, gate=None, rows_per_gate=1, alpha=1.0, res_alpha=1.0,
              glu=False):
    y = linear(x, w, bias, act, None, glu, alpha).float()
    if gate is not None:
        y = gate_rows(y, gate, rows_per_gate)
    if residual is not None:
        y = y + res_alpha * residual.float()
    out.copy_(y.to(out.dtype))
    return out


def layernorm_mod(x, scale, shift, rows_per_mod, eps):
    D = x.shape[-1]
    xf = x.float().reshape(-1, D)
    y = torch.nn.functional.layer_norm(xf, (D,), eps=eps)
    idx = torch.arange(xf.shape[0], device=x.device) // rows_per_mod
    y = y * (1 + scale.float()[idx]) + shift.float()[idx]
    return y.reshape(x.shape).to(x.dtype)


def qk_norm_rope(x, q_w, k_w, cos, sin, H, D, S, eps):
    """In place on x [rows, >= 2*H*D]: RMSNorm per head on q (cols [0, HD)) and k (cols [HD, 2HD)), then pair RoPE
    with row r at position r % S."""
    rows = x.shape[0]
    pos = torch.arange(rows, device=x.device) % S
    for j, w in enumerate((q_w, k_w)):
        t = x[:, j * H * D:(j + 1) * H * D].float().reshape(rows, H, D)
        if w is not None:
            t = t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * w.float()
        if cos is not None:
            c = cos[pos].view(rows, 1, D // 2)
            s_ = sin[pos].view(rows, 1, D // 2)
            a, b = t[..., 0::2].clone(), t[..., 1::2].clone()
            t[..., 0::2] = a * c - b * s_
            t[..., 1::2] = b * c + a * s_
        x[:, j * H * D:(j + 1) * H * D] = t.reshape(rows, H * D).to(x.dtype)
    return x


def unpack_conv_weight(w_packed, cin, kh, kw):
    cout = w_packed.shape[0]
    return w_packed.reshape(cout, kh, kw, cin).permute(0, 3, 1, 2).contiguous()


def pack_conv_weight(w):
    """torch conv weight [Cout, Cin, KH, KW] -> [Cout, KH*KW*Cin] (k ordered (kh, kw, c))."""
    cout = w.shape[0]
    return w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()


# taps of a 3x3 kernel that land on source row (column) i - 1 + p + a of output phase p of a nearest-2x upsample:
# phase 0 (even output rows 2i) reads rows i - 1 (kh 0) and i (kh 1, 2); phase 1 reads i (kh 0, 1) and i + 1 (kh 2)
_UP2_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))


def pack_up2_phase_weight(w_packed, cin):
    """Packed 3x3 weight [Cout, 9 Cin] of a conv over a nearest-2x upsampled input -> the 4 output phases' 2x2
    weights [4 Cout, 4 Cin] (phase py * 2 + px, k ordered (a, b, c)): W_ph[a][b] = sum of the 3x3 taps that read the
    same source pixel, accumulated in fp32 (csrc/kernels/gemm_8ph.hip CONV 3)."""
    cout = w_packed.shape[0]
    w = w_packed.float().reshape(cout, 3, 3, cin)
    out = w.new_zeros(2, 2, cout, 2, 2, cin)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    for kh in _UP2_TAPS[py][a]:
                        for kw in _UP2_TAPS[px][b]:
                            out[py, px, :, a, b] += w[:, kh, kw]
    return out.reshape(4 * cout, 4 * cin).to(w_packed.dtype)


def conv2d_up2_phases(x, w_phase, bias=None, temb=None, act=None):
    """Reference of the phase-decomposed upsample conv: out[n, 2i + py, 2j + px] = sum_{a, b} x[n, i - 1 + py + a,
    j - 1 + px + b] W_ph (zero outside the source)."""
    N, H, W, C = x.shape
    cout = w_phase.shape[0] // 4
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1))
    wp = w_phase.float().reshape(2, 2, cout, 2, 2, C)
    y = x.new_zeros(N, 2 * H, 2 * W, cout, dtype=torch.float32)
    for py in range(2):
        for px in range(2):
            acc = 0
            for a in range(2):
                for b in range(2):
                    acc = acc + xp[:, py + a:py + a + H, px + b:px + b + W] @ wp[py, px, :, a, b].t()
            y[:, py::2, px::2] = acc
    if bias is not None:
        y = y + bias.float()
    if temb is not None:
        y = y + temb.float()[:, None, None, :]
    return apply_act(y, act).to(x.dtype)


def conv2d(x, w_packed, bias, kh, kw, stride=1, pad=0, upsample=False, x2=None, norm=None, temb=None,
           residual=None, act=None, res_alpha=1.0, residual_rows=0):
    """x NHWC [N,H,W,C1] (+x2 [N,H,W,C2] concatenated on C) -> NHWC output.  residual_rows > 0: the residual holds
    that many output pixels (rows), and output row m adds residual row m % residual_rows."""
    xin = x.float() if x2 is None else torch.cat([x.float(), x2.float()], dim=-1)
    if norm is not None:
        scale, shift, nact = norm
        N, C = xin.shape[0], xin.shape[-1]
        xin = xin * scale.view(N, 1, 1, C) + shift.view(N, 1, 1, C)
        xin = apply_act(xin, nact)
    xin = xin.to(x.dtype).float()  # the kernel rounds the gathered operand to bf16
    if upsample:
        xin = xin.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    cin = xin.shape[-1]
    w = unpack_conv_weight(w_packed.float(), cin, kh, kw)
    y = F.conv2d(xin.permute(0, 3, 1, 2), w, None, stride=stride, padding=pad).permute(0, 2, 3, 1)
    if bias is not None:
        y = y + bias.float()
    if temb is not None:
        y = y + temb.float()[:, None, None, :]
    y = apply_act(y, act)
    if residual is not None:
        r = residual.float()
        if residual_rows:
            r = wrap_rows(r, y.numel() // y.shape[-1], y.shape[-1])
        y = y + res_alpha * r.reshape(y.shape)
    return y.to(x.dtype)


def attention(q, k, v, scale=None, causal=False, causal_offset=0, kv_lens=None, q_lens=None, bias=None,
              q_batch_mod=0):
    """q [B,Sq,Hq,D], k/v [B,Skv,Hkv,D] -> [B,Sq,Hq,D].  q_batch_mod > 0: q holds q_batch_mod batches and batch b of
    the output (k / v's batch) attends with the queries of batch b % q_batch_mod."""
    if q_batch_mod:
        assert q.shape[0] == q_batch_mod and k.shape[0] % q_batch_mod == 0
        q = q[torch.arange(k.shape[0], device=q.device) % q_batch_mod]
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(Hq // Hkv, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(Hq // Hkv, dim=1)
    if kf.shape[0] == 1 and B > 1:
        kf = kf.expand(B, -1, -1, -1)
        vf = vf.expand(B, -1, -1, -1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.float()[None]
    qi = torch.arange(Sq, device=q.device).view(1, 1, Sq, 1)
    ki = torch.arange(Skv, device=q.device).view(1, 1, 1, Skv)
    mask = torch.zeros(B, 1, Sq, Skv, dtype=torch.bool, device=q.device)
    kvl = kv_lens.view(B, 1, 1, 1).to(q.device) if kv_lens is not None else torch.full((B, 1, 1, 1), Skv,
                                                                                          device=q.device)
    mask |= ki >= kvl
    if causal:
        if q_lens is not None:
            off = kvl - q_lens.view(B, 1, 1, 1).to(q.device)
        else:
            off = causal_offset
        mask |= ki > qi + off
    s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)
    o = torch.matmul(p, vf).permute(0, 2, 1, 3).contiguous()
    if q_lens is not None:
        valid = (torch.arange(Sq, device=q.device).view(1, Sq) < q_lens.view(B, 1).to(q.device))
        o = o * valid.view(B, Sq, 1, 1)
    return o.to(q.dtype)


FP8_KV_DTYPE = torch.float8_e4m3fn   # OCP e4m3fn (not fnuz)
FP8_KV_MAX = 448.0


def quantize_kv_fp8(x, scale=1.0):
    """The fp8 KV-cache quantisation rule (the oracle every writer is tested against):
    code = RNE fp8(clamp(float(x) * (1 / scale), -448, 448)), with 1 / scale computed once in fp32 and the clamp
    applied in fp32 BEFORE the conversion (torch's conversion returns NaN above 464 without it)."""
    inv = (torch.ones((), dtype=torch.float32) / torch.tensor(float(scale), dtype=torch.float32)).to(x.device)
    return (x.float() * inv).clamp(-FP8_KV_MAX, FP8_KV_MAX).to(FP8_KV_DTYPE)


def dequant_kv_fp8(c, scale=1.0, dtype=torch.float32):
    """value = float(code) * scale (fp32 product, then one rounding to ``dtype``)."""
    return (c.float() * torch.tensor(float(scale), dtype=torch.float32, device=c.device)).to(dtype)


def is_fp8_kv(cache) -> bool:
    return cache.dtype == FP8_KV_DTYPE


def _check_kv_pair(k_cache, v_cache):
    if is_fp8_kv(k_cache) != is_fp8_kv(v_cache):
        raise ValueError(f"k_cache / v_cache dtypes differ ({k_cache.dtype} vs {v_cache.dtype})")


def gather_paged(cache, block_table, length, scale=1.0):
    """cache [blocks, H, 64, D], table row -> [length, H, D]; an fp8 cache is dequantised to fp32"""
    nb = (length + 63) // 64
    blocks = cache[block_table[:nb].long()]  # [nb, H, 64, D]
    if is_fp8_kv(cache):
        blocks = dequant_kv_fp8(blocks, scale)
    return blocks.permute(0, 2, 1, 3).reshape(nb * 64, cache.shape[1], cache.shape[3])[:length]


def kv_dequant_blocks(k_cache, v_cache, phys, k_out, v_out, k_scale=1.0, v_scale=1.0):
    """scratch block i = dequantised fp8 cache block phys[i] (k_out / v_out [capacity, H, 64, D])."""
    n = int(phys.numel())
    if n > k_out.shape[0]:
        raise ValueError(f"kv_dequant_blocks: {n} blocks do not fit the scratch capacity {k_out.shape[0]}")
    k_out[:n] = dequant_kv_fp8(k_cache[phys.long()], k_scale, k_out.dtype)
    v_out[:n] = dequant_kv_fp8(v_cache[phys.long()], v_scale, v_out.dtype)


def paged_attention(q, k_cache, v_cache, block_table, kv_lens, q_lens, scale=None, causal=True, k_scale=1.0,
                    v_scale=1.0):
    _check_kv_pair(k_cache, v_cache)
    B, Sq, Hq, D = q.shape
    out = torch.zeros_like(q)
    for b in range(B):
        L = int(kv_lens[b])
        ql = int(q_lens[b]) if q_lens is not None else Sq
        k = gather_paged(k_cache, block_table[b], L, k_scale)[None]
        v = gather_paged(v_cache, block_table[b], L, v_scale)[None]
        o = attention(q[b:b + 1, :ql], k, v, scale=scale, causal=causal, causal_offset=L - ql)
        out[b, :ql] = o[0]
    return out


def paged_attention_varlen(q, k_cache, v_cache, block_table, kv_lens, q_lens, q_start, scale=None, causal=True,
                           k_scale=1.0, v_scale=1.0):
    """q [T, Hq, D] packed (sequence b = rows q_start[b] .. + q_lens[b] - 1)."""
    _check_kv_pair(k_cache, v_cache)
    out = torch.zeros_like(q)
    for b in range(block_table.shape[0]):
        L, ql, q0 = int(kv_lens[b]), int(q_lens[b]), int(q_start[b])
        k = gather_paged(k_cache, block_table[b], L, k_scale)[None]
        v = gather_paged(v_cache, block_table[b], L, v_scale)[None]
        out[q0:q0 + ql] = attention(q[None, q0:q0 + ql], k, v, scale=scale, causal=causal, causal_offset=L - ql)[0]
    return out


def decode_attention(q, k_cache, v_cache, block_table, ctx_lens, scale=None, k_scale=1.0, v_scale=1.0):
    _check_kv_pair(k_cache, v_cache)
    B, Hq, D = q.shape
    out = torch.empty_like(q)
    for b in range(B):
        L = int(ctx_lens[b])
        k = gather_paged(k_cache, block_table[b], L, k_scale)[None]
        v = gather_paged(v_cache, block_table[b], L, v_scale)[None]
        out[b] = attention(q[b:b + 1, None], k, v, scale=scale)[0, 0]
    return out


def kv_write(k, v, k_cache, v_cache, slots, k_scale=1.0, v_scale=1.0):
    _check_kv_pair(k_cache, v_cache)
    if is_fp8_kv(k_cache):  # an fp8 cache stores the codes of quantize_kv_fp8
        k, v = quantize_kv_fp8(k, k_scale), quantize_kv_fp8(v, v_scale)
    for t in range(k.shape[0]):
        s = int(slots[t])
        if s < 0:
            continue
        k_cache[s // 64, :, s % 64] = k[t]
        v_cache[s // 64, :, s % 64] = v[t]


def rope(x, positions, cos, sin, rot_dim, neox=True):
    """in-place rotary on x [T, H, Dh]"""
    half = rot_dim // 2
    c = cos[positions.long()].unsqueeze(1)  # [T,1,half]
    s = sin[positions.long()].unsqueeze(1)
    xf = x.float()
    if neox:
        a, b = xf[..., :half], xf[..., half:rot_dim]
    else:
        a, b = xf[..., 0:rot_dim:2], xf[..., 1:rot_dim:2]
    ra = a * c - b * s
    rb = b * c + a * s
    if neox:
        x[..., :half] = ra.to(x.dtype)
        x[..., half:rot_dim] = rb.to(x.dtype)
    else:
        x[..., 0:rot_dim:2] = ra.to(x.dtype)
        x[..., 1:rot_dim:2] = rb.to(x.dtype)
    return x


def rope_pairs(x, cos, sin):
    """in-place Flux rope: x [B,T,H,Dh], cos/sin [T, Dh/2] applied to pairs (2j, 2j+1)."""
    xf = x.float()
    a, b = xf[..., 0::2], xf[..., 1::2]
    c = cos.view(1, cos.shape[0], 1, -1)
    s = sin.view(1, sin.shape[0], 1, -1)
    x[..., 0::2] = (a * c - b * s).to(x.dtype)
    x[..., 1::2] = (b * c + a * s).to(x.dtype)
    return x


def gated_act(x, act, gate_first=False):
    F_ = x.shape[-1] // 2
    a, g = x[..., :F_].float(), x[..., F_:].float()
    y = apply_act(a, act) * g if gate_first else a * apply_act(g, act)
    return y.to(x.dtype)


def bias_act(x, bias=None, residual=None, act=None, alpha=1.0):
    y = x.float() * alpha
    if bias is not None:
        y = y + bias.float()
    y = apply_act(y, act)
    if residual is not None:
        y = y + residual.float()
    return y.to(x.dtype)


def sched_step(model_out, latents, cfg, guidance, pred_type, a_t, a_prev, dt):
    n = latents.numel()
    e = model_out.float().reshape(-1)
    if cfg:
        eu, ec = e[:n], e[n:]
        e = eu + guidance * (ec - eu)
    x = latents.float().reshape(-1)
    if pred_type == 2:
        x = x + dt * e
    else:
        sa, s1a = math.sqrt(a_t), math.sqrt(1 - a_t)
        if pred_type == 0:
            eps = e
            x0 = (x - s1a * eps) / sa
        else:
            x0 = sa * x - s1a * e
            eps = sa * e + s1a * x
        x = math.sqrt(a_prev) * x0 + math.sqrt(1 - a_prev) * eps
    latents.copy_(x.view_as(latents).to(latents.dtype))
    return latents


def sched_step_rows(model_out, latents, cfg, guidance, pred_type, rows_params):
    B = latents.shape[0]
    mo = model_out.reshape(2 if cfg else 1, B, -1)
    rp = rows_params.float().cpu().tolist()
    for b in range(B):
        a_t, a_prev, dt = rp[b]
        if a_t < 0:
            continue
        out_b = torch.cat([mo[0, b], mo[1, b]]) if cfg else mo[0, b]
        sched_step(out_b, latents[b], cfg, guidance, pred_type, a_t, a_prev, dt)
    return latents


def quant_rows_fp8(x, rms_eps=None):
    """Per-row e4m3 quantisation (scale = absmax / 448, times the RMSNorm rstd with ``rms_eps``)."""
    xf = x.float()
    s = (xf.abs().amax(dim=-1) / 448.0).clamp(min=1e-30)
    a8 = (xf / s[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    if rms_eps is not None:
        s = s * torch.rsqrt(xf.pow(2).mean(-1) + rms_eps)
    return a8, s


def gemm_f8(a8, w8, a_scale, w_scale, bias=None, act=None, residual=None, glu=False, res_alpha=1.0):
    y = (a8.float() @ w8.float().t()) * a_scale.float()[:, None] * w_scale.float()[None, :]
    if bias is not None:
        y = y + bias.float()
    if glu:
        y = y[:, 0::2] * apply_act(y[:, 1::2], act)
    else:
        y = apply_act(y, act)
    if residual is not None:
        y = y + res_alpha * residual.float()
    return y.to(torch.bfloat16)


# ---------------------------------------------------------------------- sampling with penalties, min_p, logprobs
# The oracle of csrc/kernels/sampling.hip's penalised sampler and log-probability kernel (and what the CPU engine and
# the full-vocabulary route run).  Penalty state: one int32 word per (state row, vocabulary entry) -- bit 30: the
# token occurs in the request's original prompt; bits 0..29: how often the sequence has sampled it.
PENALTY_PROMPT_FLAG = 1 << 30
PENALTY_COUNT_MASK = PENALTY_PROMPT_FLAG - 1


def penalty_state_init(state, row, tokens, n_prompt):
    """Clear ``state[row]`` and scatter ``tokens`` into it: the first ``n_prompt`` set the prompt flag, the rest
    count as sampled.  Ids outside [0, V) are ignored."""
    V = state.shape[1]
    t = torch.as_tensor(tokens, dtype=torch.int64, device=state.device).reshape(-1)
    n_prompt = min(int(n_prompt), t.numel())
    ok = (t >= 0) & (t < V)
    prompt, out = t[:n_prompt][ok[:n_prompt]], t[n_prompt:][ok[n_prompt:]]
    words = torch.bincount(out, minlength=V).to(torch.int32)
    flag = torch.zeros(V, dtype=torch.bool, device=state.device)
    flag[prompt] = True
    state[row] = words | (flag.to(torch.int32) * PENALTY_PROMPT_FLAG)
    return state


def penalty_state_add(state, rows, tokens):
    """What the sampler does after picking: count token ``tokens[b]`` in state row ``rows[b]`` (rows < 0: none)."""
    if state is None:
        return
    rows, tokens = rows.long(), tokens.long()
    ok = (rows >= 0) & (rows < state.shape[0]) & (tokens >= 0) & (tokens < state.shape[1])
    state.index_put_((rows[ok], tokens[ok]), torch.ones(int(ok.sum()), dtype=state.dtype, device=state.device),
                     accumulate=True)


def penalty_words(state, rows, B, V, device):
    """The [B, V] state words of a batch (zero rows where ``rows`` < 0 or there is no table)."""
    if state is None:
        return torch.zeros(B, V, dtype=torch.int32, device=device)
    ok = (rows >= 0) & (rows < state.shape[0])
    w = state.index_select(0, rows.clamp(0, state.shape[0] - 1).long())
    return torch.where(ok[:, None], w, torch.zeros_like(w))


def penalize_logits(logits, words, rep, freq, pres):
    """fp32 logits after the penalties: where the token is in the prompt or was sampled, l / rep if l > 0 else
    l * rep (IEEE fp32 division); then l -= freq * count; then l -= pres where count > 0."""
    l = logits.float()
    if words is None:
        return l
    c = (words & PENALTY_COUNT_MASK)
    seen = words != 0
    r = rep.float()[:, None]
    l = torch.where(seen, torch.where(l > 0, l / r, l * r), l)
    l = l - freq.float()[:, None] * c.float()
    return torch.where(c > 0, l - pres.float()[:, None], l)


def sample_candidates(l, temps, top_k, top_p, min_p, uniforms, dtype=torch.float32, return_kept=False):
    """The sampling rule on (already penalised) fp32 logits ``l`` [B, V]: greedy rows (temperature <= 0) take the
    first index of the maximum; the others sort the top-k candidates (descending value, ascending index), weigh them
    p_i = exp((l_i - l_0) / T), drop p_i < min_p (candidate 0 stays), keep candidate i of the survivors while the
    mass before it is <= top_p of their total, and draw by inverse CDF at the uniform.  Candidates whose value is
    -inf are dropped with the min_p cut (candidate 0 must be finite).  ``dtype``: precision of the
    probabilities.  ``return_kept``: also the [B, V] mask of the tokens that can be drawn."""
    B, V = l.shape
    vals, idx = torch.sort(l, dim=-1, descending=True, stable=True)
    ar = torch.arange(V, device=l.device)[None, :]
    k = torch.where((top_k <= 0) | (top_k > V), torch.full_like(top_k, V), top_k)[:, None]
    greedy = temps <= 0
    T = torch.where(greedy, torch.ones_like(temps), temps).to(dtype)[:, None]
    p = torch.exp((vals - vals[:, :1]).to(dtype) / T)
    # (candidates at -inf -- tokens a constraint masks -- go before the min_p cut: they are a suffix of the sorted
    # candidates, and a masked token is never returned whatever top_k, top_p and the uniform are)
    keep = (ar < k) & (((p >= min_p.to(dtype)[:, None]) & (vals > float("-inf"))) | (ar == 0))
    p = p * keep
    cum = p.cumsum(-1)
    keep = keep & ((cum - p) <= top_p.to(dtype)[:, None] * cum[:, -1:])
    L = keep.sum(-1).clamp(min=1)
    target = uniforms.to(dtype) * cum.gather(-1, (L - 1)[:, None]).squeeze(-1)
    pick = ((cum <= target[:, None]) & (ar < (L - 1)[:, None])).sum(-1)
    pick = torch.where(greedy, torch.zeros_like(pick), pick)
    toks = idx.gather(-1, pick[:, None]).squeeze(-1)
    if not return_kept:
        return toks
    keep = torch.where(greedy[:, None], ar == 0, ar < L[:, None])
    return toks, torch.zeros(B, V, dtype=torch.bool, device=l.device).scatter_(1, idx, keep)


def sample_penalized(logits, temps, top_k, top_p, uniforms, state=None, rows=None, rep=None, freq=None, pres=None,
                     min_p=None, dtype=torch.float32, update=True):
    """Penalise, sample, and count the picked tokens in ``state`` (what the fused kernel does in one launch)."""
    B, V = logits.shape
    words = None
    if state is not None and rows is not None:
        words = penalty_words(state, rows, B, V, logits.device)
    l = penalize_logits(logits, words, rep, freq, pres)
    if min_p is None:
        min_p = torch.zeros(B, dtype=torch.float32, device=logits.device)
    toks = sample_candidates(l, temps.float(), top_k.long(), top_p.float(), min_p.float(), uniforms.float(), dtype)
    if update and state is not None and rows is not None:
        penalty_state_add(state, rows, toks)
    return toks


def token_logprobs(logits, tokens, n, row_n=None, dtype=torch.float32):
    """Log-softmax of the RAW logits at the picked token and at the ``n`` most likely tokens (descending value,
    ascending index): (vals [B, 1 + n] fp32, ids [B, 1 + n] int32).  ``row_n``: per-row count <= n; the entries past
    it read -inf / -1, and a row with a negative count is left at -inf / -1 altogether."""
    B, V = logits.shape
    lf = logits.float()
    lp = lf.to(dtype) - torch.logsumexp(lf.to(dtype), dim=-1, keepdim=True)
    m = min(int(n), V)
    _, idx = torch.sort(lf, dim=-1, descending=True, stable=True)
    idx = idx[:, :m]
    tok = tokens.long().clamp(0, V - 1)
    ids = torch.full((B, 1 + n), -1, dtype=torch.int64, device=logits.device)
    vals = torch.full((B, 1 + n), float("-inf"), dtype=dtype, device=logits.device)
    ids[:, 0], vals[:, 0] = tokens.long(), lp.gather(-1, tok[:, None]).squeeze(-1)
    ids[:, 1:1 + m], vals[:, 1:1 + m] = idx, lp.gather(-1, idx)
    if row_n is not None:
        cnt = row_n.long()[:, None]
        gone = (torch.arange(1 + n, device=logits.device)[None, :] > cnt)
        ids, vals = ids.masked_fill(gone, -1), vals.masked_fill(gone, float("-inf"))
    return vals.to(torch.float32 if dtype == torch.float32 else dtype), ids.to(torch.int32)


# ---------------------------------------------------------------------- constrained sampling
# The oracle of the constrained sampler (csrc/kernels/sampling.hip, sample_con_kernel).  A constraint PROGRAM is an
# immutable block of int32 words (``con_pack``); programs lie back to back in a pool and a row names its program by
# the block's word offset (-1: the row is unconstrained).  Block layout, CON_HDR header words then the sections:
#   header   S (states), W = ceil(V / 32), E (edges), NB (bias entries), total words of the block, 0, 0, 0
#   masks    [S, W]  allow-mask of every state: bit i & 31 of word i >> 5 set = token i allowed; pad bits zero
#   stop     [W]     the EOS ids and the request's stop_token_ids (removed from the mask of a row with ban_stop set)
#   plane    [W]     "has a bias" bits: the bias list is searched for flagged tokens only
#   default  [S]     next state of a token without an edge
#   estart   [S + 1] edges of state s: etok / enext [estart[s], estart[s + 1]), tokens ascending
#   etok, enext [E]
#   bid, bval   [NB] bias ids (ascending) and fp32 values (bit patterns)
# The mutable part is one int32 state word per sequence slot (``cstate``), advanced by the sampler after its pick.
CON_HDR = 8
CON_MAX_STATES = 1024
CON_MAX_BIAS = 300


def con_words(V):
    return (int(V) + 31) // 32


def con_mask(ids, V):
    """int32 [W] allow-mask with the bits of ``ids`` set (ids outside [0, V) are ignored; pad bits stay zero)."""
    bits = torch.zeros(con_words(V) * 32, dtype=torch.bool)
    ids = torch.as_tensor(list(ids), dtype=torch.int64).reshape(-1)
    bits[ids[(ids >= 0) & (ids < V)]] = True
    return con_mask_pack(bits)


def con_mask_pack(bits):
    """bool [..., 32 * W] -> int32 [..., W]."""
    w = (bits.reshape(*bits.shape[:-1], -1, 32).long() << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def con_mask_bits(words, V):
    """int32 [..., W] -> bool [..., V]."""
    sh = torch.arange(32, device=words.device)
    return (((words.long()[..., None] >> sh) & 1) != 0).reshape(*words.shape[:-1], -1)[..., :V]


def con_pack(V, masks, stop, default, edges, bias=()):
    """The int32 block of one program.  masks: int32 [S, W]; stop: int32 [W]; default: S next states; edges: per
    state a list of (token, next state), tokens ascending; bias: (id, value) pairs, ids ascending."""
    import numpy as np
    S, W = masks.shape
    assert W == con_words(V) and len(default) == S and len(edges) == S and stop.numel() == W
    estart, etok, enext = [0], [], []
    for es in edges:
        etok += [int(t) for t, _ in es]
        enext += [int(n) for _, n in es]
        estart.append(len(etok))
    bid = [int(i) for i, _ in bias]
    bval = np.asarray([v for _, v in bias], dtype=np.float32).view(np.int32).tolist()
    total = CON_HDR + S * W + 2 * W + S + (S + 1) + 2 * len(etok) + 2 * len(bid)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32)
    blk = torch.cat([i32([S, W, len(etok), len(bid), total, 0, 0, 0]), masks.reshape(-1).to(torch.int32),
                     stop.to(torch.int32), con_mask(bid, V), i32(list(default)), i32(estart), i32(etok), i32(enext),
                     i32(bid), i32(bval)])
    assert blk.numel() == total
    return blk


def con_view(pool, off, V):
    """The sections of the program at word offset ``off`` of ``pool`` (views), or None if there is no valid block."""
    from types import SimpleNamespace
    n = pool.numel()
    if off < 0 or off + CON_HDR > n:
        return None
    S, W, E, NB, total = pool[off:off + 5].tolist()
    if not (1 <= S <= CON_MAX_STATES and W == con_words(V) and E >= 0 and 0 <= NB <= CON_MAX_BIAS):
        return None
    if total != CON_HDR + S * W + 2 * W + S + (S + 1) + 2 * E + 2 * NB or off + total > n:
        return None
    o, out = off + CON_HDR, SimpleNamespace(S=S, W=W, E=E, NB=NB, total=total)
    for name, k in (("masks", S * W), ("stop", W), ("plane", W), ("default", S), ("estart", S + 1), ("etok", E),
                    ("enext", E), ("bid", NB), ("bval", NB)):
        setattr(out, name, pool[o:o + k])
        o += k
    out.masks = out.masks.view(S, W)
    out.bval = out.bval.view(torch.float32)
    return out


def con_rows(pool, cstate, prog, slot, V):
    """Per batch row (program view, state word index, state) or None where the row is unconstrained (no program, or
    a slot / state out of range: the kernel takes the penalised path for such a row too)."""
    out = []
    if pool is None or cstate is None:
        return [None] * prog.numel()
    views = {}
    states = cstate.tolist()
    for off, sl in zip(prog.tolist(), slot.tolist()):
        if off < 0 or not 0 <= sl < len(states):
            out.append(None)
            continue
        if off not in views:
            views[off] = con_view(pool, off, V)
        pv = views[off]
        out.append((pv, sl, states[sl]) if pv is not None and 0 <= states[sl] < pv.S else None)
    return out


def con_next(pv, state, tok):
    """The automaton's step: the edge of ``tok`` out of ``state``, else the state's default."""
    lo, hi = int(pv.estart[state]), int(pv.estart[state + 1])
    toks = pv.etok[lo:hi].tolist()
    import bisect
    j = bisect.bisect_left(toks, tok)
    if j < len(toks) and toks[j] == tok:
        return int(pv.enext[lo + j])
    return int(pv.default[state])


def ban_stop(generated, min_tokens):
    """The per-step flag of a row: EOS and the stop tokens are masked while fewer than ``min_tokens`` tokens have been
    generated."""
    return generated < min_tokens


def constrain_logits(logits, words, rep, freq, pres, rows, ban, pad_allowed=False, bias_last=False):
    """The constrained fp32 logits: raw, + bias where the token has one, the penalties (``penalize_logits``), then
    -inf where the current state does not allow the token or ``ban`` is set and the token is in the stop mask.
    ``rows``: ``con_rows``.  (pad_allowed / bias_last: mutants of the rule, for the tests.)"""
    B, V = logits.shape
    l = logits.float()
    bias = torch.zeros_like(l)
    has = torch.zeros(B, V, dtype=torch.bool, device=l.device)
    allowed = torch.ones(B, V, dtype=torch.bool, device=l.device)
    for b, r in enumerate(rows):
        if r is None:
            continue
        pv, _, st = r
        if pv.NB:
            ids = pv.bid.long()
            has[b, ids] = True
            bias[b, ids] = pv.bval
        m = pv.masks[st]
        if int(ban[b]) != 0:
            m = m & ~pv.stop
        allowed[b] = con_mask_bits(m, V)
        if pad_allowed and V % 32:
            allowed[b, V - V % 32:] = True
    if not bias_last:
        l = torch.where(has, l + bias, l)
    l = penalize_logits(l, words, rep, freq, pres)
    if bias_last:
        l = torch.where(has, l + bias, l)
    return torch.where(allowed, l, torch.full_like(l, float("-inf")))


def con_advance(cstate, rows, toks):
    """What the sampler does after picking: state' = edge(state, token), else the state's default."""
    for r, t in zip(rows, toks.tolist()):
        if r is not None:
            cstate[r[1]] = con_next(r[0], r[2], int(t))


def sample_constrained(logits, temps, top_k, top_p, uniforms, state, rows, rep, freq, pres, min_p, pool, cstate, prog,
                       slot, ban, dtype=torch.float32, update=True):
    """Constrain, penalise, sample; count the picked tokens in ``state`` and advance the automaton states in
    ``cstate`` (what the fused kernel does in one launch)."""
    B, V = logits.shape
    words = None
    if state is not None and rows is not None:
        words = penalty_words(state, rows, B, V, logits.device)
    crows = con_rows(pool, cstate, prog, slot, V)
    l = constrain_logits(logits, words, rep, freq, pres, crows, ban)
    if min_p is None:
        min_p = torch.zeros(B, dtype=torch.float32, device=logits.device)
    toks = sample_candidates(l, temps.float(), top_k.long(), top_p.float(), min_p.float(), uniforms.float(), dtype)
    if update:
        if state is not None and rows is not None:
            penalty_state_add(state, rows, toks)
        con_advance(cstate, crows, toks)
    return toks

"""Operator layer: thin wrappers over the gfx950 HIP kernels (``torch.ops.shai``).

GPU tensors always go to the native kernels (raising if the library is not
built -- no silent eager fallback).  CPU tensors use the fp32 references in
:mod:`shai_amd.ops.reference` (tests / CPU plumbing config).

All wrappers allocate their outputs with torch (graph-pool aware), launch on
the current stream and never synchronise, so whole model steps can be
captured into HIP graphs (``torch.cuda.CUDAGraph`` is hipGraph on ROCm).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from .. import native
from . import reference as ref
from .reference import (ACT_GELU, ACT_GELU_TANH, ACT_NONE, ACT_QUICK_GELU, ACT_RELU, ACT_SILU, act_id, mxfp4_pack,
                        mxfp4_unpack, quantize_mxfp4, pack_conv_weight, pack_up2_phase_weight, unpack_conv_weight)

__all__ = [
    "rmsnorm", "layernorm", "groupnorm_stats", "groupnorm_apply", "groupnorm", "linear", "conv2d", "attention",
    "paged_attention", "decode_attention", "kv_write", "rope", "rope_pairs", "gated_act", "bias_act", "sched_step",
    "softmax_", "embedding", "token_feedback", "decode_attention_rope", "decode_attention_rope_qkv", "gemm_partials", "quantize_fp8_rows", "dequant_fp8", "quantize_mxfp4", "dequant_mxfp4", "mxfp4_pack", "mxfp4_unpack", "is_mxfp4", "quant_rows_fp8", "gemm_f8", "pack_conv_weight", "pack_up2_phase_weight", "linear_wslices", "unpack_conv_weight", "act_id", "ACT_NONE", "ACT_SILU", "ACT_GELU",
    "ACT_GELU_TANH", "ACT_QUICK_GELU", "ACT_RELU", "decode_splits", "set_decode_wb",
    "paged_attention_varlen", "rope_qkv_cache", "quantize_kv_fp8", "dequant_kv_fp8", "kv_dequant_blocks",
    "plan_kv_scratch", "build_kv_rounds", "KVRound", "FP8_KV_DTYPE", "resolve_kv_prefill", "KV_PREFILL_ROUTES",
    "sample_penalized", "penalty_state_init", "token_logprobs", "LOGPROBS_MAX",
    "sample_constrained", "constraint_state_init",
]


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def _K():
    return native.ops()


def _i32(t: Optional[torch.Tensor]):
    if t is None:
        return None
    return t if t.dtype == torch.int32 else t.to(torch.int32)


# ----------------------------------------------------------------------------- norms
def rmsnorm(x: torch.Tensor, w: Optional[torch.Tensor], eps: float = 1e-6, residual: Optional[torch.Tensor] = None,
            w_offset: float = 0.0, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """y = rmsnorm(x (+ residual)) * (w + w_offset); returns (y, x + residual or None)."""
    if not _gpu(x):
        return ref.rmsnorm(x, w, eps, residual, w_offset)
    shape = x.shape
    x2 = x if x.dim() == 2 else x.reshape(-1, shape[-1])
    res2 = residual.reshape(-1, shape[-1]) if residual is not None else None
    y = out if out is not None else torch.empty(x2.shape, dtype=x.dtype, device=x.device)
    new_res = torch.empty(x2.shape, dtype=x.dtype, device=x.device) if residual is not None else None
    _K().rmsnorm(x2, w, y, res2, new_res, float(eps), float(w_offset))
    return y.view(shape), (new_res.view(shape) if new_res is not None else None)


def layernorm(x: torch.Tensor, w: Optional[torch.Tensor], b: Optional[torch.Tensor], eps: float = 1e-5,
              residual: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    if not _gpu(x):
        return ref.layernorm(x, w, b, eps, residual)
    shape = x.shape
    x2 = x if x.dim() == 2 else x.reshape(-1, shape[-1])
    res2 = residual.reshape(-1, shape[-1]) if residual is not None else None
    y = torch.empty(x2.shape, dtype=x.dtype, device=x.device)
    new_res = torch.empty(x2.shape, dtype=x.dtype, device=x.device) if residual is not None else None
    _K().layernorm(x2, w, b, y, res2, new_res, float(eps))
    return y.view(shape), (new_res.view(shape) if new_res is not None else None)


_GN_TICKETS: dict = {}
# Finalize fused into the stats launch (last-block ticket) is opt-in: on MI355X the per-block
# agent-scope add + vmcnt drain made GN+SiLU 1.3-1.45x SLOWER than a separate 8-block finalize
# launch (8x4096x320: 40.6 vs 28.2 us), so the two-launch path stays the default.
_GN_FUSED = os.environ.get("SHAI_GN_FUSED_FINALIZE", "0") == "1"


def _gn_tickets(x: torch.Tensor, n: int) -> Optional[torch.Tensor]:
    """Zeroed int32 tickets for the stats kernel's fused finalize, one set per (device, stream):
    the kernel re-arms them to 0, so they stay valid across launches and HIP-graph replays."""
    if not _GN_FUSED or n > 4096:
        return None
    key = (x.device.index, torch.cuda.current_stream(x.device).cuda_stream)
    t = _GN_TICKETS.get(key)
    if t is None:
        t = _GN_TICKETS[key] = torch.zeros(4096, dtype=torch.int32, device=x.device)
    return t


def _scale_shift_pair(n: int, c: int, device):
    """GroupNorm (scale, shift) [n, c] fp32 as the two halves of ONE allocation (shift = scale + n c): the layout
    the halo-tiled conv's scale / shift DMA reads (csrc/kernels/conv_halo.hip)."""
    ss = torch.empty(2, n, c, dtype=torch.float32, device=device)
    return ss[0], ss[1]


def groupnorm_stats(x: torch.Tensor, gamma, beta, groups: int, eps: float, x2: Optional[torch.Tensor] = None):
    """Channels-last GroupNorm statistics. x [N, ..., C] -> (scale, shift) fp32 [N, C].
    With ``x2`` the statistics are those of ``cat([x, x2], -1)`` without materialising it."""
    N = x.shape[0]
    x3 = x.reshape(N, -1, x.shape[-1])
    x23 = x2.reshape(N, -1, x2.shape[-1]) if x2 is not None else None
    C = x3.shape[-1] + (x23.shape[-1] if x23 is not None else 0)
    if not _gpu(x):
        xx = torch.cat([x3, x23], -1) if x23 is not None else x3
        return ref.groupnorm_stats(xx, gamma, beta, groups, eps)
    part = torch.empty(N * 256 * groups * 2, dtype=torch.float32, device=x.device)
    scale, shift = _scale_shift_pair(N, C, x.device)
    _K().groupnorm_stats(x3, x23, gamma, beta, part, scale, shift, _gn_tickets(x, N), int(groups), float(eps))
    return scale, shift


def groupnorm_apply(x: torch.Tensor, scale, shift, silu: bool = False, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = (silu)(x * scale + shift); with ``x2`` the input is ``cat([x, x2], -1)`` (never materialised)."""
    if not _gpu(x):
        xx = torch.cat([x, x2], -1) if x2 is not None else x
        return ref.groupnorm_apply(xx, scale, shift, silu)
    N = x.shape[0]
    C = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
    out = torch.empty(*x.shape[:-1], C, dtype=x.dtype, device=x.device)
    _K().groupnorm_apply(x.reshape(N, -1, x.shape[-1]), x2.reshape(N, -1, x2.shape[-1]) if x2 is not None else None,
                         scale, shift, out.view(N, -1, C), bool(silu))
    return out


def groupnorm(x, gamma, beta, groups, eps, silu=False, x2=None):
    scale, shift = groupnorm_stats(x, gamma, beta, groups, eps, x2=x2)
    return groupnorm_apply(x, scale, shift, silu, x2=x2)


# ----------------------------------------------------------------------------- GEMM / conv
FP8_E4M3_MAX = 448.0


def quantize_fp8_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-output-row symmetric fp8 (OCP e4m3) quantisation: w ~= w8 * scale[:, None].
    One-time load transform (not a hot op): returns (w8 float8_e4m3fn [N, K], scale fp32 [N])."""
    wf = w.float()
    scale = (wf.abs().amax(dim=1) / FP8_E4M3_MAX).clamp(min=1e-12)
    w8 = (wf / scale[:, None]).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    return w8.contiguous(), scale.contiguous()


def dequant_fp8(w8: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """w8 * scale[:, None] -> bf16 (native kernel on the GPU)."""
    if not w8.is_cuda:
        return (w8.float() * scale.float()[:, None]).to(dtype)
    out = torch.empty(w8.shape, dtype=torch.bfloat16, device=w8.device)
    _K().dequant_fp8(w8, scale, out)
    return out


# ---- MXFP4 weight-only quantisation (``quantize_mxfp4``: a load-time transform in pure torch, CPU and GPU; format and
# layout in ops/reference.py).  GEMMs stream the packed codes: <= 64 rows through the skinny kernel
# (csrc/kernels/gemv_fp4.hip), more rows through the tile kernel (csrc/kernels/gemm_fp4.hip: codes widened to bf16 in
# registers, bf16 MFMA -- weight-only and exact).  Gated / LayerNorm-folded / batched calls and the CPU dequantise to
# bf16 first.  An MX-scaled MFMA (W4A8: quantised activations, other numbers) would be a separate opt-in.
def is_mxfp4(w: torch.Tensor) -> bool:
    return w.dtype == torch.float4_e2m1fn_x2


def dequant_mxfp4(wq: torch.Tensor, scales: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """MXFP4 codes [N, K / 2] + group scales -> [N, K] (torch on the CPU, the native kernel on the GPU)."""
    if not wq.is_cuda:
        return ref.dequant_mxfp4(wq, scales, dtype)
    out = torch.empty(wq.shape[0], wq.shape[1] * 2, dtype=torch.bfloat16, device=wq.device)
    _K().dequant_mxfp4(wq, scales, out)
    return out if dtype == torch.bfloat16 else out.to(dtype)


# MXFP4 weights on problems of more than 64 rows (prefill, decode above 64 sequences): "fused" streams the packed codes
# through the fp4 tile GEMM (gemm_fp4.hip); "dequant" widens the whole matrix to bf16 per call and runs the bf16 GEMMs
MXFP4_PREFILL = os.environ.get("SHAI_MXFP4_PREFILL", "fused")
# largest row count the fused route takes (0: no cap): the largest measured M at which it is not slower than the
# dequantise route at any Mistral-7B / 70B projection shape (table in profiles/mxfp4_prefill.md: it wins 1.1-3.6x up
# to 768 rows, loses at one shape at 1024 and at every shape at 4096, where the four-wave bf16 GEMM outruns it)
MXFP4_FUSED_MAX_ROWS = int(os.environ.get("SHAI_MXFP4_FUSED_MAX_ROWS", "768"))


def _mxfp4_route(x: torch.Tensor, w: torch.Tensor, w_scale: Optional[torch.Tensor], direct_ok: bool = True):
    """(w, w_scale) for a GEMM of ``x`` against MXFP4 weights: the packed pair where an fp4 kernel takes the problem
    (GPU, K % 32 == 0; <= 64 rows: the skinny kernel; more rows: the tile kernel, unless ``MXFP4_PREFILL`` is
    "dequant" or the row count is above ``MXFP4_FUSED_MAX_ROWS``), else the dequantised bf16 matrix."""
    if w_scale is None:
        raise ValueError("MXFP4 weights need w_scale= (the group scales of quantize_mxfp4)")
    K = x.shape[-1]
    if w.shape[1] * 2 != K:
        raise ValueError(f"MXFP4 weight {tuple(w.shape)} holds K = {w.shape[1] * 2}, the activation has K = {K}")
    M = x.numel() // K
    if direct_ok and _gpu(x) and M >= 1 and K % 32 == 0:
        # (N % 4: the tile kernel wants whole column quads under GLU; such widths kept the dequantise route)
        if M <= 64 or (MXFP4_PREFILL == "fused" and w.shape[0] % 4 == 0
                       and (MXFP4_FUSED_MAX_ROWS <= 0 or M <= MXFP4_FUSED_MAX_ROWS)):
            return w, w_scale
    return dequant_mxfp4(w, w_scale), None


# fp8 weights on problems of more than 64 rows (prefill): "w8a8" quantises the activation per row on the fly and
# runs the fp8 MFMA GEMM (gemm_f8.hip); "dequant" widens the weights to bf16 and runs the bf16 GEMMs
FP8_PREFILL = os.environ.get("SHAI_FP8_PREFILL", "w8a8")


def quant_rows_fp8(x: torch.Tensor, rms_eps: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row e4m3 quantisation of a 2-D bf16 activation: x ~= a8 * scale[:, None] (scale = absmax / 448).
    With ``rms_eps`` the row's RMSNorm rstd is multiplied into the scale (the consumer's weights carry the
    folded norm gain), so the product a8 @ w^T * scale is the product of the normalised row."""
    if not _gpu(x):
        return ref.quant_rows_fp8(x, rms_eps)
    M, K = x.shape
    a8 = torch.empty(M, K, dtype=torch.float8_e4m3fn, device=x.device)
    scale = torch.empty(M, dtype=torch.float32, device=x.device)
    _K().quant_rows_fp8(x, a8, scale, float(rms_eps) if rms_eps is not None else -1.0)
    return a8, scale


def gemm_f8(a8: torch.Tensor, w8: torch.Tensor, a_scale: torch.Tensor, w_scale: torch.Tensor,
            bias: Optional[torch.Tensor] = None, act=None, residual: Optional[torch.Tensor] = None,
            glu: bool = False, res_alpha: float = 1.0, cfg: int = -1,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W8A8 GEMM on the fp8 MFMA: act(a_scale[m] * w_scale[n] * a8 @ w8^T + bias) (+ res_alpha * residual),
    GLU as in ``linear``; bf16 output."""
    if not _gpu(a8):
        return ref.gemm_f8(a8, w8, a_scale, w_scale, bias, act, residual, glu, res_alpha)
    N = w8.shape[0]
    y = out if out is not None else torch.empty(a8.shape[0], N // 2 if glu else N, dtype=torch.bfloat16,
                                                device=a8.device)
    _K().gemm_f8(a8, w8, a_scale, w_scale, y, bias, residual, float(res_alpha), act_id(act), bool(glu), int(cfg))
    return y


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act=None,
           residual: Optional[torch.Tensor] = None, glu: bool = False, alpha: float = 1.0,
           res_alpha: float = 1.0, rms_eps: Optional[float] = None,
           w_scale: Optional[torch.Tensor] = None, row_affine=None, force_cfg: int = -1,
           residual_rows: int = 0) -> torch.Tensor:
    """y = act(alpha * x @ w^T + bias) (+ res_alpha * residual).

    residual_rows > 0: ``residual`` holds that many rows and output row m adds residual row m % residual_rows (a
    B-image stream under 2B output images).  The v4 / W-stationary kernels read it in place (multiples of 256 / 32
    rows that divide M); the binding expands it for any other problem.  bf16 weights only.

    glu=True: ``w`` rows are interleaved (value_i, gate_i) pairs and the output
    has N/2 columns: value * act(gate) (SwiGLU / GEGLU fused in the epilogue).
    rms_eps: x is RMS-normalised first (unweighted: the norm gain must already be
    folded into w's columns); on the GPU this is fused into the decode GEMM.
    row_affine = (mr [M, 2] fp32, s [N] fp32): a LayerNorm of x folded into the GEMM -- y = rstd[m] * (x @ w^T -
    mean[m] * s[n]) + bias, with the norm gain / shift pre-folded into w / bias (``fold_layernorm``) and
    (mean, rstd) from the producer of x (``linear_stats`` / ``conv2d(stats="ln")``).
    w_scale: ``w`` is fp8 e4m3 with one fp32 scale per row (``quantize_fp8_rows``).  Decode-shaped
    problems (<= 64 rows) stream the fp8 bytes through the skinny kernel (half the weight
    traffic); larger ones run W8A8 on the fp8 MFMA (``FP8_PREFILL``: the activation is quantised per row, with
    the folded RMSNorm in its row scale) or dequantize to bf16 first and run the bf16 GEMMs.
    ``w`` of dtype float4_e2m1fn_x2 is MXFP4 (``quantize_mxfp4``; ``w_scale`` its e8m0 group scales): on the GPU the
    packed codes stream through the fp4 skinny kernel (<= 64 rows) or the fp4 tile GEMM (more rows, up to
    ``MXFP4_FUSED_MAX_ROWS``; ``MXFP4_PREFILL``); larger problems, a ``row_affine`` call and the CPU dequantise to bf16
    first.  force_cfg (tests / tools) then
    names an fp4 config: 1000 (+ kg) / 1100 + kg at <= 64 rows, 1300 + 32 * tile + splits above.
    """
    if is_mxfp4(w):
        w, w_scale = _mxfp4_route(x, w, w_scale, direct_ok=row_affine is None)
    if w_scale is not None and not is_mxfp4(w):
        M = x.numel() // x.shape[-1]
        K = x.shape[-1]
        if (_gpu(x) and M > 64 and FP8_PREFILL == "w8a8" and alpha == 1.0 and K % 16 == 0
                and (not glu or w.shape[0] % 4 == 0)):
            x2 = x.reshape(-1, K) if (x.dim() == 2 or x.is_contiguous()) else x.contiguous().reshape(-1, K)
            a8, a_scale = quant_rows_fp8(x2, rms_eps)
            N = w.shape[0] // 2 if glu else w.shape[0]
            r2 = residual.reshape(-1, N) if residual is not None else None
            y = gemm_f8(a8, w, a_scale, w_scale, bias, act, r2, glu, res_alpha)
            return y.view(*x.shape[:-1], N)
        if not _gpu(x) or M > 64 or K % 16 != 0:
            w = dequant_fp8(w, w_scale)
            w_scale = None
    if not _gpu(x):
        if rms_eps is not None:
            x = ref.rmsnorm(x, None, rms_eps)[0]
        return ref.linear(x, w, bias, act, residual, glu, alpha, res_alpha, row_affine=row_affine,
                          residual_rows=residual_rows)
    if row_affine is not None:
        return _linear_norm_io(x, w, bias, act, residual, glu, alpha, res_alpha, row_affine, None, 0.0, force_cfg,
                               residual_rows)[0]
    K = x.shape[-1]
    N = w.shape[0]
    lead = x.shape[:-1]
    if x.dim() == 2 or x.is_contiguous():
        x2 = x.reshape(-1, K)
    else:
        x2 = x.contiguous().reshape(-1, K)
    Nout = N // 2 if glu else N
    y = torch.empty(x2.shape[0], Nout, dtype=x.dtype, device=x.device)
    r2 = residual.reshape(-1, Nout) if residual is not None else None
    # (force_cfg names an fp4 config, or pins the kernel of a broadcast-residual problem for the tests)
    _K().gemm(x2, w, y, bias, None, 1, r2, float(alpha), float(res_alpha), act_id(act), bool(glu), None, 1,
              int(force_cfg) if (is_mxfp4(w) or residual_rows) else -1,
              float(rms_eps) if rms_eps is not None else -1.0, w_scale, None, None, None, None, 1e-5, 0,
              int(residual_rows))
    return y.view(*lead, Nout)


def _linear_norm_io(x, w, bias, act, residual, glu, alpha, res_alpha, row_affine, stats, eps, force_cfg=-1,
                    residual_rows=0):
    K = x.shape[-1]
    x2 = x.reshape(-1, K) if (x.dim() == 2 or x.is_contiguous()) else x.contiguous().reshape(-1, K)
    M, N = x2.shape[0], w.shape[0]
    Nout = N // 2 if glu else N
    y = torch.empty(M, Nout, dtype=x.dtype, device=x.device)
    r2 = residual.reshape(-1, Nout) if residual is not None else None
    mr, s = row_affine if row_affine is not None else (None, None)
    gp = torch.empty(M // 128, Nout, 2, dtype=torch.float32, device=x.device) if stats == "gn" else None
    ls = torch.empty(M, 2, dtype=torch.float32, device=x.device) if stats == "ln" else None
    _K().gemm(x2, w, y, bias, None, 1, r2, float(alpha), float(res_alpha), act_id(act), bool(glu), None, 1,
              int(force_cfg), -1.0, None, mr, s, gp, ls, float(eps), 0, int(residual_rows))
    return y.view(*x.shape[:-1], Nout), (gp if stats == "gn" else ls)


def stats_supported(rows: int, cols: int, kind: str, hw: Optional[int] = None) -> bool:
    """Whether ``linear_stats`` / ``conv2d(stats=...)`` can hand statistics of this output to the next norm:
    GroupNorm partials need 128-row blocks inside one image (hw % 128 == 0), N % 8 == 0, N <= 2048."""
    if cols % 8 != 0:
        return False
    if kind == "gn":
        return rows % 128 == 0 and cols <= 2048 and (hw is None or hw % 128 == 0)
    return True


def fold_profitable(rows: int, cols: int) -> bool:
    """A LayerNorm folded into a GEMM pins that GEMM to the v4 kernel (256-row tiles, unsplit): worth it only when
    the problem has about a wave of 256 x 320 tiles for the 256 CUs -- otherwise the standalone norm pass plus the
    tuner's choice (smaller tiles, split-K) is faster (SD2.1 at batch 1: 32 tiles)."""
    return ((rows + 255) // 256) * ((cols + 319) // 320) >= FOLD_MIN_TILES


FOLD_MIN_TILES = int(os.environ.get("SHAI_FOLD_MIN_TILES", "192"))  # tests lower it to force the folded path


def linear_stats(x: torch.Tensor, w: torch.Tensor, bias=None, residual=None, act=None, stats: str = "ln",
                 eps: float = 1e-5, row_affine=None, force_cfg: int = -1, residual_rows: int = 0):
    """``linear`` that also returns statistics of its output for the next norm: stats="ln" -> (mean, rstd) [M, 2]
    with ``eps``; "gn" -> GroupNorm partials [M / 128, N, 2] (``groupnorm_stats_from_partials``).  On the GPU the
    v4 GEMM epilogue writes them (a pass over the output when the tuned kernel cannot)."""
    if not _gpu(x):
        y = ref.linear(x, w, bias, act, residual, False, 1.0, 1.0, row_affine=row_affine,
                       residual_rows=residual_rows)
        y2 = y.reshape(-1, y.shape[-1])
        return y, (ref.row_moments(y2, eps) if stats == "ln" else ref.col_partials(y2))
    return _linear_norm_io(x, w, bias, act, residual, False, 1.0, 1.0, row_affine, stats, eps, force_cfg,
                           residual_rows)


def linear_wslices(x: torch.Tensor, w_slices: torch.Tensor, bias2d: Optional[torch.Tensor], rows_per_slice: int,
                   stats: Optional[str] = None, eps: float = 1e-5):
    """y[rows of slice s] = x[rows] w_slices[s]^T + bias2d[s]: one GEMM whose row blocks of ``rows_per_slice`` rows
    (multiples of 256) each take their own weight [N, K] -- e.g. a GroupNorm's per-image scale folded into the
    following projection's weight (``Transformer2DModel``).  x [M, K], w_slices [M / rows_per_slice, N, K], bias2d
    [M / rows_per_slice, N].  ``stats`` as ``linear_stats`` (returns (y, st) then)."""
    S, N, K = w_slices.shape
    M = x.shape[0]
    if not _gpu(x):
        y = torch.einsum("smk,snk->smn", x.float().view(S, M // S, K), w_slices.float())
        if bias2d is not None:
            y = y + bias2d.float()[:, None, :]
        y = y.reshape(M, N).to(x.dtype)
        if stats is None:
            return y
        return y, (ref.row_moments(y, eps) if stats == "ln" else ref.col_partials(y))
    y = torch.empty(M, N, dtype=x.dtype, device=x.device)
    gp = torch.empty(M // 128, N, 2, dtype=torch.float32, device=x.device) if stats == "gn" else None
    ls = torch.empty(M, 2, dtype=torch.float32, device=x.device) if stats == "ln" else None
    _K().gemm(x, w_slices.reshape(S * N, K), y, None, bias2d, int(rows_per_slice), None, 1.0, 1.0, ACT_NONE, False,
              None, 1, -1, -1.0, None, None, None, gp, ls, float(eps), int(rows_per_slice))
    if stats is None:
        return y
    return y, (gp if stats == "gn" else ls)


def linear_lnout(x: torch.Tensor, w: torch.Tensor, bias, residual: torch.Tensor, gamma, beta, eps: float = 1e-5,
                 residual_rows: int = 0):
    """(y, LayerNorm(y; gamma, beta)) with y = x @ w^T + bias + residual: the next LayerNorm computed by the producing
    GEMM's epilogue (the W-stationary kernel holds whole 320-wide rows: exact two-pass moments of the stored bf16 y),
    so the consumer runs a plain GEMM on the normalised rows.  Falls back to GEMM + standalone LayerNorm wherever
    the fused kernel does not apply (other widths, CPU)."""
    if not _gpu(x):
        y = ref.linear(x, w, bias, None, residual, residual_rows=residual_rows)
        return y, ref.layernorm(y, gamma, beta, eps)[0]
    K, N = x.shape[-1], w.shape[0]
    x2 = x.reshape(-1, K) if (x.dim() == 2 or x.is_contiguous()) else x.contiguous().reshape(-1, K)
    r2 = residual.reshape(-1, N)
    y = torch.empty(x2.shape[0], N, dtype=x.dtype, device=x.device)
    y2 = torch.empty_like(y)
    if LNOUT and _K().gemm_lnout(x2, w, y, y2, bias, r2, 1.0, gamma, beta, float(eps), int(residual_rows)):
        return y.view(*x.shape[:-1], N), y2.view(*x.shape[:-1], N)
    y = linear(x, w, bias, residual=residual, residual_rows=residual_rows)
    return y, layernorm(y, gamma, beta, eps)[0]


LNOUT = os.environ.get("SHAI_LNOUT", "1") != "0"  # A/B switch for the producer-side LayerNorm (linear_lnout)


def lnout_supported(rows: int, n: int, k: int) -> bool:
    """Whether linear_lnout runs fused on the GPU (W-stationary kernel: K = N = 320)."""
    return LNOUT and n == 320 and k == 320


def fold_layernorm(w: torch.Tensor, bias: Optional[torch.Tensor], gamma: Optional[torch.Tensor],
                   beta: Optional[torch.Tensor]):
    """(w', bias', s) so that LayerNorm(x; gamma, beta) @ w^T + bias == rstd * (x @ w'^T - mean * s) + bias':
    w' = w * gamma (columns), bias' = bias + w @ beta, s = row sums of w' (fp32, from its bf16 values)."""
    wf = w.float()
    w2 = (wf * gamma.float()[None, :]).to(w.dtype) if gamma is not None else w
    b2 = bias.float() if bias is not None else torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
    if beta is not None:
        b2 = b2 + wf @ beta.float()
    return w2.contiguous(), b2.to(w.dtype), w2.float().sum(1).contiguous()


def row_moments(x: torch.Tensor, eps: float) -> torch.Tensor:
    """(mean, rstd) [M, 2] of the rows of x [..., N] (the statistics a folded LayerNorm consumes)."""
    x2 = x.reshape(-1, x.shape[-1])
    if not _gpu(x):
        return ref.row_moments(x2, eps)
    mr = torch.empty(x2.shape[0], 2, dtype=torch.float32, device=x.device)
    _K().row_moments(x2, mr, float(eps))
    return mr


def col_partials(x: torch.Tensor) -> torch.Tensor:
    """GroupNorm partials [M / 128, N, 2] of x [..., N] (rows grouped by 128)."""
    x2 = x.reshape(-1, x.shape[-1])
    if not _gpu(x):
        return ref.col_partials(x2)
    part = torch.empty(x2.shape[0] // 128, x2.shape[1], 2, dtype=torch.float32, device=x.device)
    _K().col_partials(x2, part)
    return part


def groupnorm_stats_from_partials(part: torch.Tensor, gamma, beta, groups: int, eps: float, nimg: int, hw: int,
                                  part2: Optional[torch.Tensor] = None):
    """GroupNorm (scale, shift) fp32 [N, C] from the partials of x (and of x2 for cat([x, x2], -1))."""
    C1 = part.shape[-2]
    C2 = part2.shape[-2] if part2 is not None else 0
    if not part.is_cuda:
        return ref.groupnorm_from_partials(part, part2, C1, C2, nimg, hw, gamma, beta, groups, eps)
    scale, shift = _scale_shift_pair(nimg, C1 + C2, part.device)
    _K().groupnorm_from_partials(part, part2, C1, C2, nimg, hw, gamma, beta, scale, shift, int(groups), float(eps))
    return scale, shift


def gemm_into(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias=None, act=None, residual=None, gate=None,
              rows_per_gate: int = 1, alpha: float = 1.0, res_alpha: float = 1.0, glu: bool = False,
              force_cfg: int = -1, rms_eps: float = -1.0, w_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = gate[row // rows_per_gate] * act(alpha * x @ w^T + bias) + res_alpha * residual, written into ``out``.
    rms_eps >= 0: x is RMS-normalised first (unweighted; fold the gain into w).
    w_scale: fp8 e4m3 ``w`` with per-row scales (skinny kernel only, as in ``linear``), or the group scales of an
    MXFP4 ``w`` (2-D x without a gate: the fp4 skinny kernel at <= 64 rows, force_cfg 1000 (+ kg) / 1100 + kg as
    below, the fp4 tile GEMM above, force_cfg 1300 + 32 * tile + splits; anything else dequantises first).
    force_cfg (tests / tools): a tile config index, 1000 (+ kg) = skinny kernel with a separate split-K fold,
    1100 + kg = skinny kernel reducing its K groups inside the launch, 2000 = hipBLASLt.

    x / out / residual are 2D [M, *] or 3D [B, M, *] views whose rows may be strided
    (e.g. the text / image halves of a joint-sequence buffer); the row index used
    for ``gate`` is the flattened b * M + m (AdaLN-Zero gates per image)."""
    if is_mxfp4(w):
        w, w_scale = _mxfp4_route(x, w, w_scale, direct_ok=x.dim() == 2 and gate is None)
        if w_scale is None and force_cfg >= 1000:
            force_cfg = -1  # the forced number named the fp4 kernel
    if not _gpu(x):
        if w_scale is not None:
            w = dequant_fp8(w, w_scale)
        if rms_eps >= 0:
            x = ref.rmsnorm(x, None, rms_eps)[0]
        return ref.gemm_into(x, w, out, bias, act, residual, gate, rows_per_gate, alpha, res_alpha, glu)
    _K().gemm(x, w, out, bias, None, 1, residual, float(alpha), float(res_alpha), act_id(act), bool(glu), gate,
              int(rows_per_gate), int(force_cfg), float(rms_eps), w_scale)
    return out


def layernorm_mod(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, rows_per_mod: int,
                  eps: float = 1e-6, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """AdaLN: LayerNorm(x) (no affine) * (1 + scale[r // rows_per_mod]) + shift[r // rows_per_mod].
    scale / shift: [G, D] (may be strided column chunks of one modulation tensor)."""
    if not _gpu(x):
        y = ref.layernorm_mod(x, scale, shift, rows_per_mod, eps)
        return out.copy_(y) if out is not None else y
    x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
    y = out if out is not None else torch.empty(x2.shape, dtype=x.dtype, device=x.device)
    _K().layernorm_mod(x2, scale, shift, y if y.dim() == 2 else y.view(-1, x.shape[-1]), int(rows_per_mod),
                       float(eps))
    return y.view(x.shape) if out is None else out


def qk_norm_rope(x: torch.Tensor, q_w, k_w, cos, sin, heads: int, head_dim: int, seq: int, eps: float = 1e-6):
    """In place on a packed QKV buffer x [rows, >= 2*H*D]: per-head RMSNorm of q and k (weights optional) and
    pair RoPE with cos/sin [seq, D/2] (row r uses position r % seq)."""
    if not _gpu(x):
        return ref.qk_norm_rope(x, q_w, k_w, cos, sin, heads, head_dim, seq, eps)
    _K().qk_norm_rope(x, q_w, k_w, cos, sin, int(heads), int(head_dim), int(seq), float(eps))
    return x


def bmm(a: torch.Tensor, w: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """Batched C[b] = alpha * a[b] @ w[b]^T (a [B,M,K], w [B,N,K])."""
    if not _gpu(a):
        return (torch.matmul(a.float(), w.float().transpose(-1, -2)) * alpha).to(a.dtype)
    B, M, K = a.shape
    N = w.shape[-2]
    y = torch.empty(B, M, N, dtype=a.dtype, device=a.device)
    _K().gemm(a, w, y, None, None, 1, None, float(alpha), 1.0, ACT_NONE, False)
    return y


def set_decode_wb(mode: int = -1) -> int:
    """Decode attention routing at D 128 / GQA 4 / one split: 1 = the wave-per-block short-context kernel (default),
    0 = the split kernel (``SHAI_DECODE_WB=0``); -1 keeps the mode.  Returns the previous mode (A/B in one process)."""
    return int(_K().set_decode_wb(int(mode)))


def set_halo_conv(mode: int = -1, waves: int = -1) -> int:
    """Routing of the halo-tiled conv (csrc/kernels/conv_halo.hip): mode 0 off (default, SHAI_HALO_CONV), 1
    GroupNorm-fused convs, 2 also plain 3x3 convs; waves 4 / 8 pins its wave layout (0: default).  -1 keeps a
    setting.  Returns the previous mode (A/B in one process)."""
    return int(_K().set_halo_conv(int(mode), int(waves)))


# upsample + 3x3 conv as 4 output-phase 2x2 convs over the source (2.25x fewer MACs; SHAI_UP2_PHASES=0: off)
UP2_PHASES = os.environ.get("SHAI_UP2_PHASES", "1") != "0"
# models keep the 9-tap conv below this many 256 x 256 output tiles (``up2_phases_ok(..., cout=)``)
UP2_MIN_TILES = int(os.environ.get("SHAI_UP2_MIN_TILES", "256"))


def up2_phases_ok(x: torch.Tensor, kh: int, kw: int, stride: int, pad: int, x2=None, norm=None, residual=None,
                  cout: int = 0, temb=None) -> bool:
    """Whether an upsample conv of this shape runs phase-decomposed (v4 kernel CONV 3): plain 3x3 pad-1 conv, 64-channel
    multiples, H and W powers of two; below H W = 256 the rows run over groups of 256 / (H W) images (N a multiple,
    no per-image bias), so a 256-row tile still holds one phase.  With cout given, at least 256 output tiles: a small
    problem (SD2.1 at batch 1) stays on the 9-tap conv (measured: b32 +3.2 % img/s; b1 p50 1-1.3 % slower with every
    shape phased, split-K or not)."""
    N, H, W, C = x.shape
    if cout and (4 * N * H * W // 256) * ((cout + 255) // 256) < UP2_MIN_TILES:
        return False
    pow2 = (H & (H - 1)) == 0 and (W & (W - 1)) == 0
    grouped = H * W < 256
    return (UP2_PHASES and x.is_cuda and kh == 3 and kw == 3 and stride == 1 and pad == 1 and x2 is None and norm is None
            and residual is None and C % 64 == 0 and pow2
            and (not grouped or (N % (256 // (H * W)) == 0 and temb is None)))


def _bias2d_in_place(t: torch.Tensor) -> bool:
    """Whether the kernels read this per-image bias where it lies (``GemmArgs::bias2d_ld``): contiguous, or a column
    slice of a wider matrix whose rows start 16-byte aligned.  Anything else is copied first."""
    if t.is_contiguous():
        return True
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0


def conv2d(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], kh: int, kw: int, stride: int = 1,
           pad: int = 0, upsample: bool = False, x2: Optional[torch.Tensor] = None, norm=None,
           temb: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act=None,
           res_alpha: float = 1.0, stats: Optional[str] = None, eps: float = 1e-5,
           w_up2: Optional[torch.Tensor] = None, residual_rows: int = 0):
    """NHWC implicit-GEMM convolution with fused prologue/epilogue.

    norm = (scale [N,Cin] f32, shift [N,Cin] f32, act) applies GroupNorm(+act) to
    the input: on the GPU one vectorised apply pass + the tuned conv inside the op (``set_halo_conv(1)``: the
    halo-tiled conv normalises each staged element once in LDS instead -- measured slower at the SD2.1 shapes);
    x2 is concatenated on channels; upsample reads a
    nearest-2x view; temb [N, Cout] is a per-image bias (a column slice of a wider matrix is read in place);
    residual is added last (residual_rows > 0: it holds that
    many output pixels and output row m adds residual row m % residual_rows, as ``linear``).  w_up2: the phase weights
    (``pack_up2_phase_weight``) of an upsample conv -- used when ``up2_phases_ok``.
    stats="gn" / "ln": also return statistics of the output for the next norm, as ``linear_stats`` -- (out, st);
    st is None when the output shape cannot carry them (``stats_supported``).
    """
    if not _gpu(x):
        y = ref.conv2d(x, w_packed, bias, kh, kw, stride, pad, upsample, x2, norm, temb, residual, act, res_alpha,
                       residual_rows)
        if stats is None:
            return y
        y2 = y.reshape(-1, y.shape[-1])
        if not stats_supported(y2.shape[0], y2.shape[1], stats, y.shape[1] * y.shape[2]):
            return y, None
        return y, (ref.row_moments(y2, eps) if stats == "ln" else ref.col_partials(y2))
    N, H, W, _ = x.shape
    IH, IW = (2 * H, 2 * W) if upsample else (H, W)
    OH = (IH + 2 * pad - kh) // stride + 1
    OW = (IW + 2 * pad - kw) // stride + 1
    cout = w_packed.shape[0]
    out = torch.empty(N, OH, OW, cout, dtype=x.dtype, device=x.device)
    sc, sh, nact = (norm if norm is not None else (None, None, None))
    M = N * OH * OW
    if stats is not None and not stats_supported(M, cout, stats, OH * OW):
        want = None
    else:
        want = stats
    gp = torch.empty(M // 128, cout, 2, dtype=torch.float32, device=x.device) if want == "gn" else None
    ls = torch.empty(M, 2, dtype=torch.float32, device=x.device) if want == "ln" else None
    if temb is not None and not _bias2d_in_place(temb):
        temb = temb.contiguous()
    if upsample and w_up2 is not None and up2_phases_ok(x, kh, kw, stride, pad, x2, norm, residual, temb=temb):
        _K().conv2d(x, None, w_up2, out, bias, temb, None, None, None, 0, 2, 2, 1, 0, True, act_id(act), 1.0, None,
                    None, gp, ls, float(eps), True)
    else:
        _K().conv2d(x, x2, w_packed, out, bias, temb, residual, sc, sh, act_id(nact), kh, kw, stride, pad,
                    bool(upsample), act_id(act), float(res_alpha), None, None, gp, ls, float(eps), False,
                    int(residual_rows))
    if stats is None:
        return out
    return out, (gp if want == "gn" else ls)


# ----------------------------------------------------------------------------- attention
def attention(q, k, v, scale: Optional[float] = None, causal: bool = False, causal_offset: int = 0, kv_lens=None,
              q_lens=None, bias=None, out: Optional[torch.Tensor] = None, q_batch_mod: int = 0) -> torch.Tensor:
    """Fused flash attention. q [B,Sq,Hq,D] (packed heads), k/v [B,Skv,Hkv,D].  q_batch_mod > 0: q holds q_batch_mod
    batches and batch b of k / v / the output attends with the queries of batch b % q_batch_mod (read in place by the
    D = 64 LDS-DMA kernels, expanded by the binding for any other)."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if not _gpu(q):
        o = ref.attention(q, k, v, scale, causal, causal_offset, kv_lens, q_lens, bias, q_batch_mod)
        return out.copy_(o) if out is not None else o
    oshape = (k.shape[0],) + tuple(q.shape[1:]) if q_batch_mod else q.shape
    o = out if out is not None else torch.empty(oshape, dtype=q.dtype, device=q.device)
    _K().flash_attn(q, k, v, o, float(scale), bool(causal), int(causal_offset), _i32(kv_lens), _i32(q_lens), bias,
                    None, 1.0, 1.0, int(q_batch_mod))
    return o


# ----------------------------------------------------------------------------- fp8 (OCP e4m3fn) KV cache
FP8_KV_DTYPE = ref.FP8_KV_DTYPE


def _kv8(k_cache, v_cache) -> bool:
    """True for an fp8 cache pair; a mixed pair is an error on every path."""
    ref._check_kv_pair(k_cache, v_cache)
    return k_cache.dtype == FP8_KV_DTYPE


def quantize_kv_fp8(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """The fp8 KV-cache quantisation rule: RNE e4m3fn of clamp(float(x) * (1 / scale), -448, 448)."""
    return ref.quantize_kv_fp8(x, scale)


def dequant_kv_fp8(c: torch.Tensor, scale: float = 1.0, dtype=torch.bfloat16) -> torch.Tensor:
    """float(code) * scale, rounded once to ``dtype``."""
    return ref.dequant_kv_fp8(c, scale, dtype)


def kv_dequant_blocks(k_cache, v_cache, phys, k_out, v_out, k_scale: float = 1.0, v_scale: float = 1.0):
    """Widen the fp8 cache blocks ``phys`` [n] into blocks 0 .. n-1 of the bf16 scratch caches ``k_out`` / ``v_out``
    [capacity, Hkv, 64, D] (value = float(code) * scale).  One launch for K and V."""
    if not _gpu(k_cache):
        return ref.kv_dequant_blocks(k_cache, v_cache, phys, k_out, v_out, k_scale, v_scale)
    if not _kv8(k_cache, v_cache):
        raise ValueError(f"kv_dequant_blocks needs float8_e4m3fn caches, got {k_cache.dtype}")
    _K().kv_dequant_blocks(k_cache, v_cache, _i32(phys), k_out, v_out, float(k_scale), float(v_scale))


@dataclass
class KVRound:
    """One dequant + attention round of a prefill step over an fp8 cache: the cache blocks ``phys`` are widened into
    scratch blocks 0 .. n-1 and the sequences ``sel`` of the step attend them through ``block_table`` (remapped to
    scratch indices).  Rounds cover every sequence of the step exactly once; sequences write disjoint q rows."""
    phys: torch.Tensor                 # [n] int32 cache block ids
    block_table: torch.Tensor          # [b, max_blocks] int32 scratch block ids
    kv_lens: torch.Tensor              # [b] int32
    q_lens: Optional[torch.Tensor]     # [b] int32
    q_start: Optional[torch.Tensor]    # [b] int32 (packed varlen layout) or None (padded [B, S] layout)
    max_q: int
    sel: Optional[torch.Tensor]        # [b] int64 sequence rows of this round; None = all of the step's sequences
    n_blocks: int = 0


def plan_kv_scratch(need: Sequence[int], capacity: int) -> List[List[int]]:
    """Group sequences (in order) so that each group's cache blocks fit a scratch of ``capacity`` blocks: ``need[i]``
    is sequence i's block count.  Every sequence lands in exactly one group; a single sequence larger than the
    scratch cannot be attended and raises."""
    groups: List[List[int]] = []
    cur: List[int] = []
    used = 0
    for i, n in enumerate(need):
        n = int(n)
        if n > capacity:
            raise ValueError(f"sequence {i} needs {n} KV blocks but the dequantisation scratch holds {capacity}")
        if cur and used + n > capacity:
            groups.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += n
    if cur:
        groups.append(cur)
    return groups


def build_kv_rounds(block_table, kv_lens, q_lens, q_start, capacity: int, device, max_q: Optional[int] = None
                    ) -> List[KVRound]:
    """Host-side plan of a prefill step over an fp8 cache (all inputs host arrays: no device sync): the rounds of
    :func:`plan_kv_scratch` with their remapped block tables, uploaded once."""
    import numpy as np
    bt = np.asarray(block_table, dtype=np.int32)
    kvl = np.asarray(kv_lens, dtype=np.int32)
    ql = None if q_lens is None else np.asarray(q_lens, dtype=np.int32)
    qs = None if q_start is None else np.asarray(q_start, dtype=np.int32)
    B, mb = bt.shape
    need = (kvl.astype(np.int64) + 63) // 64
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device, non_blocking=True)
    rounds = []
    groups = plan_kv_scratch(need, capacity)
    for g in groups:
        rbt = np.zeros((len(g), mb), dtype=np.int32)
        phys, off = [], 0
        for r, i in enumerate(g):
            n = int(need[i])
            phys.append(bt[i, :n])
            rbt[r, :n] = np.arange(off, off + n, dtype=np.int32)
            off += n
        phys = np.concatenate(phys) if phys else np.zeros(0, np.int32)
        gi = np.asarray(g, dtype=np.int64)
        mq = int(ql[gi].max()) if (ql is not None and qs is not None) else int(max_q or 0)
        rounds.append(KVRound(t(phys), t(rbt), t(kvl[gi]), None if ql is None else t(ql[gi]),
                              None if qs is None else t(qs[gi]), mq, None if len(groups) == 1 else t(gi), off))
    return rounds


KV_PREFILL_ROUTES = ("widen", "native")


def resolve_kv_prefill(kv_prefill: Optional[str] = None) -> str:
    """Route of the prefill attention over an fp8 cache: ``native`` reads the codes in the paged flash kernel (one
    launch: no scratch, no rounds, no host read of device metadata); ``widen`` copies the blocks a step needs into
    a bf16 scratch and runs the bf16 kernel on it.  None reads ``SHAI_KV8_PREFILL`` (unset: widen)."""
    name = kv_prefill if kv_prefill is not None else os.environ.get("SHAI_KV8_PREFILL")
    name = "widen" if name is None or str(name).strip() == "" else str(name).strip().lower()
    if name not in KV_PREFILL_ROUTES:
        raise ValueError(f"kv_prefill={name!r}: supported: " + ", ".join(KV_PREFILL_ROUTES))
    return name


def _paged_kv8(q, k_cache, v_cache, block_table, kv_lens, q_lens, q_start, max_q, scale, causal, k_scale, v_scale,
               scratch, rounds):
    """Prefill attention over an fp8 cache: widen the blocks a round needs into the bf16 scratch, run the bf16
    kernel on it with the remapped table.  Without ``rounds`` (operator-level calls) the plan is built here from
    the device metadata, which synchronises; the engine passes the plan it made while building the batch."""
    if rounds is None:
        cap = scratch[0].shape[0] if scratch is not None else None
        need = int(((kv_lens.cpu().long() + 63) // 64).sum())
        rounds = build_kv_rounds(block_table.cpu().numpy(), kv_lens.cpu().numpy(),
                                 None if q_lens is None else q_lens.cpu().numpy(),
                                 None if q_start is None else q_start.cpu().numpy(), cap if cap is not None else
                                 max(need, 1), q.device, max_q)
    if scratch is None:
        cap = max(max(r.n_blocks for r in rounds), 1)
        shape = (cap,) + tuple(k_cache.shape[1:])
        scratch = (torch.empty(shape, dtype=q.dtype, device=q.device), torch.empty(shape, dtype=q.dtype,
                                                                                   device=q.device))
    ks, vs = scratch
    o = torch.zeros(q.shape, dtype=q.dtype, device=q.device) if len(rounds) != 1 else torch.empty(
        q.shape, dtype=q.dtype, device=q.device)
    for r in rounds:
        kv_dequant_blocks(k_cache, v_cache, r.phys, ks, vs, k_scale, v_scale)
        if q_start is not None:   # packed rows: the round's sequences address their own rows of q / o
            _K().paged_attn_varlen(q, ks, vs, o, r.block_table, r.kv_lens, r.q_lens, r.q_start, int(r.max_q),
                                   float(scale), bool(causal))
        elif r.sel is None:
            _K().flash_attn(q, ks, vs, o, float(scale), bool(causal), 0, r.kv_lens, r.q_lens, None, r.block_table)
        else:
            qs_ = q.index_select(0, r.sel)
            os_ = torch.empty_like(qs_)
            _K().flash_attn(qs_, ks, vs, os_, float(scale), bool(causal), 0, r.kv_lens, r.q_lens, None,
                            r.block_table)
            o.index_copy_(0, r.sel, os_)
    return o


def paged_attention(q, k_cache, v_cache, block_table, kv_lens, q_lens, scale=None, causal=True,
                    k_scale: float = 1.0, v_scale: float = 1.0, scratch=None, rounds=None,
                    kv_prefill: Optional[str] = None):
    """Prefill attention over a paged KV cache (64-token blocks).  An fp8 cache (``k_scale`` / ``v_scale``) takes
    the route ``kv_prefill`` (:func:`resolve_kv_prefill`; ignored for a bf16 cache): ``native`` is one launch of the
    paged kernel on the codes (``scratch`` / ``rounds`` are ignored); ``widen`` copies the blocks into the bf16
    ``scratch`` pair ([capacity, Hkv, 64, D]) in one or more ``rounds``.  On the CPU both run the reference."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    native = _kv8(k_cache, v_cache) and resolve_kv_prefill(kv_prefill) == "native"
    if not _gpu(q):
        return ref.paged_attention(q, k_cache, v_cache, block_table, kv_lens, q_lens, scale, causal, k_scale, v_scale)
    if native:
        o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        _K().flash_attn(q, k_cache, v_cache, o, float(scale), bool(causal), 0, _i32(kv_lens), _i32(q_lens), None,
                        _i32(block_table), float(k_scale), float(v_scale))
        return o
    if _kv8(k_cache, v_cache):
        return _paged_kv8(q, k_cache, v_cache, block_table, kv_lens, q_lens, None, q.shape[1], scale, causal,
                          k_scale, v_scale, scratch, rounds)
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _K().flash_attn(q, k_cache, v_cache, o, float(scale), bool(causal), 0, _i32(kv_lens), _i32(q_lens), None,
                    _i32(block_table))
    return o


def paged_attention_varlen(q, k_cache, v_cache, block_table, kv_lens, q_lens, q_start, max_q: int, scale=None,
                           causal=True, k_scale: float = 1.0, v_scale: float = 1.0, scratch=None, rounds=None,
                           kv_prefill: Optional[str] = None, q_groups=None):
    """Packed (varlen) prefill attention over a paged KV cache: q [T, Hq, D] holds every sequence's new tokens
    back to back (sequence b = rows q_start[b] .. + q_lens[b] - 1), so no padding rows are computed.  An fp8 cache
    takes the route ``kv_prefill`` as in :func:`paged_attention`.  ``q_groups`` (native route; host integers): launch
    groups ``(first sequence, count, largest q_len)`` that partition the step's sequences -- the engine's prefill
    chunks and the decode rows that joined them -- instead of one launch sized by ``max_q``."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    native = _kv8(k_cache, v_cache) and resolve_kv_prefill(kv_prefill) == "native"
    if not _gpu(q):
        return ref.paged_attention_varlen(q, k_cache, v_cache, block_table, kv_lens, q_lens, q_start, scale, causal,
                                          k_scale, v_scale)
    if native:
        o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        bt, kl, ql, qs = _i32(block_table), _i32(kv_lens), _i32(q_lens), _i32(q_start)
        # the grid is (max_q / 128 query tiles) x heads x sequences: one launch per group keeps a step's decode rows
        # (q_len 1) from being dispatched a long prompt's worth of query tiles that exit at once
        for first, n, mq in (q_groups if q_groups else [(0, bt.shape[0], max_q)]):
            if n > 0:
                _K().paged_attn_varlen(q, k_cache, v_cache, o, bt[first:first + n], kl[first:first + n],
                                       ql[first:first + n], qs[first:first + n], int(mq), float(scale), bool(causal),
                                       float(k_scale), float(v_scale))
        return o
    if _kv8(k_cache, v_cache):
        return _paged_kv8(q, k_cache, v_cache, block_table, kv_lens, q_lens, q_start, max_q, scale, causal, k_scale,
                          v_scale, scratch, rounds)
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _K().paged_attn_varlen(q, k_cache, v_cache, o, _i32(block_table), _i32(kv_lens), _i32(q_lens), _i32(q_start),
                           int(max_q), float(scale), bool(causal))
    return o


# largest top-k the fused sampler keeps exactly (csrc/kernels/sampling.hip candidate buffer); rows asking for
# more (or for no top-k at all, top_k <= 0) are sampled over the full vocabulary by the torch path
SAMPLER_MAX_K = 1024


def decode_splits(batch: int, hkv: int, max_ctx: int) -> int:
    """Split-K factor of the paged decode attention: enough (sequence, KV head, split) workgroups to fill
    the chip (``SHAI_DECODE_WG`` of them, default 512 = two per CU), at most one split per 64-token block."""
    nblk = max(1, (max_ctx + 63) // 64)
    target = int(os.environ.get("SHAI_DECODE_WG", "512"))
    want = max(1, target // max(1, batch * hkv))
    return int(min(nblk, want, 64))


def _kv8_kw(k_cache, v_cache, k_scale, v_scale) -> dict:
    """Extra kernel arguments of an fp8 cache (none for bf16: those calls stay exactly as they were)."""
    return {"k_scale": float(k_scale), "v_scale": float(v_scale)} if _kv8(k_cache, v_cache) else {}


def decode_attention(q, k_cache, v_cache, block_table, ctx_lens, scale=None, num_splits: Optional[int] = None,
                     max_ctx: Optional[int] = None, out=None, k_scale: float = 1.0, v_scale: float = 1.0):
    """Paged single-token decode attention. q [B,Hq,D].  An fp8 cache (dtype float8_e4m3fn, values = code * scale)
    always runs the split kernel's fp8 form."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if not _gpu(q):
        return ref.decode_attention(q, k_cache, v_cache, block_table, ctx_lens, scale, k_scale, v_scale)
    B, Hq, _ = q.shape
    if num_splits is None:
        mc = max_ctx if max_ctx is not None else block_table.shape[1] * 64
        num_splits = decode_splits(B, k_cache.shape[1], mc)
    ws = torch.empty(B * Hq * num_splits * (D + 2), dtype=torch.float32, device=q.device)
    o = out if out is not None else torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _K().decode_attn(q, k_cache, v_cache, o, _i32(block_table), _i32(ctx_lens), ws, int(num_splits), float(scale),
                     **_kv8_kw(k_cache, v_cache, k_scale, v_scale))
    return o


SPEC_MAX_T = 8   # query tokens per sequence the verify kernel takes (1 + up to 7 drafts)


def spec_attention_native(q, k_cache, v_cache) -> bool:
    """Whether :func:`spec_attention` runs csrc/kernels/attention_spec.hip for these operands (GPU, bf16 cache,
    D 64 / 128, T <= 8, Hq / Hkv in {1, 2, 4, 8}); everything else takes the padded paged prefill kernel."""
    if not _gpu(q) or _kv8(k_cache, v_cache) or os.environ.get("SHAI_SPEC_ATTN", "1") == "0":
        return False
    _, T, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    return D in (64, 128) and T <= SPEC_MAX_T and Hq % Hkv == 0 and Hq // Hkv in (1, 2, 4, 8)


def spec_attention(q, k_cache, v_cache, block_table, ctx_lens, q_lens, scale=None, num_splits: Optional[int] = None,
                   out=None, k_scale: float = 1.0, v_scale: float = 1.0):
    """Verify attention of speculative decoding: q [B, T, Hq, D] holds each sequence's last token and its drafts,
    whose K / V are already in the paged cache; ``ctx_lens`` count them.  Row (b, t) sees the keys
    j < ctx_lens[b] - q_lens[b] + t + 1; rows t >= q_lens[b] are unspecified.  The split kernel of
    attention_spec.hip reads each K / V block once per KV head for all T * Hq / Hkv rows; unsupported cases
    (:func:`spec_attention_native`) run the padded :func:`paged_attention` (an fp8 cache its native route), the CPU
    ``ref.paged_attention``."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if not _gpu(q):
        o = ref.paged_attention(q, k_cache, v_cache, block_table, ctx_lens, q_lens, scale, True, k_scale, v_scale)
    elif spec_attention_native(q, k_cache, v_cache):
        B, T, Hq, _ = q.shape
        if num_splits is None:
            num_splits = decode_splits(B, k_cache.shape[1], block_table.shape[1] * 64)
        ws = torch.empty(B * T * Hq * num_splits * (D + 2), dtype=torch.float32, device=q.device)
        o = out if out is not None else torch.empty(q.shape, dtype=q.dtype, device=q.device)
        _K().spec_attn(q, k_cache, v_cache, o, _i32(block_table), _i32(ctx_lens), _i32(q_lens), ws, int(num_splits),
                       float(scale))
        return o
    else:
        o = paged_attention(q, k_cache, v_cache, block_table, ctx_lens, q_lens, scale, causal=True, k_scale=k_scale,
                            v_scale=v_scale, kv_prefill="native")
    if out is not None:
        out.copy_(o)
        return out
    return o


def decode_attention_rope(qkv, k_cache, v_cache, block_table, ctx_lens, positions, cos, sin, slots, h: int, hk: int,
                          scale=None, num_splits: Optional[int] = None, max_ctx: Optional[int] = None, out=None,
                          k_scale: float = 1.0, v_scale: float = 1.0):
    """One fused decode step on the packed QKV rows qkv [B, (h + 2 hk) D]: NeoX RoPE on q / k, this step's k / v
    written into the paged caches at ``slots`` (-1: padding row), attention over the cached context plus the
    new token (``ctx_lens`` count it).  Equivalent to rope_qkv_cache + decode_attention.  Returns [B, h D]."""
    D = k_cache.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    B = qkv.shape[0]
    if not _gpu(qkv):
        rope_qkv_cache(qkv, positions, cos, sin, k_cache, v_cache, slots, h, hk, k_scale, v_scale)
        q = qkv[:, : h * D].reshape(B, h, D)
        return decode_attention(q, k_cache, v_cache, block_table, ctx_lens, scale, k_scale=k_scale,
                                v_scale=v_scale).reshape(B, h * D)
    if num_splits is None:
        mc = max_ctx if max_ctx is not None else block_table.shape[1] * 64
        num_splits = decode_splits(B, hk, mc)
    ws = torch.empty(B * h * num_splits * (D + 2), dtype=torch.float32, device=qkv.device)
    o = out if out is not None else torch.empty(B, h * D, dtype=qkv.dtype, device=qkv.device)
    _K().decode_attn_rope(qkv, k_cache, v_cache, o, _i32(block_table), _i32(ctx_lens), _i32(positions), cos, sin,
                          _i32(slots), ws, int(h), int(hk), int(num_splits), float(scale),
                          **_kv8_kw(k_cache, v_cache, k_scale, v_scale))
    return o


def gemm_partials(x, w, rms_eps: float) -> torch.Tensor:
    """Decode-shaped x [M <= 64, K] times w [N, K]^T with the folded RMSNorm of x, left UNFOLDED: the skinny
    kernel's split-K fp32 partials [kg][M][N] followed by the [kg][M] row sums of squares (kg = numel / (M (N + 1)),
    at least 2).  decode_attention_rope_qkv folds them (no separate reduce launch)."""
    return _K().gemm_partials(x, w, float(rms_eps))


def decode_attention_rope_qkv(x, w_qkv, rms_eps: float, k_cache, v_cache, block_table, ctx_lens, positions, cos, sin,
                              slots, h: int, hk: int, scale=None, num_splits: Optional[int] = None, out=None,
                              k_scale: float = 1.0, v_scale: float = 1.0):
    """decode_attention_rope on qkv = linear(rmsnorm(x), w_qkv) (norm gain folded into w_qkv) with the QKV GEMM's
    split-K fold done inside the attention kernel.  Same values as the two-step form: the kernel adds the partial
    slabs in the fold's order and rounds q / k / v to bf16 as the fold's epilogue does.  Returns [B, h D]."""
    if not _gpu(x):
        return decode_attention_rope(linear(x, w_qkv, rms_eps=rms_eps), k_cache, v_cache, block_table, ctx_lens,
                                     positions, cos, sin, slots, h, hk, scale, num_splits, out=out, k_scale=k_scale,
                                     v_scale=v_scale)
    D = k_cache.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    B, K = x.shape
    N = w_qkv.shape[0]
    if num_splits is None:
        num_splits = decode_splits(B, hk, block_table.shape[1] * 64)
    part = gemm_partials(x, w_qkv, rms_eps)
    kg = part.numel() // (B * (N + 1))
    ws = torch.empty(B * h * num_splits * (D + 2), dtype=torch.float32, device=x.device)
    o = out if out is not None else torch.empty(B, h * D, dtype=x.dtype, device=x.device)
    # qkv slot: the (read-only) partials stand in -- never an alias of the mutated output o
    _K().decode_attn_rope(part, k_cache, v_cache, o, _i32(block_table), _i32(ctx_lens), _i32(positions), cos, sin,
                          _i32(slots), ws, int(h), int(hk), int(num_splits), float(scale), part, int(kg), int(K),
                          float(rms_eps), **_kv8_kw(k_cache, v_cache, k_scale, v_scale))
    return o


def kv_write(k, v, k_cache, v_cache, slots, k_scale: float = 1.0, v_scale: float = 1.0):
    """k / v [T, Hkv, D] into the paged caches at ``slots``; an fp8 cache stores quantize_kv_fp8(x, scale)."""
    if not _gpu(k):
        return ref.kv_write(k, v, k_cache, v_cache, slots, k_scale, v_scale)
    _K().kv_write(k, v, k_cache, v_cache, _i32(slots), **_kv8_kw(k_cache, v_cache, k_scale, v_scale))


# ----------------------------------------------------------------------------- elementwise
def rope(x, positions, cos, sin, rot_dim: Optional[int] = None, neox: bool = True):
    """In-place rotary embedding on x [T, H, Dh] (token stride may be > H*Dh)."""
    rot = rot_dim if rot_dim is not None else x.shape[-1]
    if not _gpu(x):
        return ref.rope(x, positions, cos, sin, rot, neox)
    _K().rope(x, _i32(positions), cos, sin, int(rot), bool(neox))
    return x


def rope_qkv_cache(qkv, positions, cos, sin, k_cache, v_cache, slots, heads: int, kv_heads: int,
                   k_scale: float = 1.0, v_scale: float = 1.0):
    """Packed QKV rows [T, (H + 2Hkv) * D]: NeoX RoPE on q in place, rotated k and v written to the paged
    caches [blocks, Hkv, 64, D] at ``slots`` (-1 = skip).  One fused kernel on the GPU."""
    T = qkv.shape[0]
    D = k_cache.shape[-1]
    if not _gpu(qkv):
        q = qkv[:, : heads * D].view(T, heads, D)
        k = qkv[:, heads * D:(heads + kv_heads) * D].view(T, kv_heads, D).clone()   # as the kernel: k in qkv stays
        v = qkv[:, (heads + kv_heads) * D:].view(T, kv_heads, D)
        ref.rope(q, positions, cos, sin, D, True)
        ref.rope(k, positions, cos, sin, D, True)
        ref.kv_write(k, v, k_cache, v_cache, slots, k_scale, v_scale)
        return qkv
    _K().rope_qkv_cache(qkv, _i32(positions), cos, sin, k_cache, v_cache, _i32(slots), int(heads), int(kv_heads),
                        **_kv8_kw(k_cache, v_cache, k_scale, v_scale))
    return qkv


def sample(logits, temps, top_k, top_p, uniforms, out):
    """Fused temperature / top-k / top-p sampling (GPU only; one workgroup per row)."""
    _K().sample(logits, temps, top_k, top_p, uniforms, out)
    return out


LOGPROBS_MAX = 20   # most top log-probabilities a request may ask for (vLLM's limit)


def sample_penalized(logits, temps, top_k, top_p, uniforms, out, state, state_rows, rep, freq, pres, min_p,
                     full_vocab=False):
    """``sample`` with repetition / frequency / presence penalties and min_p, into ``out`` (int32).  ``state``:
    the [rows, V] int32 penalty-state table or None; ``state_rows[b]``: row b's state row, -1 for none.  The picked
    tokens are counted in the state by the same call.  On the GPU one fused kernel (top_k <= 1024 candidates);
    ``full_vocab`` (rows without such a top-k) and CPU tensors run the oracle (``reference.sample_penalized``)."""
    if not _gpu(logits) or full_vocab:
        out.copy_(ref.sample_penalized(logits, temps, top_k, top_p, uniforms, state, state_rows, rep, freq, pres,
                                       min_p))
        return out
    _K().sample_penalized(logits.contiguous(), temps, top_k, top_p, uniforms, out, state, state_rows, rep, freq,
                          pres, min_p)
    return out


def sample_constrained(logits, temps, top_k, top_p, uniforms, out, state, state_rows, rep, freq, pres, min_p, pool,
                       cstate, prog, slot, ban, full_vocab=False):
    """``sample_penalized`` under constraint programs (``reference.con_pack``), into ``out`` (int32).  ``pool``: int32
    [P], the programs back to back; ``prog[b]``: word offset of row b's program, -1 = unconstrained (exactly the
    penalised path); ``cstate``: int32 [slots] automaton state words, ``slot[b]`` row b's; ``ban[b]`` != 0 removes the
    program's stop mask this step.  The same call counts the picked tokens in ``state`` and advances the state words.
    On the GPU one fused kernel; ``full_vocab`` and CPU tensors run the oracle (``reference.sample_constrained``)."""
    if not _gpu(logits) or full_vocab:
        out.copy_(ref.sample_constrained(logits, temps, top_k, top_p, uniforms, state, state_rows, rep, freq, pres,
                                         min_p, pool, cstate, prog, slot, ban))
        return out
    _K().sample_constrained(logits.contiguous(), temps, top_k, top_p, uniforms, out, state, state_rows, rep, freq,
                            pres, min_p, pool, cstate, prog, slot, ban)
    return out


def constraint_state_init(cstate, slot, value):
    """``cstate[slot] = value`` (one sequence's automaton state) as one stream-ordered launch."""
    if not 0 <= int(slot) < cstate.numel() or not 0 <= int(value) < ref.CON_MAX_STATES:
        raise ValueError(f"constraint_state_init: slot {slot} of {cstate.numel()}, state {value}")
    if not _gpu(cstate):
        cstate[int(slot)] = int(value)
        return cstate
    _K().constraint_state_init(cstate, int(slot), int(value))
    return cstate


def penalty_state_init(state, row, tokens, n_prompt):
    """(Re)initialise row ``row`` of the penalty-state table in one launch: clear it, then scatter ``tokens`` (a
    list or an int32 tensor) -- the first ``n_prompt`` are the request's prompt (flagged), the rest its sampled
    tokens (counted).  Ids outside [0, V) are ignored."""
    if not _gpu(state):
        return ref.penalty_state_init(state, int(row), tokens, n_prompt)
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.tensor(list(tokens), dtype=torch.int32)
    _K().penalty_state_init(state, int(row), tokens.to(device=state.device, dtype=torch.int32).contiguous(),
                            int(n_prompt))
    return state


def token_logprobs(logits, tokens, n, row_n=None, vals=None, ids=None):
    """Log-softmax of the raw logits at ``tokens`` (int32 [B]) and at the ``n`` most likely tokens of each row:
    (vals fp32 [B, 1 + n], ids int32 [B, 1 + n]), entry 0 the picked token, the rest by descending value then
    ascending index.  ``row_n`` (int32 [B]): per-row count <= n, negative = skip the row."""
    if not 0 <= int(n) <= LOGPROBS_MAX:
        raise ValueError(f"token_logprobs: n={n} outside 0..{LOGPROBS_MAX}")
    if not _gpu(logits):
        v, i = ref.token_logprobs(logits, tokens, int(n), row_n)
        if vals is None:
            return v, i
        vals.copy_(v)
        ids.copy_(i)
        return vals, ids
    B = logits.shape[0]
    if vals is None:
        vals = torch.empty(B, 1 + int(n), dtype=torch.float32, device=logits.device)
        ids = torch.empty(B, 1 + int(n), dtype=torch.int32, device=logits.device)
    _K().token_logprobs(logits.contiguous(), tokens, row_n, vals, ids)
    return vals, ids


def rope_pairs(x, cos, sin):
    """In-place Flux RoPE on x [B, T, H, Dh] with cos/sin [T, Dh/2]."""
    if not _gpu(x):
        return ref.rope_pairs(x, cos, sin)
    _K().rope_pairs(x, cos, sin)
    return x


def gated_act(x, act="silu", gate_first: bool = False):
    """[.., 2F] -> [.., F]: a*act(g) (gate_first: act(a)*g)."""
    if not _gpu(x):
        return ref.gated_act(x, act, gate_first)
    F_ = x.shape[-1] // 2
    out = torch.empty(*x.shape[:-1], F_, dtype=x.dtype, device=x.device)
    x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
    _K().gated_act(x2, out.view(-1, F_), act_id(act), bool(gate_first))
    return out


def bias_act(x, bias=None, residual=None, act=None, alpha: float = 1.0):
    if not _gpu(x):
        return ref.bias_act(x, bias, residual, act, alpha)
    x = x.contiguous()
    out = torch.empty_like(x)
    _K().bias_act(x, bias, residual.contiguous() if residual is not None else None, out, act_id(act), float(alpha))
    return out


def sched_step(model_out, latents, cfg: bool, guidance: float, pred_type: int, a_t: float, a_prev: float,
               dt: float = 0.0):
    """Fused CFG + scheduler update, in place on latents."""
    if not _gpu(latents):
        return ref.sched_step(model_out, latents, cfg, guidance, pred_type, a_t, a_prev, dt)
    _K().sched_step(model_out, latents, bool(cfg), float(guidance), int(pred_type), float(a_t), float(a_prev),
                    float(dt))
    return latents


def sched_step_rows(model_out, latents, cfg: bool, guidance: float, pred_type: int, rows_params):
    """Per-row fused CFG + scheduler update (step-level batching): latents [B, ...], every row at its own step;
    rows_params fp32 [B, 3] = (a_t, a_prev, dt) per row, a_t < 0 marks an idle row (left unchanged)."""
    if not _gpu(latents):
        return ref.sched_step_rows(model_out, latents, cfg, guidance, pred_type, rows_params)
    _K().sched_step_rows(model_out, latents, bool(cfg), float(guidance), int(pred_type), rows_params.contiguous())
    return latents


def softmax_(x, scale: float = 1.0):
    if not _gpu(x):
        x.copy_(torch.softmax(x.float() * scale, dim=-1).to(x.dtype))
        return x
    _K().softmax_(x, float(scale))
    return x


def token_feedback(ids, rowmap, prev):
    """In place: ids[i] = prev[rowmap[i]] where rowmap[i] >= 0 (decode-step token feedback; all int32)."""
    if not _gpu(ids):
        prev_rows = prev.index_select(0, rowmap.clamp(min=0).long())
        ids.copy_(torch.where(rowmap >= 0, prev_rows, ids))
        return ids
    _K().token_feedback(ids, rowmap, prev)
    return ids


def embedding(ids, table):
    if not _gpu(table):
        return table[ids.long()]
    out = torch.empty(*ids.shape, table.shape[1], dtype=table.dtype, device=table.device)
    _K().embedding(_i32(ids).contiguous(), table, out)
    return out

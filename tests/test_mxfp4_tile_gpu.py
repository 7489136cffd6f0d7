"""MXFP4 tile GEMM (csrc/kernels/gemm_fp4.hip): fp4 weights above 64 activation rows without a dequantise pass.

The reference everywhere is fp32 torch on the CPU over ``ops.dequant_mxfp4(wq, s, dtype=float32)`` (the CPU table
decode; the dequantised weights are exact in bf16, so no quantisation error enters a tolerance) -- never the kernel
under test.  Bounds: the project's rel < 1e-2 for plain problems and 2e-2 for GLU + RMSNorm (the skinny kernel's), and
rel < 1e-3 between two routes that multiply identical bf16 values with fp32 accumulation and so differ in summation
order only (``test_fp4_skinny_forced_configs`` uses it for that situation)."""
import pytest
import torch

from shai_amd import ops
from test_mxfp4_cpu import all_codes_case, group_scaled_weights

pytestmark = pytest.mark.gpu

TILE_CFGS = (1300, 1332)          # force_cfg of tile 0 (128 x 128) / tile 1 (256 x 128); + splits
RAGGED = [(65, 96, 64), (130, 320, 2112), (300, 512, 1024), (257, 1024, 4096)]


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


def _quantised(n, k, seed):
    """(wq, scales, dequantised fp32 [n, k]) on the CPU."""
    wq, s = ops.quantize_mxfp4(group_scaled_weights(n, k, seed))
    return wq, s, ops.dequant_mxfp4(wq, s, dtype=torch.float32)


def _glu_rms_ref(x, wd, eps=1e-5):
    xf = x.float().cpu()
    h = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)) @ wd.t()
    return h[:, 0::2] * torch.nn.functional.silu(h[:, 1::2])


@pytest.mark.parametrize("cfg", [-1] + [c + sp for c in TILE_CFGS for sp in (0, 1)])
def test_every_code_exactly(cuda, cfg):
    """All 256 byte values under scales 2^-20 .. 2^15 against two permutation matrices: every output is one product,
    so the result is the decode table bit for bit (nibble order, sign, scale group, row index; N << tile, K = half a
    step, M just above a tile quarter)."""
    wq, s, want = all_codes_case()
    x = torch.zeros(96, 64)
    x[:64] = torch.eye(64)
    cols = (torch.arange(32) * 7 + 3) % 64
    x[64 + torch.arange(32), cols] = 1.0
    y = ops.linear(x.bfloat16().to(cuda), wq.to(cuda), w_scale=s.to(cuda), force_cfg=cfg)
    assert y.shape == (96, 16) and y.dtype == torch.bfloat16
    table = torch.cat([want.t(), want.t()[cols]])
    torch.testing.assert_close(y.float().cpu(), table, atol=0, rtol=0)


@pytest.fixture(scope="module")
def ragged(cuda):
    """Per (M, N, K): inputs, the fp32 CPU reference and the fused route's output (bias + residual)."""
    out = {}
    for M, N, K in RAGGED:
        torch.manual_seed(M + N)
        wq, s, wd = _quantised(N, K, M + N)
        x, b, r = torch.randn(M, K).bfloat16(), torch.randn(N).bfloat16(), torch.randn(M, N).bfloat16()
        want = x.float() @ wd.t() + b.float() + r.float()
        dev = tuple(t.to(cuda) for t in (x, wq, b, r, s))
        y = ops.linear(dev[0], dev[1], dev[2], residual=dev[3], w_scale=dev[4])
        out[(M, N, K)] = (dev, want, y)
    return out


@pytest.mark.parametrize("shape", RAGGED)
def test_ragged_shapes_against_fp32(ragged, shape):
    """Rows, columns and K off every tile edge (K = 2112 is 16.5 steps)."""
    _, want, y = ragged[shape]
    rel = _rel(y, want)
    print("tile plain", shape, "rel", rel)
    assert rel < 1e-2


@pytest.mark.parametrize("shape", RAGGED)
def test_agrees_with_dequantise_route(ragged, shape, monkeypatch):
    (x, wq, b, r, s), _, y = ragged[shape]
    monkeypatch.setattr(ops, "MXFP4_PREFILL", "dequant")
    y2 = ops.linear(x, wq, b, residual=r, w_scale=s)
    rel = _rel(y, y2)
    print("tile vs dequant", shape, "rel", rel)
    assert rel < 1e-3


def test_glu_rmsnorm(cuda):
    torch.manual_seed(4)
    M, N, K = 200, 2 * 320, 512
    wq, s, wd = _quantised(N, K, 4)
    x = (torch.randn(M, K) * 3).bfloat16()
    y = ops.linear(x.to(cuda), wq.to(cuda), act="silu", glu=True, rms_eps=1e-5, w_scale=s.to(cuda))
    assert y.shape == (M, N // 2)
    rel = _rel(y, _glu_rms_ref(x, wd))
    print("tile glu+rms rel", rel)
    assert rel < 2e-2


def test_forced_configs(cuda):
    """Every tile config unsplit and with 2 and 4 K splits (K = 2112: 17 steps, the last half filled), GLU."""
    torch.manual_seed(7)
    M, N, K = 192, 256, 2112
    wq, s, wd = _quantised(N, K, 7)
    x = torch.randn(M, K).bfloat16()
    h = x.float() @ wd.t()
    want = h[:, 0::2] * torch.nn.functional.silu(h[:, 1::2])
    xg, wg, sg = x.to(cuda), wq.to(cuda), s.to(cuda)
    outs = {}
    for cfg in [c + sp for c in TILE_CFGS for sp in (1, 2, 4)]:
        out = torch.empty(M, N // 2, device=cuda, dtype=torch.bfloat16)
        ops.gemm_into(xg, wg, out, act="silu", glu=True, w_scale=sg, force_cfg=cfg)
        outs[cfg] = out
        rel = _rel(out, want)
        print("tile forced", cfg, "rel", rel)
        assert rel < 2e-2, cfg
    cfgs = sorted(outs)
    for i, a in enumerate(cfgs):
        for b in cfgs[i + 1:]:
            rel = _rel(outs[a], outs[b])
            print("tile forced", a, "vs", b, "rel", rel)
            assert rel < 1e-3, (a, b)
    out = torch.empty(M, N // 2, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="force_cfg"):      # a skinny number above 64 rows
        ops.gemm_into(xg, wg, out, act="silu", glu=True, w_scale=sg, force_cfg=1001)
    with pytest.raises(RuntimeError, match="force_cfg"):      # a tile number at 8 rows
        ops.gemm_into(xg[:8], wg, out[:8], act="silu", glu=True, w_scale=sg, force_cfg=1300)


def test_strided_rows_and_column_slice(cuda):
    """x = every second row of a buffer, out and residual column slices of wider buffers (ldc, ldr > N): the result
    is right and the neighbouring columns keep their sentinel."""
    torch.manual_seed(9)
    M, N, K = 150, 200, 320
    wq, s, wd = _quantised(N, K, 9)
    buf = torch.randn(2 * M, K).bfloat16()
    b = torch.randn(N).bfloat16()
    rwide = torch.randn(M, N + 24).bfloat16()
    want = buf[::2].float() @ wd.t() + b.float() + rwide[:, 8:8 + N].float()
    x = buf.to(cuda)[::2]
    res = rwide.to(cuda)[:, 8:8 + N]
    wide = torch.full((M, N + 64), 777.0, device=cuda, dtype=torch.bfloat16)
    out = wide[:, 32:32 + N]
    assert x.stride(0) == 2 * K and out.stride(0) == N + 64
    ops.gemm_into(x, wq.to(cuda), out, b.to(cuda), residual=res, w_scale=s.to(cuda))
    rel = _rel(out, want)
    print("tile strided rel", rel)
    assert rel < 1e-2
    assert bool((wide[:, :32] == 777.0).all()) and bool((wide[:, 32 + N:] == 777.0).all())


def _no_dequant(*a, **k):
    raise AssertionError("ops.dequant_mxfp4 called: the GEMM fell back to the dequantise route")


def test_route(cuda, monkeypatch):
    torch.manual_seed(3)
    wq, s, wd = _quantised(512, 1024, 3)
    wg, sg = wq.to(cuda), s.to(cuda)
    x = torch.randn(300, 1024).bfloat16()
    xg = x.to(cuda)
    monkeypatch.setattr(ops, "dequant_mxfp4", _no_dequant)
    y = ops.linear(xg, wg, w_scale=sg)                         # above 64 rows: the tile kernel, no dequantise pass
    assert _rel(y, x.float() @ wd.t()) < 1e-2
    y = ops.linear(xg.view(3, 100, 1024), wg, w_scale=sg)      # flattenable leading dims
    assert y.shape == (3, 100, 512) and _rel(y.view(300, 512), x.float() @ wd.t()) < 1e-2
    y64 = ops.linear(xg[:64], wg, w_scale=sg)                  # the skinny kernel, as before
    assert _rel(y64, x[:64].float() @ wd.t()) < 1e-2
    with pytest.raises(AssertionError, match="dequantise route"):     # a gate still dequantises
        ops.gemm_into(xg, wg, torch.empty(300, 512, device=cuda, dtype=torch.bfloat16),
                      gate=torch.ones(300, 512, device=cuda, dtype=torch.bfloat16), w_scale=sg)
    with pytest.raises(AssertionError, match="dequantise route"):     # a folded LayerNorm still dequantises
        ops.linear(xg, wg, w_scale=sg, row_affine=(torch.zeros(300, 2, device=cuda), torch.zeros(512, device=cuda)))
    monkeypatch.setattr(ops, "MXFP4_PREFILL", "dequant")
    with pytest.raises(AssertionError, match="dequantise route"):
        ops.linear(xg, wg, w_scale=sg)
    ops.linear(xg[:64], wg, w_scale=sg)                        # <= 64 rows never depended on the switch


# ---------------------------------------------------------------------------- engine
N_DEC = 4           # prefill + 3 decode steps
LOGIT_TOL = 3e-2


class _Recorder:
    """Greedy generation on an engine whose model.forward is wrapped once: every step's logits are kept, and
    ``forced`` replaces each step's appended tokens so two engines see the same sequences."""

    def __init__(self, eng):
        self.eng, self.logits = eng, []
        fwd = eng.model.forward

        def forward(*a, **k):
            y = fwd(*a, **k)
            self.logits.append(y.float().clone())
            return y
        eng.model.forward = forward
        self._append = eng._append

    def run(self, prompts, n_dec, forced=None):
        from shai_amd.engines.llm import SamplingParams
        self.logits = []
        eng = self.eng
        seqs = [eng.add_request(p, SamplingParams(max_tokens=n_dec, temperature=0.0, ignore_eos=True))
                for p in prompts]
        row = {id(q): i for i, q in enumerate(seqs)}
        eng._append = self._append if forced is None else (
            lambda ss, toks: self._append(ss, [forced[row[id(q)]][len(q.output)] for q in ss]))
        while not all(q.finished for q in seqs):
            eng.step()
        eng._append = self._append
        return self.logits, [list(q.output) for q in seqs]


@pytest.fixture(scope="module")
def engines(cuda):
    """(mxfp4 engine, bf16 engine carrying its dequantised weights), both eager so every step's logits are visible."""
    from shai_amd.engines.llm import LLMEngine
    from shai_amd.models.llama import LlamaConfig
    from shai_amd.parallel.layers import FP8_LAYER_TYPES
    c = LlamaConfig.tiny()
    kw = dict(device=cuda, max_num_seqs=80, max_model_len=256, seed=1, enable_prefix_caching=False)
    e4 = LLMEngine(c, quantization="mxfp4", use_graphs=False, async_decode=False, **kw)
    e16 = LLMEngine(c, use_graphs=False, async_decode=False, **kw)
    q = {n: m for n, m in e4.model.named_modules() if isinstance(m, FP8_LAYER_TYPES)}
    assert q and all(m.weight.dtype == torch.float4_e2m1fn_x2 for m in q.values())
    for n, m in e16.model.named_modules():
        if isinstance(m, FP8_LAYER_TYPES):
            m.weight.data.copy_(ops.dequant_mxfp4(q[n].weight, q[n].w_scale))
    return c, kw, _Recorder(e4), _Recorder(e16)


def _fp4_rows(monkeypatch):
    """Row counts of every ops.linear call on MXFP4 weights from here on."""
    rows, lin = set(), ops.linear

    def linear(x, w, *a, **k):
        if ops.is_mxfp4(w):
            rows.add(x.numel() // x.shape[-1])
        return lin(x, w, *a, **k)
    monkeypatch.setattr(ops, "linear", linear)
    return rows


def test_engine_packed_prefill(engines, monkeypatch):
    """Prompts of 50 and 45 tokens: one packed 95-row prefill through the tile kernel, then decode steps."""
    c, _, r4, r16 = engines
    monkeypatch.setattr(ops, "dequant_mxfp4", _no_dequant)
    rows = _fp4_rows(monkeypatch)
    prompts = [[(7 * i + 3) % c.vocab_size for i in range(50)], [(11 * i + 5) % c.vocab_size for i in range(45)]]
    ref_logits, ref_toks = r16.run(prompts, N_DEC)
    got_logits, got_toks = r4.run(prompts, N_DEC, forced=ref_toks)
    assert 95 in rows, rows
    assert got_toks == ref_toks and len(got_logits) == len(ref_logits) == N_DEC
    for i, (g, r) in enumerate(zip(got_logits, ref_logits)):
        assert g.shape == r.shape
        rel = _rel(g, r)
        print("tile engine step", i, "logits rel", rel)
        assert rel < LOGIT_TOL, i


def test_engine_decode_above_64_sequences(engines, monkeypatch, cuda):
    """72 sequences: the decode step is a 72-row GEMM, eagerly and inside the replayed graph with look-ahead.  The
    default engine's greedy tokens equal the eager MXFP4 engine's; a step may differ only where the bf16 reference's
    own margin between the two tokens is inside the logit tolerance (2 x 3e-2 of the row's largest logit), and the
    comparison of that sequence ends there."""
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    c, kw, r4, r16 = engines
    prompts = [[(5 * b + 13 * i + 1) % c.vocab_size for i in range(3 + b % 4)] for b in range(72)]
    ref_logits, ref_toks = r16.run(prompts, N_DEC)
    monkeypatch.setattr(ops, "dequant_mxfp4", _no_dequant)
    rows = _fp4_rows(monkeypatch)
    _, eager = r4.run(prompts, N_DEC)
    decode = rows - {sum(len(p) for p in prompts)}   # (the engine pads a decode batch to its size bucket)
    assert decode and all(m >= 72 for m in decode), rows
    ed = LLMEngine(c, quantization="mxfp4", **kw)
    assert ed.use_graphs and ed.async_decode
    out = [list(q.output) for q in
           ed.generate(prompts, SamplingParams(max_tokens=N_DEC, temperature=0.0, ignore_eos=True))]
    assert all(len(o) == N_DEC and all(0 <= t < c.vocab_size for t in o) for o in out)

    def within_margin(b, t, tok_a, tok_b):
        rowl = ref_logits[t][b]   # [B, V] logits of each sequence's last token
        return abs((rowl[tok_a] - rowl[tok_b]).item()) <= 2 * LOGIT_TOL * rowl.abs().max().item()

    for b in range(72):
        for t in range(N_DEC):
            toks = {out[b][t], eager[b][t], ref_toks[b][t]}
            if len(toks) == 1:
                continue
            # the reference's logits describe this step only while all three sequences are still the same
            assert all(within_margin(b, t, ref_toks[b][t], tok) for tok in toks), (b, t, out[b], eager[b], ref_toks[b])
            break

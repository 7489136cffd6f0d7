"""MXFP4 weight-only path on the GPU: the dequantise kernel against the CPU table decode, the fp4 skinny decode GEMM
(csrc/kernels/gemv_fp4.hip) against fp32 torch on the dequantised weights (which are exact in bf16, so no
quantisation error enters a tolerance), the dequantise route for prefill-shaped problems, and an MXFP4 LLM engine
against a bf16 engine carrying the dequantised weights.

No bit-equality test against the bf16 / fp8 skinny kernels: the fp4 kernel's geometry differs from both (128-row
tiles, 128-wide K steps consumed whole by one wave in a permuted k order, no cross-wave reduction), so its fp32
sums are ordered differently and only the tolerances below apply."""
import pytest
import torch

from shai_amd import ops
from test_mxfp4_cpu import all_codes_case, group_scaled_weights

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


def _quantised(n, k, seed, cuda):
    """(wq, scales, dequantised fp32 [n, k]) on the GPU; the dequantised reference is the CPU table decode."""
    wq, s = ops.quantize_mxfp4(group_scaled_weights(n, k, seed))
    wd = ops.dequant_mxfp4(wq, s, dtype=torch.float32)
    return wq.to(cuda), s.to(cuda), wd.to(cuda)


def test_dequant_kernel_is_the_table_decode(cuda):
    wq, s, want = all_codes_case()
    got = ops.dequant_mxfp4(wq.to(cuda), s.to(cuda))
    assert got.dtype == torch.bfloat16 and got.is_cuda
    torch.testing.assert_close(got.float().cpu(), want, atol=0, rtol=0)
    wq, s = ops.quantize_mxfp4(group_scaled_weights(256, 512, seed=4))
    got = ops.dequant_mxfp4(wq.to(cuda), s.to(cuda))
    torch.testing.assert_close(got.float().cpu(), ops.dequant_mxfp4(wq, s, dtype=torch.float32), atol=0, rtol=0)
    # the quantiser gives the same codes and scales on the GPU
    wq_g, s_g = ops.quantize_mxfp4(group_scaled_weights(256, 512, seed=4, device=cuda))
    assert torch.equal(wq_g.view(torch.uint8).cpu(), wq.view(torch.uint8))
    assert torch.equal(s_g.view(torch.uint8).cpu(), s.view(torch.uint8))


@pytest.mark.parametrize("M,N,K", [(1, 128, 256), (5, 96, 64), (33, 320, 2048), (64, 4096, 4096)])
def test_fp4_skinny_plain_bias_residual(cuda, M, N, K):
    torch.manual_seed(M + N)
    wq, s, wd = _quantised(N, K, M + N, cuda)
    x = torch.randn(M, K, device=cuda).bfloat16()
    b = torch.randn(N, device=cuda).bfloat16()
    r = torch.randn(M, N, device=cuda).bfloat16()
    y = ops.linear(x, wq, b, residual=r, w_scale=s)
    want = x.float() @ wd.t() + b.float() + r.float()
    rel = _rel(y, want)
    print("plain", (M, N, K), "rel", rel)
    assert rel < 1e-2


@pytest.fixture(scope="module")
def glu_weights(cuda):
    return _quantised(2 * 1792, 4096, 11, cuda)


@pytest.mark.parametrize("M", [1, 17, 64])
def test_fp4_skinny_glu_rms(cuda, glu_weights, M):
    """SwiGLU gate/up (interleaved rows) with the RMSNorm folded in, as in Mistral decode."""
    torch.manual_seed(M)
    wq, s, wd = glu_weights
    x = torch.randn(M, 4096, device=cuda).bfloat16() * 3
    y = ops.linear(x, wq, act="silu", glu=True, rms_eps=1e-5, w_scale=s)
    xf = x.float()
    h = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)) @ wd.t()
    rel = _rel(y, h[:, 0::2] * torch.nn.functional.silu(h[:, 1::2]))
    print("glu+rms M", M, "rel", rel)
    assert rel < 2e-2


def test_fp4_skinny_forced_configs(cuda):
    """No split (1001), split-K with the separate fold (1004) and with the in-launch fixup (1104); GLU + RMS,
    K = 2112 = 16.5 steps of 128 (33 of 64): K groups of 5, 5, 5 and 2 steps, the last step half filled."""
    torch.manual_seed(7)
    M, K, N = 48, 2112, 2 * 1024
    wq, s, wd = _quantised(N, K, 7, cuda)
    x = torch.randn(M, K, device=cuda).bfloat16() * 3
    xf = x.float()
    h = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)) @ wd.t()
    want = h[:, 0::2] * torch.nn.functional.silu(h[:, 1::2])
    outs = {}
    for cfg in (1001, 1004, 1104):
        out = torch.empty(M, N // 2, device=cuda, dtype=torch.bfloat16)
        ops.gemm_into(x, wq, out, act="silu", glu=True, rms_eps=1e-5, w_scale=s, force_cfg=cfg)
        outs[cfg] = out
        rel = _rel(out, want)
        print("forced", cfg, "rel", rel)
        assert rel < 2e-2, cfg
    for a, b in ((1001, 1004), (1001, 1104), (1004, 1104)):
        rel = _rel(outs[a], outs[b])
        print("forced", a, "vs", b, "rel", rel)
        assert rel < 1e-3, (a, b)


def test_fp4_prefill_route_dequantises(cuda):
    torch.manual_seed(3)
    wq, s, wd = _quantised(512, 1024, 3, cuda)
    x = torch.randn(300, 1024, device=cuda).bfloat16()
    y = ops.linear(x, wq, w_scale=s)
    rel = _rel(y, x.float() @ wd.t())
    print("prefill route rel", rel)
    assert rel < 1e-2


def _run_engine(eng, prompts, n_dec, forced=None):
    """tests/tp_worker.py's pattern: greedy generation recording every step's logits (prefill, then n_dec - 1 decode
    steps); ``forced`` replaces each step's appended tokens, so both engines see the same sequences."""
    from shai_amd.engines.llm import SamplingParams
    rec = []
    fwd = eng.model.forward
    eng.model.forward = lambda *a, **k: (lambda y: (rec.append(y.float().clone()), y)[1])(fwd(*a, **k))
    p = SamplingParams(max_tokens=n_dec, temperature=0.0, ignore_eos=True)
    seqs = [eng.add_request(pr, p) for pr in prompts]
    row = {id(s): i for i, s in enumerate(seqs)}
    if forced is not None:
        app = eng._append
        eng._append = lambda ss, toks: app(ss, [forced[row[id(q)]][len(q.output)] for q in ss])
    while not all(q.finished for q in seqs):
        eng.step()
    return rec, [q.output for q in seqs]


def test_mxfp4_llm_engine(cuda):
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    from shai_amd.parallel.layers import FP8_LAYER_TYPES
    c = LlamaConfig.tiny()
    kw = dict(device=cuda, max_num_seqs=4, max_model_len=256, seed=1, enable_prefix_caching=False)
    prompts = [[3, 17, 99, 250, 7], [5, 6, 7, 8, 9, 10, 11]]
    n_dec = 8   # prefill + 7 decode steps
    # every step's logits are visible to Python only without graph replay / look-ahead: the logit comparison runs
    # eagerly, the default engine (HIP-graph decode, async look-ahead) is checked on its tokens below
    e4 = LLMEngine(c, quantization="mxfp4", use_graphs=False, async_decode=False, **kw)
    gu = e4.model.layers[0].mlp.gate_up_proj
    assert gu.weight.dtype != torch.bfloat16 and gu.weight.dtype == torch.float4_e2m1fn_x2
    assert gu.weight.numel() * gu.weight.element_size() == 2 * c.intermediate_size * c.hidden_size // 2
    assert e4.model.embed_tokens.weight.dtype == torch.bfloat16 and e4.model.lm_head.weight.dtype == torch.bfloat16
    e16 = LLMEngine(c, use_graphs=False, async_decode=False, **kw)
    q = {n: m for n, m in e4.model.named_modules() if isinstance(m, FP8_LAYER_TYPES)}
    for n, m in e16.model.named_modules():
        if isinstance(m, FP8_LAYER_TYPES):
            m.weight.data.copy_(ops.dequant_mxfp4(q[n].weight, q[n].w_scale))
    ref_logits, ref_toks = _run_engine(e16, prompts, n_dec)
    got_logits, got_toks = _run_engine(e4, prompts, n_dec, forced=ref_toks)
    assert got_toks == ref_toks and len(got_logits) == len(ref_logits) == n_dec
    for i, (g, r) in enumerate(zip(got_logits, ref_logits)):
        assert g.shape == r.shape
        rel = _rel(g, r)
        print("engine step", i, "logits rel", rel)
        assert rel < 3e-2, i
    # defaults: HIP-graph decode and async look-ahead.  Free-running greedy tokens follow the reference's; a step may
    # differ only where the reference's own margin between the two tokens is inside the logit tolerance above
    # (2 x 3e-2 of the row's largest logit), and the comparison ends there (the sequences differ from then on).
    ed = LLMEngine(c, quantization="mxfp4", **kw)
    assert ed.use_graphs and ed.async_decode
    out = [s.output for s in ed.generate(prompts, SamplingParams(max_tokens=n_dec, temperature=0.0, ignore_eos=True))]
    assert all(len(o) == n_dec and all(0 <= t < c.vocab_size for t in o) for o in out)
    for b, (o, want) in enumerate(zip(out, ref_toks)):
        for t in range(n_dec):
            if o[t] == want[t]:
                continue
            rowl = ref_logits[t][b]   # [B, V] logits of each sequence's last token
            margin = (rowl[want[t]] - rowl[o[t]]).item()
            assert margin <= 2 * 3e-2 * rowl.abs().max().item(), (b, t, o, want, margin)
            break


def test_fp4_skinny_fixup_deterministic_graph_and_streams(cuda):
    """The in-launch fixup of the fp4 skinny kernel (forced 1104): M = 33, N = 320 (2.5 tiles), K = 2112 (16.5 steps:
    K groups of 5, 5, 5 and 2), GLU + folded RMSNorm -- eager runs, graph replays and two streams at once are
    bitwise equal."""
    from test_skinny_gpu import check_fixup_repeatable
    torch.manual_seed(11)
    M, N, K = 33, 320, 2112
    wq, s, _ = _quantised(N, K, 11, cuda)
    x = (torch.randn(M, K, device=cuda) * 2).bfloat16()
    check_fixup_repeatable(
        lambda out: ops.gemm_into(x, wq, out, act="silu", glu=True, rms_eps=1e-5, w_scale=s, force_cfg=1104),
        (M, N // 2), cuda)

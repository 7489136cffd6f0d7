"""The sparse-MoE kernels (csrc/kernels/moe.hip) against fp64 models written here, on integer operands whose partial
sums stay below 2^24 (so fp32 accumulation is exact and the rounding points of the contract can be held exactly), and
the tiny Mixtral-shaped engine across its four decode variants."""
import pytest
import torch

import gemm_exact as ge
from shai_amd import ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# (M, H, I, E, k, routing, forced tile rows).  The 32-row tile: one row / a short tile / full tiles / one past a tile /
# several tiles of one expert, a single N tile and an N-tile tail with a K that is no power of two, balanced and skewed
# (every row to experts 2 and 5) routings.  Then k = 1 and E = 16 at the host's tile choice, and the 128-row tile: a
# short tile, one row past a tile, several tiles
CASES = [(M, H, I, 8, 2, r, 32) for M in (1, 5, 64, 65, 200) for H, I in ((128, 64), (192, 320))
         for r in ("balanced", "skewed")]
CASES += [(65, 192, 320, 8, 1, "balanced", None), (65, 192, 320, 16, 2, "balanced", None),
          (5, 128, 64, 8, 2, "balanced", 128), (129, 128, 64, 8, 2, "skewed", 128),
          (200, 192, 320, 8, 2, "skewed", 128), (200, 192, 320, 8, 2, "balanced", 128)]


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _ids(g, M, E, k, routing):
    if routing == "skewed":
        return torch.tensor([[2, 5][:k]] * M, dtype=torch.int32)
    return torch.rand(M, E, generator=g).topk(k, dim=1).indices.to(torch.int32)


def _nan_unrouted(w, ids):
    """NaN in every expert no row is routed to: an empty expert must never be read into a result."""
    w = w.clone()
    for e in set(range(w.shape[0])) - set(ids.reshape(-1).tolist()):
        w[e] = float("nan")
    return w


def _route64(x, wg, k, eps):
    rstd = torch.rsqrt((x * x).mean(1) + eps) if eps is not None else torch.ones(x.shape[0], dtype=torch.float64)
    logits = (x @ wg.t()) * rstd[:, None]
    order = torch.sort(-logits, dim=1, stable=True).indices[:, :k]   # a tie goes to the lower expert index
    top = logits.gather(1, order)
    w = torch.exp(top - top[:, :1])
    return order.to(torch.int32), w / w.sum(1, keepdim=True), rstd


@pytest.mark.parametrize("M,H,E,k", [(1, 128, 8, 2), (5, 192, 8, 2), (65, 192, 8, 1), (200, 128, 16, 2)])
def test_route(cuda, M, H, E, k):
    g = torch.Generator().manual_seed(M)
    x, wg = _ints(g, -3, 3, M, H), _ints(g, -2, 2, E, H)
    wg[3] = wg[1]
    wg[5] = wg[1]        # experts 1, 3 and 5 tie in every row
    if M > 1:
        x[1] = 0         # and a row whose logits all tie
    for eps in (None, 1e-5):
        ids64, w64, rstd64 = _route64(x, wg, k, eps)
        ids, w, rstd = ops.moe_route(x.to(BF16).to(cuda), wg.float().to(cuda), k, eps)
        assert torch.equal(ids.cpu(), ids64)
        torch.testing.assert_close(w.cpu().double(), w64, rtol=1e-5, atol=0)
        torch.testing.assert_close(rstd.cpu().double(), rstd64, rtol=1e-5, atol=0)


@pytest.mark.parametrize("M,H,I,E,k,routing,tile", CASES)
def test_glu_and_down_stages(cuda, M, H, I, E, k, routing, tile):
    g = torch.Generator().manual_seed(M * 7 + H)
    ids = _ids(g, M, E, k, routing)
    flat = ids.reshape(-1).long()
    rows = torch.arange(M * k) // k
    # ---- GLU stage: |h - h64| <= ulp_bf16(h64) + 1e-6 |z| on every real row, padding rows untouched
    x, w13 = _ints(g, -3, 3, M, H), _ints(g, -2, 2, E, 2 * I, H)
    rstd = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)[torch.randint(0, 3, (M,), generator=g)]
    z = torch.einsum("sh,snh->sn", x[rows], w13[flat]) * rstd[rows, None]
    h64, zabs = z[:, 0::2] * ge.act64(z[:, 1::2], "silu"), (z[:, 0::2] * z[:, 1::2]).abs()
    s_cap = ops.moe_experts_glu(x.to(BF16).to(cuda), w13.to(BF16).to(cuda), ids.to(cuda), tile_rows=tile)[0].shape[0]
    hbuf = torch.full((s_cap, I), float("nan"), dtype=BF16, device=cuda)
    h, plan = ops.moe_experts_glu(x.to(BF16).to(cuda), _nan_unrouted(w13, ids).to(BF16).to(cuda), ids.to(cuda),
                                  rstd.float().to(cuda), tile_rows=tile, h=hbuf)
    pos = plan.pos.reshape(-1).long().cpu()
    assert h.data_ptr() == hbuf.data_ptr() and len(set(pos.tolist())) == M * k and int(pos.min()) >= 0
    ge.assert_smooth(h.cpu()[pos], h64, zabs, "h")
    pad = torch.ones(s_cap, dtype=torch.bool)
    pad[pos] = False
    assert bool(h.cpu()[pad].isnan().all()), "a padding row of h was written"
    # ---- down stage, unsplit and forced split K: exact
    hs, w2, res = _ints(g, -4, 4, M * k, I), _ints(g, -2, 2, E, H, I), _ints(g, -9, 9, M, H)
    wts = torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64)[torch.randint(0, 3, (M, k), generator=g)]
    o = ge.to_bf16_exact(torch.einsum("si,sni->sn", hs, w2[flat]) * wts.reshape(-1, 1)).double().view(M, k, H)
    want = ge.to_bf16_exact(o.sum(1) + res)
    hbuf.fill_(float("nan"))
    hbuf[pos.to(cuda)] = hs.to(BF16).to(cuda)
    for splits in (1, 2):
        yslot = torch.full((splits, s_cap, H) if splits > 1 else (s_cap, H), float("nan"), device=cuda,
                           dtype=torch.float32 if splits > 1 else BF16)
        y = ops.moe_experts_down(hbuf, _nan_unrouted(w2, ids).to(BF16).to(cuda), plan, wts.float().to(cuda),
                                 res.to(BF16).to(cuda), splits=splits, yslot=yslot)
        ge.assert_exact(y.cpu(), want, f"y splits={splits}")


@pytest.mark.parametrize("M,H,I,E,k", [(1, 128, 64, 8, 2), (65, 192, 320, 8, 2), (200, 192, 320, 16, 2),
                                       (65, 128, 64, 8, 1)])
def test_moe_mlp_composed(cuda, M, H, I, E, k):
    g = torch.Generator().manual_seed(M + E)
    x, wg = _ints(g, -2, 2, M, H), _ints(g, -2, 2, E, H)
    x[:, 0] = 1
    wg[:, 0] = torch.arange(E).double() / 16     # logit_e = integer + e / 16: no two logits of a row tie
    w13, w2, res = _ints(g, -1, 1, E, 2 * I, H), _ints(g, -2, 2, E, H, I), _ints(g, -9, 9, M, H)
    ids64, w64, _ = _route64(x, wg, k, None)
    logits = torch.sort(x @ wg.t(), dim=1, descending=True).values
    assert bool((logits[:, :-1] > logits[:, 1:]).all())
    flat, rows = ids64.reshape(-1).long(), torch.arange(M * k) // k
    z = torch.einsum("sh,snh->sn", x[rows], w13[flat])
    h64 = z[:, 0::2] * ge.act64(z[:, 1::2], "silu")
    herr = ge.ulp_bf16(h64) + 1e-6 * (z[:, 0::2] * z[:, 1::2]).abs()
    o64 = (torch.einsum("si,sni->sn", h64, w2[flat]) * w64.reshape(-1, 1)).view(M, k, H)
    oerr = (torch.einsum("si,sni->sn", herr, w2[flat].abs()) * w64.reshape(-1, 1)).view(M, k, H).sum(1)
    y64 = o64.sum(1) + res
    largest = torch.maximum(torch.maximum(o64.abs().amax(1), res.abs()), y64.abs())
    dev = lambda t, dt=BF16: t.to(dt).to(cuda)
    ids, _, _ = ops.moe_route(dev(x), dev(wg, torch.float32), k)
    assert torch.equal(ids.cpu(), ids64)
    y = ops.moe_mlp(dev(x), dev(wg, torch.float32), dev(w13), dev(w2), k, residual=dev(res)).cpu().double()
    bad = ~((y - y64).abs() <= ge.ulp_bf16(y64) + oerr + (k + 1) * ge.ulp_bf16(largest))
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements outside the bound"


def test_moe_rejects_unsupported_shapes(cuda):
    x = torch.zeros(4, 96, dtype=BF16, device=cuda)
    with pytest.raises(ValueError):
        ops.moe_route(x, torch.zeros(8, 96, device=cuda), 2)            # H % 64
    with pytest.raises(ValueError):
        ops.moe_route(x[:, :64], torch.zeros(8, 64, device=cuda), 3)    # k
    with pytest.raises(ValueError):
        ops.moe_route(x[:, :64], torch.zeros(17, 64, device=cuda), 2)   # E


def test_tiny_moe_engine(cuda):
    """Greedy tokens identical across async / sync decode and graphs on / off; one prefill step's logits against the
    CPU engine on the same weights (rel < 3e-2, the engine-vs-CPU bound of tests/test_kv8_gpu.py)."""
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    c = LlamaConfig.tiny_moe()
    kw = dict(max_num_seqs=4, max_model_len=256, seed=2, enable_prefix_caching=False)
    prompts = [[3, 17, 99, 250, 7], [5, 6, 7], list(range(20, 90)), [9, 9]]
    p = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    outs, eng = [], None
    for graphs in (False, True):
        for async_decode in (False, True):
            eng = LLMEngine(c, device=cuda, use_graphs=graphs, async_decode=async_decode, **kw)
            outs.append([s.output for s in eng.generate(prompts, p)])
    assert all(o == outs[0] for o in outs[1:]) and all(len(o) == 8 for o in outs[0])
    cpu = LLMEngine(c, device="cpu", **kw)
    cpu.model.load_state_dict({k_: v.cpu() for k_, v in eng.model.state_dict().items()})
    cpu.model._folded = True   # the GPU engine's weights are already folded
    logits = []
    for e in (cpu, eng):
        fwd = e.model.forward
        e.model.forward = lambda *a, _f=fwd, **k_: (lambda y: (logits.append(y.float().cpu().clone()), y)[1])(_f(*a, **k_))
        e.generate(prompts[:2], SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True))
    rel = float((logits[1] - logits[0]).norm() / logits[0].norm())
    assert rel < 3e-2, rel

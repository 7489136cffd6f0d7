"""MXFP4 KV cache: writers / widener bit-equal to the oracle, decode attention under tests/attn_edges.py's rule."""
import math

import pytest
import torch

import attn_edges as ae
import shai_amd.ops as ops
from shai_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
POISON = 0xFF   # scale byte 0xff is the e8m0 NaN; as a code byte it is (-6, -6)
SLOTS = (0, 63, 64)   # first, last and next-block row of a sequence whose blocks are 2 and 1
CTX = [1, 63, 64, 65, 257]   # one row, a block edge, one past it, 5 blocks (two splits, ragged tail)


def _slots():
    return torch.tensor([(2, 1)[s // 64] * 64 + s % 64 for s in SLOTS] + [-1], dtype=torch.int32, device="cuda")


def _cache(nb, H, D):
    return torch.full((nb, H, 64, D // 2 + D // 32), POISON, dtype=torch.uint8, device="cuda")


def _rows(T, H, D):
    """bf16 rows with an all-zero group, a group whose amax is a power of two, and a value that saturates."""
    x = (torch.randn(T, H, D, device="cuda") * 3).bfloat16()
    x[:, 0, :32] = 0
    x[:, -1, 32:64] = x[:, -1, 32:64].clamp(-3.9, 3.9)
    x[:, -1, 40] = 4.0
    x[0, 0, 32:64] = x[0, 0, 32:64].clamp(-7, 7)
    x[0, 0, 33] = 7.5   # amax 7.5: scale 1, 7.5 -> 6
    return x


def _expect(cache, x, D):
    """The poisoned cache with the oracle's codes and scales of x [T, H, D] at SLOTS (block table 2, 1)."""
    want = cache.clone()
    codes, sb = ref.quantize_kv_mxfp4(x.cpu())
    pc, ps = ref.mxfp4_kv_planes(want)
    for t, s in enumerate(SLOTS):
        blk, row = (2, 1)[s // 64], s % 64
        pc[blk, :, row] = codes[t].cuda()
        ps[blk, :, row] = sb[t].cuda()
    return want


@pytest.mark.parametrize("D", [64, 128])
def test_kv_write_bit_exact(cuda, D):
    torch.manual_seed(2)
    k, v = _rows(4, 3, D), _rows(4, 3, D)
    kc, vc = _cache(4, 3, D), _cache(4, 3, D)
    wk, wv = _expect(kc, k[:3], D), _expect(vc, v[:3], D)
    ops.kv_write(k, v, kc, vc, _slots())
    assert torch.equal(kc, wk) and torch.equal(vc, wv)   # neighbouring rows keep the poison


@pytest.mark.parametrize("D,H,Hk", [(64, 4, 4), (128, 8, 2)])
def test_rope_qkv_cache_bit_exact(cuda, D, H, Hk):
    torch.manual_seed(3)
    T = 4
    qkv = torch.cat([_rows(T, H + Hk, D), _rows(T, Hk, D)], 1).reshape(T, -1).contiguous()
    ang = torch.rand(200, D // 2, device="cuda") * 3
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    pos = torch.tensor([0, 63, 64, 199], dtype=torch.int32, device="cuda")
    kc, vc = _cache(4, Hk, D), _cache(4, Hk, D)
    q_ref = qkv.cpu().clone()
    kr = q_ref[:, H * D:(H + Hk) * D].reshape(T, Hk, D).clone()
    ref.rope(q_ref[:, :H * D].view(T, H, D), pos.cpu(), cos.cpu(), sin.cpu(), D)
    ref.rope(kr, pos.cpu(), cos.cpu(), sin.cpu(), D)
    wk = _expect(kc, kr[:3].cuda(), D)
    wv = _expect(vc, qkv[:3, (H + Hk) * D:].reshape(3, Hk, D), D)
    ops.rope_qkv_cache(qkv, pos, cos, sin, kc, vc, _slots(), H, Hk)
    assert torch.equal(kc, wk) and torch.equal(vc, wv)
    assert torch.equal(qkv[:, :H * D].cpu(), q_ref[:, :H * D])


@pytest.mark.parametrize("D", [64, 128])
def test_kv_dequant_blocks_exact(cuda, D):
    torch.manual_seed(4)
    H = 3
    kc = torch.randint(0, 256, (5, H, 64, D // 2 + D // 32), dtype=torch.uint8, device="cuda")
    vc = torch.randint(0, 256, kc.shape, dtype=torch.uint8, device="cuda")
    for c in (kc, vc):   # scale bytes the writers produce (2 .. 252)
        ref.mxfp4_kv_planes(c)[1].clamp_(2, 252)
    phys = torch.tensor([4, 0, 3, 1], dtype=torch.int32, device="cuda")   # a permutation with a gap (2)
    ko = torch.full((5, H, 64, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    vo = ko.clone()
    ops.kv_dequant_blocks(kc, vc, phys, ko, vo)
    for out, c in ((ko, kc), (vo, vc)):
        assert torch.equal(out[:4].cpu(), ref.dequant_kv_mxfp4_blocks(c.cpu()[phys.cpu().long()], torch.bfloat16))
        assert out[4].isnan().all()


def _paged(B, Hkv, D, ctx, extra=0):
    """Caches: the oracle's codes of random rows inside each context, poison everywhere else; the fp32 values."""
    nblk = [(c + extra + 63) // 64 for c in ctx]
    nb = sum(nblk) + 3
    perm = torch.randperm(nb)[:sum(nblk)].int()
    bt = torch.zeros(B, max(nblk), dtype=torch.int32)
    caches, vals = [], []
    for _ in range(2):
        cache = torch.full((nb, Hkv, 64, D // 2 + D // 32), POISON, dtype=torch.uint8)
        pc, ps = ref.mxfp4_kv_planes(cache)
        per_seq, i = [], 0
        for b, c in enumerate(ctx):
            bt[b, :nblk[b]] = perm[i:i + nblk[b]]
            i += nblk[b]
            x = (torch.randn(c, Hkv, D) * 2).bfloat16()
            x[:, 0, :32] = 0
            codes, sb = ref.quantize_kv_mxfp4(x)
            for t in range(c):
                pc[bt[b, t // 64], :, t % 64] = codes[t]
                ps[bt[b, t // 64], :, t % 64] = sb[t]
            per_seq.append(ref.dequant_kv_mxfp4(codes, sb, torch.float32))
        caches.append(cache.cuda())
        vals.append(per_seq)
    return caches[0], caches[1], bt.cuda(), vals[0], vals[1]


def _check(o, q, kv, vv, D, what):
    for b in range(q.shape[0]):
        vis = torch.tensor([kv[b].shape[0]])
        o64, a = ae.attend64(q[b:b + 1].cpu(), kv[b], vv[b], vis, 1 / math.sqrt(D))
        ae.assert_edges_close(o[b:b + 1].cpu().float(), o64, a, what=f"{what} sequence {b}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 4, 8])
def test_decode_attn_mxfp4(cuda, D, G):
    torch.manual_seed(5)
    kc, vc, bt, kv, vv = _paged(len(CTX), 2, D, CTX)
    q = torch.randn(len(CTX), 2 * G, D, device="cuda").bfloat16()
    lens = torch.tensor(CTX, dtype=torch.int32, device="cuda")
    for splits in (1, 2):   # 257 tokens = 5 blocks: two splits of 3 and 2 blocks, the last one ragged
        o = ops.decode_attention(q, kc, vc, bt, lens, num_splits=splits)
        _check(o, q, kv, vv, D, f"splits {splits}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 4, 8])
def test_decode_attn_mxfp4_fused(cuda, D, G):
    """This step's token is stored as rope_qkv_cache stores it (bit for bit) and attended after that rounding."""
    torch.manual_seed(6)
    Hkv, B = 2, len(CTX)
    Hq = Hkv * G
    kc, vc, bt, _, _ = _paged(B, Hkv, D, [c - 1 for c in CTX], extra=1)
    lens = torch.tensor(CTX, dtype=torch.int32, device="cuda")
    pos = lens - 1
    slots = torch.stack([bt[b, (c - 1) // 64] * 64 + (c - 1) % 64 for b, c in enumerate(CTX)]).int()
    ang = torch.rand(max(CTX) + 1, D // 2, device="cuda") * 3
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    qkv = torch.cat([_rows(B, Hq + Hkv, D), _rows(B, Hkv, D)], 1).reshape(B, -1).contiguous()
    for splits in (1, 2):
        k2, v2, k3, v3, q2 = kc.clone(), vc.clone(), kc.clone(), vc.clone(), qkv.clone()
        o = ops.decode_attention_rope(qkv.clone(), k2, v2, bt, lens, pos, cos, sin, slots, Hq, Hkv, num_splits=splits)
        ops.rope_qkv_cache(q2, pos, cos, sin, k3, v3, slots, Hq, Hkv)
        assert torch.equal(k2, k3) and torch.equal(v2, v3) and not torch.equal(k2, kc)
        kv = [ref.gather_paged(k3.cpu(), bt[b].cpu(), c) for b, c in enumerate(CTX)]
        vv = [ref.gather_paged(v3.cpu(), bt[b].cpu(), c) for b, c in enumerate(CTX)]
        _check(o.view(B, Hq, D), q2[:, :Hq * D].reshape(B, Hq, D), kv, vv, D, f"fused splits {splits}")


def test_mxfp4_kv_llm_engine(cuda):
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    from test_kv8_gpu import _rel, _run_engine
    c = LlamaConfig.tiny()
    kw = dict(max_num_seqs=4, max_model_len=256, seed=1, enable_prefix_caching=False)
    prompts = [[3, 17, 99, 250, 7], list(range(5, 75))]
    eg = LLMEngine(c, device=cuda, kv_cache_dtype="mxfp4", use_graphs=False, async_decode=False, **kw)
    ec = LLMEngine(c, device="cpu", kv_cache_dtype="mxfp4", **kw)
    ec.model.load_state_dict({k: v.cpu() for k, v in eg.model.state_dict().items()})
    ec.model._folded = True
    assert eg.kv_buf.dtype == torch.uint8 and eg.kv_buf.shape[-1] == c.head_dim // 2 + c.head_dim // 32
    ref_logits, _ = _run_engine(ec, prompts, 1)
    got_logits, _ = _run_engine(eg, prompts, 1)
    rel = _rel(got_logits[0], ref_logits[0])
    print(f"mxfp4 KV: prefill GPU-vs-CPU logits rel {rel:.5f}")   # measured 0.0215
    assert rel < 3e-2
    p = SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)
    outs = []
    for graphs, async_ in ((False, False), (True, False), (True, True), (False, True)):
        e = LLMEngine(c, device=cuda, kv_cache_dtype="mxfp4", use_graphs=graphs, async_decode=async_, **kw)
        outs.append([s.output for s in e.generate(prompts, p)])
        assert e.bm.num_free == e.num_kv_blocks
    assert all(o == outs[0] for o in outs[1:]), outs
    big = dict(kw, gpu_memory_utilization=0.5, max_num_seqs=4096)
    b4, b8 = (LLMEngine(c, device=cuda, kv_cache_dtype=d, **big).kv_blocks_budget for d in ("mxfp4", "fp8"))
    assert b4 > b8

"""Case builders shared by the NF4 tests (tests/test_nf4_cpu.py, tests/test_nf4_gpu.py)."""
import torch

from shai_amd import ops


def nf4_case(n, k, seed, absmax=None):
    """Random codes [n, k] with a +-1 code (0 or 15) forced into every block, absmax [n, k / 64] (default: random fp32
    values that bf16 holds, so that max |w| of the bf16 matrix IS the absmax), and w = bf16(TABLE[c] * absmax)."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    blocks = codes.view(n, k // 64, 64)
    pos = torch.randint(0, 64, (n, k // 64, 1), generator=g)
    blocks.scatter_(2, pos, torch.randint(0, 2, (n, k // 64, 1), generator=g, dtype=torch.uint8) * 15)
    if absmax is None:
        absmax = (torch.rand(n, k // 64, generator=g) * 4 + 0.01).bfloat16().float()
    table = torch.tensor(ops.NF4_TABLE, dtype=torch.float32)
    w = (table[codes.long()].view(n, k // 64, 64) * absmax[..., None]).reshape(n, k).bfloat16()
    return codes, absmax, w


def random_packed(n, k, seed):
    """Random codes and random full-precision fp32 absmax (24 significant bits, never the maximum of bf16 numbers),
    packed: (wq, absmax, oracle-dequantised bf16 from the CPU table decode)."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    absmax = torch.rand(n, k // 64, generator=g) * 0.5 + 1e-3
    wq, am = ops.nf4_pack(codes, absmax)
    return wq, am, ops.dequant_nf4(wq, am)


def random_quantised(n, k, seed):
    """General weights (fp32 Gaussian, a scale per row, so the absmax are full-precision fp32 numbers) quantised on
    the CPU: (wq, absmax, oracle-dequantised bf16)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * (torch.rand(n, 1, generator=g) * 0.2 + 0.01)
    wq, am = ops.quantize_nf4(w)
    return wq, am, ops.dequant_nf4(wq, am)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-6)).item()


def run_engine(eng, prompts, n_dec, forced=None):
    """Greedy generation recording every step's logits (prefill, then n_dec - 1 decode steps); ``forced`` replaces
    each step's appended tokens, so two engines see the same sequences."""
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

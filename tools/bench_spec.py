#!/usr/bin/env python3
"""Speculative decoding on the GPU: the verify attention kernel against the two routes it replaces, and the engine
with speculation off and on at forced acceptance rates.

python tools/bench_spec.py [--kernel] [--engine mistral_7b|deepseek_r1_distill_70b|tiny] [--batch 1,8,64]
                           [--prompt-len 128] [--gen-len 128] [--json out.json]

Kernel rows (--kernel): ops.spec_attention's kernel (csrc/kernels/attention_spec.hip), the padded
ops.paged_attention and T calls of ops.decode_attention on the same q / cache / block table, each captured into a HIP
graph and replayed, the three variants alternating round by round in one process (median of the rounds).  Mistral
heads (32 / 8, D 128) at (B, ctx) = (1, 1k) (1, 16k) (1, 64k) (8, 1k) (64, 1k), 70B heads (64 / 8) at (1, 1k) (1, 16k),
T in {2, 4, 8}.

Engine rows (--engine): tokens/s of LLMEngine.generate with speculation off and with k = 4 at forced acceptance 0,
0.5 and 1.  Random weights do not repeat themselves, so n-gram hit rates on them say nothing: a first run with an
always-wrong proposer records the outputs, and a scripted proposer replays them with the drafts corrupted at fixed
positions (every draft / the third and fourth of each proposal / none).  The acceptance actually reached
(spec_accepted / spec_drafted) is printed beside the forced one.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import shai_amd.ops as ops
from tools.bench_kernels import graph_time


def engine_splits(B, hkv, ctx):
    """LLMEngine.decode_splits for a batch whose longest context is ctx (max_model_len = ctx)."""
    need = 1
    while need < 64 and need * 1024 < ctx:
        need *= 2
    return max(ops.decode_splits(B, hkv, ctx), min(need, max(1, (ctx + 63) // 64)))


def kernel_rows(rounds=5):
    rows = []
    shapes = [("mistral", 32, 8, B, ctx) for B, ctx in ((1, 1024), (1, 16384), (1, 65536), (8, 1024), (64, 1024))]
    shapes += [("70b", 64, 8, 1, 1024), ("70b", 64, 8, 1, 16384)]
    D = 128
    for name, Hq, Hkv, B, ctx in shapes:
        nb = (ctx + 63) // 64
        g = torch.Generator(device="cuda")
        g.manual_seed(0)
        kc = torch.randn(B * nb + 1, Hkv, 64, D, device="cuda", generator=g).to(torch.bfloat16)
        vc = torch.randn(B * nb + 1, Hkv, 64, D, device="cuda", generator=g).to(torch.bfloat16)
        bt = (torch.randperm(B * nb, device="cuda", generator=g).int() + 1).view(B, nb).contiguous()
        lens = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
        splits = engine_splits(B, Hkv, ctx)
        for T in (2, 4, 8):
            q = torch.randn(B, T, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
            ql = torch.full((B,), T, dtype=torch.int32, device="cuda")
            qt = [q[:, t].contiguous() for t in range(T)]
            lt = [lens - T + t + 1 for t in range(T)]
            o1 = torch.empty_like(q)
            o3 = torch.empty(B, Hq, D, dtype=q.dtype, device="cuda")

            def spec():
                ops.spec_attention(q, kc, vc, bt, lens, ql, num_splits=splits, out=o1)

            def padded():
                ops.paged_attention(q, kc, vc, bt, lens, ql)

            def decode_t():
                for t in range(T):
                    ops.decode_attention(qt[t], kc, vc, bt, lt[t], num_splits=splits, out=o3)

            assert ops.spec_attention_native(q, kc, vc)
            variants = {"spec": spec, "padded": padded, "decode_x_T": decode_t}
            times = {k: [] for k in variants}
            for _ in range(rounds):
                for k, fn in variants.items():
                    times[k].append(graph_time(fn, iters=8, reps=2))
            r = dict(op="spec_attention", heads=name, B=B, ctx=ctx, T=T, splits=splits,
                     **{k + "_us": round(statistics.median(v) * 1e6, 1) for k, v in times.items()})
            r["kv_GBps_spec"] = round(2 * B * ctx * Hkv * D * 2 / statistics.median(times["spec"]) / 1e9, 1)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del kc, vc
    return rows


class _Wrong:
    def __init__(self, vocab):
        self.vocab = vocab

    def propose(self, tokens, k):
        return [(tokens[-1] + 1 + i) % self.vocab for i in range(k)]


class _Replay:
    """Replays recorded outputs; drafts at proposal positions >= ``right`` are corrupted."""

    def __init__(self, prompts, outputs, right, vocab):
        self.by_len = {}
        for p, o in zip(prompts, outputs):
            self.by_len.setdefault((len(p), p[0], p[-1]), []).append((list(p), list(o)))
        self.right, self.vocab = right, vocab

    def propose(self, tokens, k):
        for (n, first, last), cands in self.by_len.items():
            if len(tokens) >= n and tokens[0] == first and tokens[n - 1] == last:
                for p, o in cands:
                    if tokens[:n] == p:
                        at = len(tokens) - n
                        d = o[at:at + k]
                        return [t if i < self.right else (t + 1) % self.vocab for i, t in enumerate(d)]
        return []


def engine_rows(model, batches, prompt_len, gen_len, k=4):
    import numpy as np
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    cfg = getattr(LlamaConfig, model)()
    rows = []
    # a seeded noise stream per position: the replayed runs redraw the recorded run's values
    params = SamplingParams(temperature=0.7, top_k=50, top_p=0.9, max_tokens=gen_len, ignore_eos=True, seed=1234)
    for B in batches:
        rng = np.random.default_rng(0)
        prompts = [rng.integers(10, cfg.vocab_size - 10, prompt_len).tolist() for _ in range(B)]
        recorded = None
        for label, spec, right in (("off", None, None), ("acc0", k, 0), ("acc0.5", k, k // 2), ("acc1", k, k)):
            eng = LLMEngine(cfg, device="cuda:0", max_num_seqs=B, max_model_len=prompt_len + gen_len + 64,
                            enable_prefix_caching=False,
                            speculative=None if spec is None else {"method": "ngram", "num_speculative_tokens": spec})
            if spec is not None:
                if right == 0 or recorded is None:
                    eng.proposer = _Wrong(cfg.vocab_size)
                else:
                    eng.proposer = _Replay(prompts, recorded, right, cfg.vocab_size)
            with torch.inference_mode():
                eng.generate(prompts, params)          # warm-up: graph capture, GEMM tuning
                base = dict(eng.stats)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = eng.generate(prompts, params)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            if spec is not None and right == 0:
                recorded = [list(s.output) for s in out]
            st = {x: eng.stats[x] - base[x] for x in eng.stats}
            r = dict(op="engine", model=model, B=B, prompt_len=prompt_len, gen_len=gen_len, spec=label,
                     tok_per_s=round(B * gen_len / dt, 1), steps=st["steps"])
            if spec is not None:
                r["accept"] = round(st["spec_accepted"] / max(1, st["spec_drafted"]), 3)
                r["tok_per_verify_step"] = round((B * gen_len - B) / max(1, st["spec_steps"]) / B, 2)
            print(json.dumps(r), flush=True)
            rows.append(r)
            del eng, out
            gc.collect()               # the engine and its captured graphs refer to each other
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--engine", default=None)
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--gen-len", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    if a.kernel:
        rows += kernel_rows(a.rounds)
    if a.engine:
        rows += engine_rows(a.engine, [int(x) for x in a.batch.split(",")], a.prompt_len, a.gen_len)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

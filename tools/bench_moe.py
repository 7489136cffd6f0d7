#!/usr/bin/env python3
"""Mixtral sparse-MoE measurements, one JSON line each.

(a) one Mixtral-shaped MoE layer (H 4096, I 14336, E 8, top-2) at M = 1, 16, 64, 256, 2048: ``ops.moe_mlp`` (route,
    align, the two grouped GEMMs, combine) against the per-expert loop over ``ops.linear`` with host-side gathers, the
    only way to compute the layer without the grouped kernels.  Times are device events around ``--iters`` calls after
    ``--warmup`` calls; ``weight_gbs`` is the bytes of the active experts' w13 and w2 over the layer time.
(b) with ``--engine``: a random-init ``mixtral_8x7b`` engine at batch 1 and 64, 128 + 128 tokens: TPOT, output
    tokens/s and the achieved weight bytes/s of the active experts per decode step.

python tools/bench_moe.py [--rows 1,16,64,256,2048] [--iters 20] [--warmup 5] [--engine] [--layers 32] [--sweep]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def expert_loop(ops, x, wg, w13, w2, k, eps):
    """The layer without the grouped kernels: route, then per active expert a host-side gather, two GEMMs, scatter."""
    import torch
    ids, wts, _ = ops.moe_route(x, wg, k, eps)
    y = x.float()
    for e in ids.unique().tolist():   # (device-to-host sync)
        m, j = (ids == e).nonzero(as_tuple=True)
        h = ops.linear(x[m], w13[e], glu=True, act="silu", rms_eps=eps)
        y.index_add_(0, m, ops.linear(h, w2[e]).float() * wts[m, j, None])
    return y.to(torch.bfloat16)


def layer_lines(a):
    import torch
    from shai_amd import ops
    H, I, E, k, eps = 4096, 14336, 8, 2, 1e-5
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s, std: (torch.randn(*s, generator=g, device="cuda") * std)
    wg = rnd(E, H, std=H ** -0.5)
    w13, w2 = rnd(E, 2 * I, H, std=H ** -0.5).bfloat16(), rnd(E, H, I, std=I ** -0.5).bfloat16()
    for M in [int(v) for v in a.rows.split(",")]:
        x = rnd(M, H, std=1.0).bfloat16()
        y = ops.moe_mlp(x, wg, w13, w2, k, eps, x)
        want = expert_loop(ops, x, wg, w13, w2, k, eps)
        rel = float((y.float() - want.float()).norm() / want.float().norm())
        active = int(ops.moe_route(x, wg, k, eps)[0].unique().numel())
        t = timed(lambda: ops.moe_mlp(x, wg, w13, w2, k, eps, x), a.warmup, a.iters)
        t0 = timed(lambda: expert_loop(ops, x, wg, w13, w2, k, eps), a.warmup, a.iters)
        wbytes = active * 3 * I * H * 2
        print(json.dumps({"bench": "moe_layer", "M": M, "H": H, "I": I, "E": E, "k": k, "active_experts": active,
                          "moe_mlp_us": round(t * 1e6, 1), "expert_loop_us": round(t0 * 1e6, 1),
                          "speedup": round(t0 / t, 2), "weight_gbs": round(wbytes / t / 1e9, 1),
                          "tflops": round(2 * M * k * 3 * I * H / t / 1e12, 1), "rel_vs_loop": round(rel, 5)}),
              flush=True)


def sweep_lines(a):
    """The two host choices, measured: the row-tile height (32 / 128) around the switch-over, and the K split of the
    down GEMM at small M."""
    import torch
    from shai_amd import ops
    H, I, E, k, eps = 4096, 14336, 8, 2, 1e-5
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s, std: (torch.randn(*s, generator=g, device="cuda") * std)
    wg = rnd(E, H, std=H ** -0.5)
    w13, w2 = rnd(E, 2 * I, H, std=H ** -0.5).bfloat16(), rnd(E, H, I, std=I ** -0.5).bfloat16()

    def layer(x, tile, splits):
        ids, wts, rstd = ops.moe_route(x, wg, k, eps)
        h, plan = ops.moe_experts_glu(x, w13, ids, rstd, tile_rows=tile)
        return ops.moe_experts_down(h, w2, plan, wts, x, splits=splits)
    xs = {}   # one activation per M: every variant of a row count sees the same routing
    for M, tile, splits in ([(M, t, None) for M in (16, 32, 64, 128, 256, 512, 1024) for t in (32, 128)] +
                            [(M, None, s) for M in (1, 2, 4, 8, 16) for s in (1, 2, 4, 8)]):
        x = xs.setdefault(M, rnd(M, H, std=1.0).bfloat16())
        t = timed(lambda: layer(x, tile, splits), a.warmup, a.iters)
        print(json.dumps({"bench": "moe_sweep", "M": M, "tile_rows": tile or "host", "down_splits": splits or "host",
                          "layer_us": round(t * 1e6, 1)}), flush=True)


def engine_lines(a):
    import numpy as np
    import torch
    from shai_amd.engines.llm import LLMEngine, SamplingParams
    from shai_amd.models.llama import LlamaConfig
    cfg = LlamaConfig.mixtral_8x7b()
    cfg.num_hidden_layers = a.layers
    P = G = 128
    eng = LLMEngine(cfg, device="cuda:0", max_num_seqs=64, max_model_len=P + G + 64, enable_prefix_caching=False)
    rng = np.random.default_rng(0)
    params = SamplingParams(temperature=0.7, top_k=50, top_p=0.9, max_tokens=G, ignore_eos=True)
    expert_bytes = 3 * cfg.intermediate_size * cfg.hidden_size * 2
    for B in (1, 64):
        prompts = lambda: [rng.integers(10, cfg.vocab_size - 10, P).tolist() for _ in range(B)]
        eng.generate(prompts(), params)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.generate(prompts(), params)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        tpot = float(np.median([(s.finish_time - s.first_token_time) / (len(s.output) - 1) for s in out]))
        active = min(cfg.num_local_experts, B * cfg.num_experts_per_tok)   # upper bound: distinct experts per layer
        print(json.dumps({"bench": "mixtral_8x7b_engine", "layers": a.layers, "batch": B, "prompt_len": P,
                          "gen_len": G, "tpot_ms": round(tpot * 1e3, 3), "tokens_per_s": round(B * G / el, 1),
                          "expert_weight_gbs_upper": round(a.layers * active * expert_bytes / tpot / 1e9, 1)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,16,64,256,2048")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--engine", action="store_true", help="also the mixtral_8x7b engine lines (93 GB of weights)")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--sweep", action="store_true", help="row-tile height and down-GEMM split sweeps instead")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe: needs a GPU (a CPU timing says nothing about the kernels)")
    with torch.inference_mode():
        if a.sweep:
            sweep_lines(a)
            return 0
        layer_lines(a)
        if a.engine:
            engine_lines(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())

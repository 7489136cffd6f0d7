#!/usr/bin/env python3
"""LLM decode with a bf16 and an fp8 (OCP e4m3fn) KV cache, crossed with bf16 and MXFP4 weights, one variant after
another in fresh child processes (each run owns the GPU and its own autotuner cache): ``bench_decode_throughput`` of
engines/llm.py per variant, one JSON line each, with the engine's block-pool size (num_kv_blocks, and
kv_blocks_budget: what the memory budget allows before the cap by what max_num_seqs can use) and KV bytes added.  A variant
is named ``<kv>+<weights>``: bf16+bf16, fp8+bf16, mxfp4+bf16, bf16+mxfp4, fp8+mxfp4, mxfp4+mxfp4 (kv mxfp4: the OCP
MXFP4 cache).  ``--attn`` instead times the paged decode attention alone over bf16, fp8 and mxfp4 caches in this one
process, the variants alternating round by round, and prints median and min - max per shape and cache.

python tools/bench_kv8.py [--llm-model mistral_7b] [--batch 256] [--prompt-len 1024] [--gen-len 64]
                          [--steps 1] [--warmup 1] [--variants bf16+bf16,fp8+bf16,bf16+mxfp4,fp8+mxfp4]
                          [--kv-prefill widen|native]   (the fp8 variants' prefill attention route)
python tools/bench_kv8.py --attn [--rounds 7]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("bf16+bf16", "fp8+bf16", "mxfp4+bf16", "bf16+mxfp4", "fp8+mxfp4", "mxfp4+mxfp4")
ATTN_SHAPES = ((64, 192), (64, 1024), (256, 1024), (1, 65536))   # (sequences, context tokens), Mistral-7B heads


def attn_table(rounds):
    """Decode attention (Hq 32, Hkv 8, D 128; the engine's split factor) per cache format: each round times every
    format once, 20 launches per timing, so drift lands on all formats alike; median and spread over the rounds."""
    sys.path.insert(0, ROOT)
    import torch
    from shai_amd import ops
    Hq, Hkv, D = 32, 8, 128
    for B, ctx in ATTN_SHAPES:
        nb = (ctx + 63) // 64
        bt = torch.randperm(B * nb, device="cuda").int().view(B, nb)
        lens = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
        q = torch.randn(B, Hq, D, device="cuda").bfloat16()
        x = torch.randn(B * nb, Hkv, 64, D, device="cuda").bfloat16()
        codes, sb = ops.quantize_kv_mxfp4(x)
        c4 = torch.cat([codes.flatten(2), sb.flatten(2)], 2).view(B * nb, Hkv, 64, D // 2 + D // 32).contiguous()
        caches = {"bf16": x, "fp8": ops.quantize_kv_fp8(x), "mxfp4": c4}
        splits = ops.decode_splits(B, Hkv, ctx)
        if ctx > 8192:
            splits = 64
        times = {k: [] for k in caches}
        for r in range(rounds + 1):
            for name, c in caches.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                for _ in range(20):
                    ops.decode_attention(q, c, c, bt, lens, num_splits=splits)
                ev[1].record()
                torch.cuda.synchronize()
                if r:   # round 0 warms up
                    times[name].append(ev[0].elapsed_time(ev[1]) * 50)   # us per launch
        for name, t in times.items():
            t.sort()
            print(json.dumps({"attn": f"{B}x{ctx}", "kv": name, "splits": splits, "us_median": round(t[len(t) // 2], 1),
                              "us_min": round(t[0], 1), "us_max": round(t[-1], 1)}), flush=True)


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from shai_amd.engines import llm
    seen = {}
    init = llm.LLMEngine.__init__

    def recording_init(self, *args, **kw):
        init(self, *args, **kw)
        seen.update(num_kv_blocks=int(self.num_kv_blocks), kv_blocks_budget=self.kv_blocks_budget,
                    kv_bytes=int(self.kv_bytes),
                    kv_scratch_bytes=int(self.kv_scratch_bytes), kv_dtype=str(self.kv_buf.dtype),
                    kv_prefill=self.kv_prefill)
    llm.LLMEngine.__init__ = recording_init
    kv, w = a.child.split("+")
    ns = argparse.Namespace(batch=a.batch, prompt_len=a.prompt_len, gen_len=a.gen_len, steps=a.steps,
                            warmup=a.warmup, tp=1, llm_model=a.llm_model, quantization=None if w == "bf16" else w,
                            kv_cache_dtype=kv, kv_prefill=a.kv_prefill if kv == "fp8" else None)
    with torch.inference_mode():
        r = llm.bench_decode_throughput(ns, 0, 1)
    r["variant"] = a.child
    if kv == "fp8":
        r["kv_prefill"] = seen.get("kv_prefill")
    r.update(seen)
    r["kv_gb"] = round(seen.get("kv_bytes", 0) / 1e9, 2)
    print("BENCH_KV8 " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--llm-model", default="mistral_7b",
                    choices=["mistral_7b", "llama3_8b", "deepseek_r1_distill_70b"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--prompt-len", type=int, default=1024)
    ap.add_argument("--gen-len", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--kv-prefill", default=None, choices=["widen", "native"],
                    help="prefill attention route of the fp8-cache variants (default: SHAI_KV8_PREFILL, else widen)")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per variant")
    ap.add_argument("--attn", action="store_true", help="time the decode attention alone over the three cache formats")
    ap.add_argument("--rounds", type=int, default=7, help="--attn: timed rounds per shape")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.attn:
        attn_table(a.rounds)
        return 0
    if a.child:
        child(a)
        return 0
    for v in a.variants.split(","):
        assert v in VARIANTS, v
        cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--llm-model", a.llm_model,
               "--batch", str(a.batch), "--prompt-len", str(a.prompt_len), "--gen-len", str(a.gen_len),
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
        if a.kv_prefill:
            cmd += ["--kv-prefill", a.kv_prefill]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"variant": v, "error": f"timed out after {a.timeout} s"}), flush=True)
            return 1   # nothing more is started on a GPU that may be hung
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("BENCH_KV8 ")]
        if p.returncode != 0 or not lines:
            print(json.dumps({"variant": v, "error": f"exit {p.returncode}", "tail": p.stdout[-2000:]}), flush=True)
            return 1   # a failed variant ends the run: nothing more is started on the GPU
        print(lines[-1][len("BENCH_KV8 "):], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

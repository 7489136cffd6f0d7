#!/usr/bin/env python3
"""LLM decode with bf16, fp8 and MXFP4 weights, one after another in fresh child processes (each run owns the GPU
and its own autotuner cache): ``bench_decode_throughput`` of engines/llm.py per variant, one JSON line each, with
the resident weight bytes of the engine added.  The variant ``mxfp4_dequant`` is mxfp4 with
``SHAI_MXFP4_PREFILL=dequant`` (problems of more than 64 rows dequantise the weights per call, the route before the fp4
tile GEMM): ``--variants mxfp4,mxfp4_dequant --repeats 3 --batch 128`` alternates the two and ends with one summary
line per variant (median and spread of output tokens/s, TPOT and TTFT over the repeats).

python tools/bench_mxfp4.py [--llm-model mistral_7b] [--batch 64] [--prompt-len 128] [--gen-len 128]
                            [--steps 2] [--warmup 1] [--variants bf16,fp8,mxfp4] [--repeats 1]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from shai_amd.engines import llm
    seen = {}
    init = llm.LLMEngine.__init__

    def recording_init(self, *args, **kw):
        init(self, *args, **kw)
        ts = list(self.model.parameters()) + list(self.model.buffers())
        seen["weight_bytes"] = int(sum(t.numel() * t.element_size() for t in ts))
    llm.LLMEngine.__init__ = recording_init
    ns = argparse.Namespace(batch=a.batch, prompt_len=a.prompt_len, gen_len=a.gen_len, steps=a.steps,
                            warmup=a.warmup, tp=1, llm_model=a.llm_model,
                            quantization={"bf16": None, "mxfp4_dequant": "mxfp4"}.get(a.child, a.child))
    with torch.inference_mode():
        r = llm.bench_decode_throughput(ns, 0, 1)
    r["variant"] = a.child
    r["weight_bytes"] = seen.get("weight_bytes")
    r["weight_gb"] = round(seen.get("weight_bytes", 0) / 1e9, 2)
    print("BENCH_MXFP4 " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--llm-model", default="mistral_7b",
                    choices=["mistral_7b", "llama3_8b", "deepseek_r1_distill_70b"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--gen-len", type=int, default=128)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variants", default="bf16,fp8,mxfp4")
    ap.add_argument("--repeats", type=int, default=1, help="runs per variant, the variants alternating")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per variant")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return 0
    rc = 0
    variants = a.variants.split(",")
    assert all(v in ("bf16", "fp8", "mxfp4", "mxfp4_dequant") for v in variants), variants
    results = {v: [] for v in variants}
    for v in [v for _ in range(max(1, a.repeats)) for v in variants]:
        env = dict(os.environ)
        if v == "mxfp4_dequant":
            env["SHAI_MXFP4_PREFILL"] = "dequant"
        elif v == "mxfp4":
            env.pop("SHAI_MXFP4_PREFILL", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--llm-model", a.llm_model,
               "--batch", str(a.batch), "--prompt-len", str(a.prompt_len), "--gen-len", str(a.gen_len),
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout,
                               env=env)
        except subprocess.TimeoutExpired:
            print(json.dumps({"variant": v, "error": f"timed out after {a.timeout} s"}), flush=True)
            return 1   # nothing more is started on a GPU that may be hung
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("BENCH_MXFP4 ")]
        if p.returncode != 0 or not lines:
            print(json.dumps({"variant": v, "error": f"exit {p.returncode}", "tail": p.stdout[-2000:]}), flush=True)
            return 1   # a failed variant ends the run: nothing more is started on the GPU
        print(lines[-1][len("BENCH_MXFP4 "):], flush=True)
        results[v].append(json.loads(lines[-1][len("BENCH_MXFP4 "):]))
    if a.repeats > 1:   # median and spread ((max - min) / median) of every numeric figure the runs share
        for v, rs in results.items():
            out = {"variant": v, "summary_of": len(rs)}
            for k in rs[0]:
                xs = sorted(r[k] for r in rs if isinstance(r.get(k), (int, float)) and not isinstance(r.get(k), bool))
                if len(xs) == len(rs) and k not in ("weight_bytes", "weight_gb") and xs[len(xs) // 2]:
                    out[k] = xs[len(xs) // 2]
                    out[k + "_spread_pct"] = round(100.0 * (xs[-1] - xs[0]) / abs(xs[len(xs) // 2]), 2)
            print("SUMMARY " + json.dumps(out), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())

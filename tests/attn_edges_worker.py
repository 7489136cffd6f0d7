"""Child process of tests/test_attn_edges_gpu.py::test_knob_only_kernels: the dense causal edge-probe cases at D = 64
(S 2200) and D = 128 (S 1100) under whichever routing knob the parent set in the environment (the knobs are read
once per process).  Exit status 0 = both cases met the strict rule."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import attn_edges as ae  # noqa: E402
import shai_amd.ops as ops  # noqa: E402


def main():
    knobs = {k: v for k, v in os.environ.items() if k in ("SHAI_FLASH64", "SHAI_FLASH64_DMA", "SHAI_FLASH_V1")}
    for name in ("knob_d64", "knob_d128"):
        c = ae.make(name, device="cuda")
        o = ops.attention(c.q, c.k, c.v, causal=c.causal, causal_offset=c.causal_offset, kv_lens=c.kv_lens,
                          q_lens=c.q_lens)
        torch.cuda.synchronize()
        worst = ae.check(c, o, what=f"{knobs} {name}")
        print(f"{knobs} {name}: worst |err| / bound {worst:.3f}", flush=True)


if __name__ == "__main__":
    main()

"""Attention kernels against the fp64 oracle on edge-probe inputs (tests/attn_edges.py): every probed query row's
last visible key dominates its softmax and the first masked key behind it is a stronger match carrying other
values, so a mask edge (kv_lens, the causal diagonal, causal_offset, a paged context's stale slots) that is off by one
key changes whole rows by ~8.  Every element is compared: |o - o64| <= C * a_abs + 1e-4, no share left out.  Each
case is the smallest shape that reaches its kernel (the routing of launch_flash_attn / launch_flash64 /
flash2_supported / launch_decode_attn in csrc/kernels)."""
import os
import subprocess
import sys

import pytest
import torch

import attn_edges as ae
import shai_amd.ops as ops

pytestmark = pytest.mark.gpu

_cases = {}


def case(name):
    """(case on the GPU, its oracle): built once per name and shared, never modified."""
    if name not in _cases:
        c = ae.make(name, device="cuda")
        _cases[name] = (c, ae.oracle(c))
    return _cases[name]


def run_dense(name, what):
    c, ref = case(name)
    o = ops.attention(c.q, c.k, c.v, causal=c.causal, causal_offset=c.causal_offset, kv_lens=c.kv_lens,
                      q_lens=c.q_lens, bias=c.bias, q_batch_mod=c.q_batch_mod)
    worst = ae.check(c, o, ref, what=f"{what} {name}")
    print(f"{what} {name}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("name", ["v1_d128", "v1_d128_causal", "v1_d128_causal_qlens"])
def test_v1_d128(cuda, name):
    """flash_fwd_kernel<128> (v1): D = 128 with Sq, Skv < 512 is below flash2's and flash128x2's range.  B 2, S 333,
    GQA 4:1, kv_lens [333, 65] (a full range ending at the buffer's poison rows; one key into the second tile),
    non-causal, causal, and causal with q_lens [200, 40] (offsets 133 / 25)."""
    run_dense(name, "v1<128>")


def test_v1_d64_bias(cuda):
    """flash_fwd_kernel<64> (v1): an additive bias is the only dense way to it at D = 64 (flash64 takes none).
    B 2, S 150, kv_lens [150, 77], a zero-mean bias of scale 0.5 (the probe still dominates)."""
    run_dense("v1_d64_bias", "v1<64> + bias")


@pytest.mark.parametrize("name", ["f64dma", "f64dma_causal", "f64dma_cross"])
def test_flash64_dma(cuda, name):
    """flash64_dma_kernel: D = 64 without bias / paging, fewer than 1024 256-query workgroups (3 * 8 * 3 = 72; the
    cross shape also has Skv < 512).  S 700 GQA 4:1 with kv_lens [700, 600, 65], causal and not; Sq 600 x Skv 77 with
    kv_lens [77, 33]: a key tail inside the first 64-key tile."""
    run_dense(name, "flash64-DMA")


def test_flash64_dma_shared_queries(cuda):
    """flash64_dma_kernel with q_batch_mod = 1: both k / v batches attend with the one query batch, read in place
    (flash_q_mod_supported); kv_lens [700, 590] differ per batch."""
    run_dense("f64dma_shared_q", "flash64-DMA shared q")


@pytest.mark.parametrize("name", ["f64x2", "f64x2_causal"])
def test_flash64_x2(cuda, name):
    """flash64x2_kernel: ceil(1100 / 256) * 32 heads * 8 batches = 1280 >= 1024 workgroups and Skv >= 512.  kv_lens
    as test_flash64_x2_large_grid ([1100, 1090, 1024, 777, 300, 1100, 65, 1000]), causal (q_lens = kv_lens) and
    not."""
    run_dense(name, "flash64x2")


D128_LONG = ["f128", "f128_causal", "f128_chunk"]


@pytest.mark.parametrize("name", D128_LONG)
def test_flash2_d128(cuda, name):
    """flash2_kernel<128>: D = 128, Sq and Skv >= 512, the default (set_flash128x2(0)).  B 2, S 1100, GQA 2:1,
    kv_lens [1100, 1090], causal and not; Sq 600 x Skv 1500 with causal_offset 900: diagonal probes in the last
    query tile (keys 1412 .. 1499)."""
    K = ops._K()
    prev = K.set_flash128x2(0)
    try:
        run_dense(name, "flash2<128>")
    finally:
        K.set_flash128x2(prev)


@pytest.mark.parametrize("name", D128_LONG)
def test_flash128x2(cuda, name):
    """flash128x2_kernel (opt-in): the shapes of test_flash2_d128 under set_flash128x2(1)."""
    K = ops._K()
    prev = K.set_flash128x2(1)
    try:
        run_dense(name, "flash128x2")
    finally:
        K.set_flash128x2(prev)


@pytest.mark.parametrize("name", ["a512_1000", "a512_1024"])
def test_attn512(cuda, name):
    """attn512_kernel (D = 512, one head, no masks): S 1000 ends with an 8-key tail of a 32-key tile, S 1024 with a
    full tile; k / v are views of [B, S + 64] buffers, so the keys right behind S are poison rows in memory."""
    run_dense(name, "attn512")


def test_paged_prefill_padded(cuda):
    """flash_fwd_kernel<KvBf16<128>> (v1 body, paged K / V): (kv_len, q_len) = (64, 64) (65, 65) (128, 37)
    (300, 300) (129, 1) in one padded launch; the stale slots of each last block and the poison block behind every
    sequence's table entries hold stronger matches than the last valid key."""
    c, ref = case("paged_prefill")
    o = ops.paged_attention(c.q, c.kc, c.vc, c.bt, c.kv_lens, c.q_lens)
    print(f"paged prefill: worst |err| / bound {ae.check(c, o, ref, what='paged prefill'):.3f}")


def test_paged_prefill_packed_varlen(cuda):
    """The same kernel through paged_attn_varlen: the five sequences' query rows packed back to back."""
    c, ref = case("paged_prefill")
    q, q_start = ae.packed(c)
    o = ops.paged_attention_varlen(q, c.kc, c.vc, c.bt, c.kv_lens, c.q_lens, q_start, max(c.q_list))
    out = torch.zeros_like(c.q)
    for b, n in enumerate(c.q_list):
        out[b, :n] = o[int(q_start[b]):int(q_start[b]) + n]
    print(f"packed varlen prefill: worst |err| / bound {ae.check(c, out, ref, what='varlen prefill'):.3f}")


def run_decode(name, splits, wb, what):
    c, ref = case(name)
    prev = ops.set_decode_wb(wb)
    try:
        o = ops.decode_attention(c.q[:, 0].contiguous(), c.kc, c.vc, c.bt, c.kv_lens, num_splits=splits,
                                 k_scale=c.k_scale, v_scale=c.v_scale)
    finally:
        ops.set_decode_wb(prev)
    worst = ae.check(c, o[:, None], ref, what=f"{what} {name} splits {splits}")
    print(f"{what} {name} splits {splits}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("name", [n for n in ae.CASES if n.startswith("decode")])
def test_decode_split_kernel(cuda, name, splits):
    """decode_attn_kernel (the split kernel, bf16 and fp8 cache formats; set_decode_wb(0) keeps D 128 / GQA 4 / one
    split on it): contexts [1, 2, 63, 64, 65, 128, 129, 300, 1000], the last key is the probe, the slots behind the
    context and every unused table entry's block are poison; fp8 caches with k_scale 0.5 / v_scale 2."""
    run_decode(name, splits, 0, "decode split")


def test_decode_wave_per_block(cuda):
    """decode_attn_wb_kernel: D 128, GQA 4, one split, bf16 cache under set_decode_wb(1) -- the only launches it
    takes; the same contexts and poison."""
    run_decode("decode_d128_g4", 1, 1, "decode wave-per-block")


KNOBS = [("SHAI_FLASH64", "0"),        # D = 64 at Sq, Skv >= 2048: flash2_kernel<64>
         ("SHAI_FLASH64_DMA", "0"),    # D = 64: the register-staged flash64_kernel
         ("SHAI_FLASH_V1", "1")]       # flash_fwd_kernel (v1) at long rows, D = 64 and D = 128


def test_knob_only_kernels(cuda):
    """Kernels that only a once-per-process environment knob selects, each in a fresh child process
    (tests/attn_edges_worker.py: dense causal D = 64 S 2200 and D = 128 S 1100 probe cases), one after another; the
    first child that fails ends the test."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(root, "tests", "attn_edges_worker.py")
    for knob, value in KNOBS:
        env = dict(os.environ, **{knob: value})
        for other, _ in KNOBS:
            if other != knob:
                env.pop(other, None)
        r = subprocess.run([sys.executable, worker], env=env, cwd=root, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120)
        print(r.stdout.decode(errors="replace"))
        assert r.returncode == 0, f"{knob}={value}: exit {r.returncode}"

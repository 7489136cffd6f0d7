// Test-only operators (namespace `shai`): host-side probes of the kernels' *_supported checks, kept out of
// bindings.cpp.  Nothing here launches a kernel.
#include <torch/library.h>

#include <string>
#include <vector>

#include "kernels/launchers.h"

namespace {

// Tests: for every kernel family that does NOT implement a broadcast operand, "<family>=<a>,<b>" with a = its
// *_supported check on a problem it takes and b = the same check with the broadcast field set (GemmArgs::res_rows /
// AttnArgs::q_batch_mod).  Host checks only: the pointers are aligned placeholders, nothing is launched.
std::vector<std::string> broadcast_refusals() {
  alignas(16) static char buf[64];
  const shai::bf16_t* p = reinterpret_cast<const shai::bf16_t*>(buf);
  std::vector<std::string> out;
  const auto row = [&](const char* name, bool before, bool after) {
    out.push_back(std::string(name) + "=" + (before ? "1" : "0") + "," + (after ? "1" : "0"));
  };
  const auto both = [&](const char* name, shai::GemmArgs g, int res_rows, auto&& check) {
    const bool before = check(g);
    g.res_rows = res_rows;
    row(name, before, check(g));
  };
  shai::GemmArgs g{};  // plain GEMM with a residual, 512 x 320 x 192
  g.A = g.W = g.residual = p;
  g.C = reinterpret_cast<shai::bf16_t*>(buf);
  g.M = 512, g.N = 320, g.K = 192, g.lda = g.ldw = 192, g.ldc = g.ldr = 320, g.batch = 1;
  g.alpha = g.res_alpha = 1.f, g.rows_per_bias2d = g.rows_per_gate = 1;
  both("v2", g, 256, [](const shai::GemmArgs& a) { return shai::gemm2_cfg_supported(a, 2); });
  both("w4", g, 256, [](const shai::GemmArgs& a) { return shai::gemm_w4_supported(a); });
  both("f8", g, 256, [](const shai::GemmArgs& a) { return shai::gemm_f8_supported(a); });
  shai::GemmArgs f4 = g;  // MXFP4 weights: ldw in bytes
  f4.w_mx_scale = reinterpret_cast<const uint8_t*>(buf);
  f4.ldw = 96;
  both("fp4", f4, 256, [](const shai::GemmArgs& a) { return shai::gemm_fp4_supported(a); });
  shai::GemmArgs sk = g;  // decode-shaped
  sk.M = 64;
  both("skinny", sk, 32, [](const shai::GemmArgs& a) { return shai::skinny_supported(a); });
  both("skinny2", sk, 32, [](const shai::GemmArgs& a) { return shai::skinny2_supported(a); });
  f4.M = 64;
  both("skinny_fp4", f4, 32, [](const shai::GemmArgs& a) { return shai::skinny_fp4_supported(a); });
  shai::GemmArgs h = g;  // 3x3 conv, 2 images of 64 x 64 x 64 -> 320
  h.conv = 1, h.Nimg = 2, h.H = h.Wd = h.OH = h.OW = 64, h.Cin = h.Cin1 = 64, h.KH = h.KW = 3, h.stride = h.pad = 1;
  h.M = 2 * 64 * 64, h.K = 9 * 64, h.lda = h.ldw = h.K;
  both("halo", h, 4096, [](const shai::GemmArgs& a) { return shai::conv_halo_supported(a); });
  shai::AttnArgs t{};  // 4 x 4096 x 4096, D = 128 / 512 / 64 with a bias
  t.q = t.k = t.v = p;
  t.o = reinterpret_cast<shai::bf16_t*>(buf);
  t.B = 4, t.Sq = t.Skv = 4096, t.Hq = t.Hkv = 1, t.D = 128;
  t.q_ts = t.k_ts = t.v_ts = t.o_ts = 128, t.q_bs = t.k_bs = t.v_bs = t.o_bs = 4096L * 128;
  const auto attn = [&](const char* name, shai::AttnArgs a, auto&& check) {
    const bool before = check(a);
    a.q_batch_mod = 2;
    row(name, before, check(a));
  };
  attn("flash2", t, [](const shai::AttnArgs& a) { return shai::flash2_supported(a); });
  attn("flash128x2", t, [](const shai::AttnArgs& a) { return shai::flash128x2_supported(a); });
  shai::AttnArgs t5 = t;
  t5.D = 512, t5.q_ts = t5.k_ts = t5.v_ts = t5.o_ts = 512, t5.q_bs = t5.k_bs = t5.v_bs = t5.o_bs = 4096L * 512;
  attn("attn512", t5, [](const shai::AttnArgs& a) { return shai::attn512_supported(a); });
  // the v1 body (bias, paged or fp8 K/V) has no check of its own; flash_q_mod_supported is the gate in front of it:
  // true for shared queries the LDS-DMA kernels take, false once a bias routes the problem to v1
  shai::AttnArgs tb = t;
  tb.D = 64, tb.q_ts = tb.k_ts = tb.v_ts = tb.o_ts = 64, tb.q_batch_mod = 2;
  const bool dma = shai::flash_q_mod_supported(tb);
  tb.bias = p;
  row("v1", dma, shai::flash_q_mod_supported(tb));
  return out;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(shai, m) { m.def("broadcast_refusals() -> str[]", &broadcast_refusals); }

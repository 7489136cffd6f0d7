// flash_fwd_kernel, the v1 flash attention body (4 waves x 32 queries, register-staged K/V tiles, double-buffered
// XOR-swizzled LDS; see attention.hip's header), written once for both K/V storage formats: KvBf16 (dense or paged
// bf16 K/V, instantiated in attention.hip) and KvFp8 (the paged fp8 KV cache read directly, instantiated in
// attention_kv8.hip).  The format decides only how a tile is staged:
//  * bf16: a thread moves NST 16-byte chunks of 8 elements per operand, global -> registers -> LDS;
//  * fp8:  a thread loads NST 16-byte chunks of 16 codes per operand (half as many chunks and staging registers),
//    widens each once with v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (exact: every e4m3 value is a bf16 value) and
//    writes the two bf16 x 8 chunks to the swizzled positions the bf16 format fills.  The conversion sits at
//    staging -- once per tile and workgroup -- not between the fragment reads and the MFMAs, where each of the four
//    waves would widen the whole K tile again.  k_scale folds into the score scale, v_scale into the final
//    normalisation (Fmt::qk_scale / out_scale), so the LDS tiles hold the unscaled code values.
// Everything from the LDS tiles on is the same code.  Rows at or beyond kv_len are zero-filled in either format
// (never loaded: a never-written fp8 slot may hold a NaN code, and P = 0 times NaN would poison P.V).
#pragma once
#include "common.h"
#include "decode_common.h"
#include "launchers.h"

namespace shai {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s4v __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kRescaleThr = 8.f;   // flash_fwd deferred-max threshold (log2 units)

template <int D>
__device__ __forceinline__ int k_swz(int row, int ch) {
  if constexpr (D == 128) return row * 128 + ((ch ^ (row & 15)) << 3);
  else return row * 64 + ((ch ^ ((row >> 1) & 7)) << 3);
}
template <int D>
__device__ __forceinline__ int v_swz(int row, int ch) {
  if constexpr (D == 128) return row * 128 + ((ch ^ ((row & 3) << 2)) << 3);
  else return row * 64 + ((ch ^ (((row >> 1) & 1) << 2)) << 3);
}

// 8 fp8 codes (two words) -> 8 bf16, scale 1.0: exact
__device__ __forceinline__ uint4_ kv8_widen8(uint32_t w0, uint32_t w1) {
  uint4_ r;
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
  r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
  r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
  return r;
}

template <typename Fmt, int D>
__global__ void __launch_bounds__(256, 2) flash_fwd_kernel(const AttnArgs p) {
  typedef typename Fmt::E E;             // stored K/V element: bf16_t, or one fp8 code
  constexpr bool kFp8 = sizeof(E) == 1;  // paged only (no dense K/V, no bias): the bindings reject anything else
  constexpr int KT = 64;                 // keys per tile
  constexpr int EPC = Fmt::EPC;          // stored elements per 16-byte chunk
  constexpr int CPR = D / EPC;           // 16-byte chunks per stored row
  constexpr int NST = KT * CPR / 256;    // chunks per thread per operand
  constexpr int NS = D / 16;             // k-steps for QK^T
  constexpr int ND = D / 32;             // 32-wide d blocks of O
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  bf16_t* sK = smem;                     // [2][64*D]
  bf16_t* sV = smem + 2 * KT * D;        // [2][64*D]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int b = blockIdx.z, hq = blockIdx.y;
  const int hk = hq / (p.Hq / p.Hkv);
  const int q_len = p.q_lens ? p.q_lens[b] : p.Sq;
  const int kv_len = p.kv_lens ? p.kv_lens[b] : p.Skv;
  const int c_off = p.q_lens ? kv_len - q_len : p.causal_offset;
  if ((int)blockIdx.x * 128 >= q_len) return;
  const int q0 = blockIdx.x * 128;
  const int qi = q0 + wid * 32 + fr;  // this lane's query

  // ---- Q fragments (B operand of S^T = K Q^T): Q[qi][16 s + 8 fh .. +7]
  bf16x8 qf[NS];
  {
    const bf16_t* qp = p.q + (p.q_start ? (long)p.q_start[b] * p.q_ts : (long)b * p.q_bs) +
                        (long)min(qi, q_len - 1) * p.q_ts + (long)hq * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      uint4_ v = *reinterpret_cast<const uint4_*>(qp + 16 * s + 8 * fh);
      if (qi >= q_len) v = uint4_{0u, 0u, 0u, 0u};
      qf[s] = __builtin_bit_cast(bf16x8, v);
    }
  }

  // ---- number of key tiles this block needs
  int kv_end = kv_len;
  if (p.causal) kv_end = min(kv_end, q0 + 127 + c_off + 1);
  const int ntiles = kv_end > 0 ? (kv_end + KT - 1) / KT : 0;

  // (strides count stored elements: with an fp8 cache the 64-bit offsets below are bytes)
  const E* pk = reinterpret_cast<const E*>(p.k);
  const E* pv = reinterpret_cast<const E*>(p.v);
  const E* kbase = pk + (long)b * p.k_bs + (long)hk * D;
  const E* vbase = pv + (long)b * p.v_bs + (long)hk * D;

  uint4_ rk[NST], rv[NST];
  auto load_tile = [&](int t) {
    const int key0 = t * KT;
    const E* kb = kbase;
    const E* vb = vbase;
    long ts_k = p.k_ts, ts_v = p.v_ts;
    int kbase_row = key0;
    if (kFp8 || p.block_table) {
      const int phys = p.block_table[(long)b * p.max_blocks + t];
      kb = pk + (long)phys * p.kc_bs + (long)hk * p.kc_hs;
      vb = pv + (long)phys * p.kc_bs + (long)hk * p.kc_hs;
      ts_k = ts_v = D;
      kbase_row = 0;
    }
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int id = tid + 256 * i;
      const int row = id / CPR, ch = id % CPR;
      const bool ok = key0 + row < kv_len;
      rk[i] = ok ? *reinterpret_cast<const uint4_*>(kb + (long)(kbase_row + row) * ts_k + ch * EPC) : uint4_{0u, 0u, 0u, 0u};
      rv[i] = ok ? *reinterpret_cast<const uint4_*>(vb + (long)(kbase_row + row) * ts_v + ch * EPC) : uint4_{0u, 0u, 0u, 0u};
    }
  };
  auto store_tile = [&](int stage) {
    bf16_t* ks = sK + stage * KT * D;
    bf16_t* vs = sV + stage * KT * D;
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int id = tid + 256 * i;
      const int row = id / CPR, ch = id % CPR;
      if constexpr (kFp8) {  // 16 codes -> the bf16 chunks 2 ch and 2 ch + 1 of the row
        *reinterpret_cast<uint4_*>(ks + k_swz<D>(row, 2 * ch)) = kv8_widen8(rk[i][0], rk[i][1]);
        *reinterpret_cast<uint4_*>(ks + k_swz<D>(row, 2 * ch + 1)) = kv8_widen8(rk[i][2], rk[i][3]);
        *reinterpret_cast<uint4_*>(vs + v_swz<D>(row, 2 * ch)) = kv8_widen8(rv[i][0], rv[i][1]);
        *reinterpret_cast<uint4_*>(vs + v_swz<D>(row, 2 * ch + 1)) = kv8_widen8(rv[i][2], rv[i][3]);
      } else {
        *reinterpret_cast<uint4_*>(ks + k_swz<D>(row, ch)) = rk[i];
        *reinterpret_cast<uint4_*>(vs + v_swz<D>(row, ch)) = rv[i];
      }
    }
  };

  float16_ o[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float sl2 = Fmt::qk_scale(p) * kLog2e;
  const bf16_t* bias_row =
      (!kFp8 && p.bias) ? p.bias + ((long)hq * p.Sq + min(qi, q_len - 1)) * p.Skv : nullptr;

  if (ntiles > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();

  // lane roles for the transposed V reads
  const int g16 = lane >> 4, i16 = lane & 15;
  const int tq = i16 >> 2, tp = i16 & 3;

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) load_tile(t + 1);
    const bf16_t* ks = sK + cur * KT * D;
    const bf16_t* vs = sV + cur * KT * D;

    // ---- S^T = K Q^T for two 32-key blocks
    float16_ sacc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + k_swz<D>(kb * 32 + fr, 2 * s + fh));
        sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sacc[kb], 0, 0, 0);
      }
    }
    // ---- mask (+ bias), row max on raw scores, exp2 with the scale folded into one FMA
    const int key0 = t * KT;
    const bool need_mask = (key0 + KT > kv_len) || (p.causal && key0 + KT - 1 > q0 + c_off);
    float mloc = -INFINITY;
    if (bias_row) {  // T5 relative-position bias: additive in the natural-log domain
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
          sacc[kb][r] += (key < p.Skv ? bf2f(bias_row[key]) : 0.f) / p.scale;
        }
    }
    if (need_mask) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
          const bool bad = key >= kv_len || (p.causal && key > qi + c_off);
          sacc[kb][r] = bad ? -INFINITY : sacc[kb][r];
        }
    }
    {  // 4 independent max chains (a single chain is 32 dependent v_max on the critical path)
      float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) m4[r & 3] = fmaxf(m4[r & 3], sacc[kb][r]);
      mloc = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64)) * sl2;   // scale > 0: max commutes with scaling
    // Deferred max: keep the running max (and skip the O rescale) unless some row's max grew by more
    // than kRescaleThr (log2 units) -- P is then bounded by 2^kRescaleThr instead of 1, which the bf16 P /
    // fp32 O, l accumulators absorb; the decision precedes this tile's exponentials, so everything still at
    // the old max is rescaled exactly once.
    const float m_cand = fmaxf(m_run, mloc);
    const bool grew = __any(m_cand > m_run + kRescaleThr);
    const float m_keep = grew ? m_cand : m_run;
    const float m_use = m_keep == -INFINITY ? 0.f : m_keep;
    const float alpha = grew ? __builtin_amdgcn_exp2f(m_run - m_use) : 1.f;
    m_run = m_keep;
    float ls4[4] = {0.f, 0.f, 0.f, 0.f};  // independent partial row sums (ILP)
    bf16x8 pf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(sacc[kb][r], sl2, -m_use));
        sacc[kb][r] = e;
        ls4[r & 3] += e;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (__bf16)sacc[kb][8 * s + j];
        pf[kb][s] = v;
      }
    }
    const float lsum = (ls4[0] + ls4[1]) + (ls4[2] + ls4[3]);
    l_run = l_run * alpha + lsum;
    if (grew) {
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
    }

    // ---- O^T += V^T P^T
#pragma unroll
    for (int d = 0; d < ND; ++d) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int r0 = kb * 32 + 16 * s + 4 * fh + tq;
          const int col = d * 32 + 16 * (g16 & 1) + 4 * tp;
          const int ch = col >> 3, half = (col >> 2) & 1;
          const bf16_t* a0 = vs + v_swz<D>(r0, ch) + 4 * half;
          const bf16_t* a1 = vs + v_swz<D>(r0 + 8, ch) + 4 * half;
          const s4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a0));
          const s4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a1));
          short8 vv;
          vv[0] = t0[0]; vv[1] = t0[1]; vv[2] = t0[2]; vv[3] = t0[3];
          vv[4] = t1[0]; vv[5] = t1[1]; vv[6] = t1[2]; vv[7] = t1[3];
          o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vv), pf[kb][s], o[d], 0, 0, 0);
        }
      }
    }
    if (t + 1 < ntiles) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = (l_tot > 0.f ? 1.f / l_tot : 0.f) * Fmt::out_scale(p);
  if (qi < q_len) {
    bf16_t* op = p.o + (p.q_start ? (long)p.q_start[b] * p.o_ts : (long)b * p.o_bs) + (long)qi * p.o_ts +
                 (long)hq * D;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = d * 32 + 8 * g + 4 * fh;
        uint2_ w;
        w[0] = pack2(o[d][4 * g] * inv, o[d][4 * g + 1] * inv);
        w[1] = pack2(o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv);
        *reinterpret_cast<uint2_*>(op + dd) = w;
      }
    }
  }
}

}  // namespace shai

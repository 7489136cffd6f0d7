// FP8 (OCP e4m3fn) paged KV cache for gfx950: cache writers, the split decode attention over byte caches, and the
// block widener that lets the bf16 prefill kernels run over a bf16 scratch copy of the blocks a step needs.
//
// One rule for every writer (ops/reference.py quantize_kv_fp8 is the oracle):
//   code  = RNE fp8(clamp(float(x_bf16) * inv_scale, -448, 448))      inv_scale = 1 / scale, computed on the host
//   value = float(code) * scale
// x_bf16 is what the bf16 cache would have stored (for K: the roped value rounded to bf16).  The clamp is explicit
// f32 arithmetic: the conversion's own overflow result depends on a mode bit.
//
// Every e4m3 value is a bf16 value, so the decode kernel widens codes to bf16 pairs (v_cvt_scalef32_pk_bf16_fp8,
// scale 1: exact) and keeps the bf16 kernel's packed dot products.  The scalar scales cost nothing per element:
// k_scale multiplies the softmax scale, v_scale the final normalisation (or the split partial's o).
#include "common.h"
#include "decode_common.h"
#include "launchers.h"

#include <algorithm>
#include <cstdlib>

namespace shai {

typedef __attribute__((address_space(3))) void kv8_lds_void;
typedef __bf16 kv8_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 kv8_bf16x8 __attribute__((ext_vector_type(8)));
typedef float kv8_f32x2 __attribute__((ext_vector_type(2)));
#define KV8_PAIR(v, i) __builtin_shufflevector(v, v, 2 * (i), 2 * (i) + 1)

constexpr float kKv8Log2e = 1.4426950408889634f;

__device__ __forceinline__ float kv8_clamp(float x) { return fminf(fmaxf(x, -448.f), 448.f); }
// two values -> two codes in the low 16 bits (a in byte 0)
__device__ __forceinline__ uint32_t kv8_q2(float a, float b, float inv) {
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a * inv), kv8_clamp(b * inv), 0, false) & 0xffffu;
}
// four values -> four codes (a in byte 0)
__device__ __forceinline__ uint32_t kv8_q4(float a, float b, float c, float d, float inv) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a * inv), kv8_clamp(b * inv), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(c * inv), kv8_clamp(d * inv), w, true);
  return (uint32_t)w;
}
// 8 bf16 (one uint4) -> 8 codes (two words)
__device__ __forceinline__ uint2_ kv8_q8(const uint4_ v, float inv) {
  float f[8];
  unpack8(v, f);
  uint2_ r;
  r[0] = kv8_q4(f[0], f[1], f[2], f[3], inv);
  r[1] = kv8_q4(f[4], f[5], f[6], f[7], inv);
  return r;
}
// NeoX rotation of one (x0, x1) pair for K, each product and the sum rounded separately (the build contracts
// a * b - c * d into an FMA otherwise): the roped k then equals the fp32 reference's bit for bit, so the stored
// codes can be checked exactly.  The empty asm keeps the products opaque to the contraction.
__device__ __forceinline__ void kv8_rope_k(float x0, float x1, float c, float s, float& a, float& b) {
  float p0 = x0 * c, p1 = x1 * s, p2 = x1 * c, p3 = x0 * s;
  asm("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
  a = p0 - p1;
  b = p2 + p3;
}
// the two codes in the low 16 bits -> their values
__device__ __forceinline__ kv8_f32x2 kv8_dq2(uint32_t codes) {
  return __builtin_amdgcn_cvt_pk_f32_fp8((int)codes, false);
}

// ----------------------------------------------------------------------------
// Paged decode attention over an fp8 cache: the split kernel of attention.hip (same contract: grid over
// (sequence, KV head, split) items, G = Hq/Hkv waves, per-sequence split counts, persistent walk, fused RoPE /
// new-token form with q / k / v from the QKV rows or the skinny GEMM's split-K partials, the same partial format
// for decode_combine_kernel) with a byte cache:
//  * a block's K + V is 2 * 64 * D bytes = D / 8 one-KB wave DMA instructions (half the bf16 count) into a ring
//    slot of half the size;
//  * K rows are D bytes = CPR = D / 16 chunks of 16 codes.  The lane = key score loop reads one 16-byte chunk per
//    lane per step (ds_read_b128: lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32, each one
//    LDS cycle over 64 banks = 256 B).  Row r starts at byte r * D, so 256 / D rows share a 256-byte bank window;
//    the chunk XOR (r / (256 / D)) & (CPR - 1) gives the 16 lanes of every group 16 different 16-byte bank
//    quads (D = 128: the even lanes of a group have r >> 1 = {0,1,6,7,10..13} or {2,3,4,5,8,9,14,15}, all
//    different mod 8, and the odd lanes sit 128 B further; D = 64: the four lanes of each r & 3 class have
//    r >> 2 = {0,3,5,6} or {1,2,4,7}, all different mod 4).  The swizzle is applied on the source side of the
//    DMA, as in the bf16 kernel;
//  * V rows stay linear: lane = output dim pair reads 2 bytes per key (128 contiguous bytes per wave);
//  * rows past the context are zero-filled by the buffer range check (P = 0 times a never-written NaN code
//    would poison P.V).
// This step's token (fused form) is attended after the same rounding the cache applies: the codes wave 0 stores
// are widened again and those values enter the score and P.V.
template <int D, int NI>
__device__ __forceinline__ void decode_attn8_item(const DecodeAttnArgs& p, char* dsm, const int b, const int hk,
                                                  const int split) {
  constexpr int CPR = D / 16;                   // 16-byte chunks per K / V row
  constexpr int RPI = 1024 / D;                 // rows per 1-KB wave DMA instruction
  constexpr int RSH = D == 128 ? 1 : 2;         // log2 of the rows per 256-byte bank window
  constexpr int SLOT = 2 * 64 * D;              // bytes per ring slot (K then V)
  uint8_t* ring = reinterpret_cast<uint8_t*>(dsm);             // [2][K 64xD swizzled | V 64xD linear]
  bf16_t* sQb = reinterpret_cast<bf16_t*>(ring + 2 * SLOT);    // [8][D]
  float* sP = reinterpret_cast<float*>(sQb + 8 * D);           // [8][64]
  const uint8_t* kc8 = reinterpret_cast<const uint8_t*>(p.k_cache);
  const uint8_t* vc8 = reinterpret_cast<const uint8_t*>(p.v_cache);
  const int G = p.Hq / p.Hkv;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hq = hk * G + w;
  const bool fused = p.knew != nullptr;
  const int ctx = p.ctx_lens[b] - (fused ? 1 : 0);  // tokens read from the cache
  const int nblk = (ctx + 63) / 64;
  const int nsp = da_splits(nblk, p.num_splits);
  if (split >= nsp) return;
  const int per = (nblk + nsp - 1) / nsp;
  const int blk0 = split * per, blk1 = min(nblk, blk0 + per);

  // physical block ids of this split, 64 per lane-distributed chunk, read ahead of the ring's DMA issue
  const int* bt = p.block_table + (long)b * p.max_blocks;
  int chunk0 = blk0;
  int my_phys = (blk0 + lane < blk1) ? bt[blk0 + lane] : 0;
  auto phys_of = [&](int bi) {
    if (bi - chunk0 >= 64) {
      chunk0 += 64;
      my_phys = (chunk0 + lane < blk1) ? bt[chunk0 + lane] : 0;
    }
    return __builtin_amdgcn_readfirstlane(__shfl(my_phys, bi - chunk0, 64));
  };
  // wave w issues instructions j = w + G * t (t < NI) of the block's 2 * 64 * D / 1024 = NI * G
  auto stage = [&](int slot, int bi) {
    const int phys = phys_of(bi);
    const long base = ((long)phys * p.Hkv + hk) * 64 * D;
    const __amdgpu_buffer_rsrc_t rk =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(kc8 + base), (short)0, 64 * D, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(vc8 + base), (short)0, 64 * D, 0x00020000);
    uint8_t* dst = ring + slot * SLOT;
#pragma unroll
    for (int t = 0; t < NI; ++t) {
      const int j = w + G * t;
      const bool isv = j >= NI * G / 2;
      const int jj = isv ? j - NI * G / 2 : j;
      const int row = jj * RPI + lane / CPR;    // this lane's row and LDS chunk position
      const int pos = lane % CPR;
      const int ch = isv ? pos : (pos ^ ((row >> RSH) & (CPR - 1)));  // K: source-side XOR swizzle
      const uint32_t off = (bi * 64 + row < ctx) ? (uint32_t)(row * D + ch * 16) : 0x80000000u;
      SHAI_DASSERT_DMA(off, 64 * D, 0x80000000u);
      SHAI_DASSERT(jj * 1024 + 1024 <= 64 * D);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isv ? rv : rk, (kv8_lds_void*)(dst + (isv ? 64 * D : 0) + jj * 1024),
                                               16, off, 0, 0, 0);
    }
  };

  // first block's DMA before the q prologue: its HBM latency overlaps the q / RoPE-table loads
  if (blk0 < blk1) stage(0, blk0);
  const int rpos = fused ? p.positions[b] : 0;
  const bool new_tok = fused && split == nsp - 1 && p.slots[b] >= 0;
  // QKV fold fused in (as the bf16 kernel): element col of this row = bf16(sum of the kg partial slabs, in slab
  // order, x the folded RMSNorm scale); four slabs per round with every load issued before the first add
  const bool part = p.qkv_ws != nullptr;
  float pv[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (part) {
    const long pslab = (long)p.B * p.qkv_n;
    const int lq = lane & (D / 2 - 1), kcol = (p.Hq + hk) * D, vcol = (p.Hq + p.Hkv + hk) * D;
    const int col[6] = {hq * D + lq, hq * D + lq + D / 2, kcol + lq, kcol + lq + D / 2,
                        D == 128 ? vcol + 2 * lane : vcol + lane, D == 128 ? vcol + 2 * lane + 1 : vcol + lane};
    const float* row = p.qkv_ws + (long)b * p.qkv_n;
    const float* ssr = p.qkv_ws + (long)p.qkv_kg * pslab + b;
    for (int s0 = 0; s0 < p.qkv_kg; s0 += 4) {
      float t[4][7];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int sl = min(s0 + u, p.qkv_kg - 1);  // past the last slab: re-read it, dropped below
#pragma unroll
        for (int e = 0; e < 6; ++e) t[u][e] = row[(long)sl * pslab + col[e]];
        t[u][6] = ssr[(long)sl * p.B];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (s0 + u < p.qkv_kg) {
#pragma unroll
          for (int e = 0; e < 7; ++e) pv[e] += t[u][e];
        }
    }
    const float rstd = rsqrtf(pv[6] / p.qkv_k + p.qkv_eps);
#pragma unroll
    for (int e = 0; e < 6; ++e) pv[e] = bf2f(f2bf(pv[e] * rstd));
  }
  float kn0 = 0.f, kn1 = 0.f, kc0 = 0.f, ks0 = 0.f;
  uint32_t vn_pair = 0u;
  float vn_one = 0.f;
  if (new_tok) {
    const bf16_t* kn = p.knew + (long)b * p.new_bs + (long)hk * D;
    const bf16_t* vn = p.vnew + (long)b * p.new_bs + (long)hk * D;
    if (lane < D / 2) {
      kn0 = part ? pv[2] : bf2f(kn[lane]);
      kn1 = part ? pv[3] : bf2f(kn[lane + D / 2]);
      kc0 = p.rope_cos[(long)rpos * (D / 2) + lane];
      ks0 = p.rope_sin[(long)rpos * (D / 2) + lane];
    }
    if constexpr (D == 128) {
      vn_pair = part ? pack2(pv[4], pv[5]) : *reinterpret_cast<const uint32_t*>(vn + 2 * lane);
    } else {
      vn_one = part ? pv[4] : bf2f(vn[lane]);
    }
  }
  if (fused) {  // NeoX RoPE on q (f32 math, bf16 result: what rope_qkv_cache would have stored)
    const bf16_t* qs = p.q + (long)b * p.q_bs + (long)hq * D;
    const float* cp = p.rope_cos + (long)rpos * (D / 2);
    const float* sp = p.rope_sin + (long)rpos * (D / 2);
    for (int i = lane; i < D / 2; i += 64) {
      const float x0 = part ? pv[0] : bf2f(qs[i]);  // (i == lane: one pass)
      const float x1 = part ? pv[1] : bf2f(qs[i + D / 2]);
      const float c = cp[i], sn = sp[i];
      sQb[w * D + i] = f2bf(x0 * c - x1 * sn);
      sQb[w * D + i + D / 2] = f2bf(x1 * c + x0 * sn);
    }
  } else {
    for (int i = lane; i < D; i += 64) sQb[w * D + i] = p.q[(long)b * p.q_bs + (long)hq * D + i];
  }
  const float sl2 = p.scale * p.k_scale * kKv8Log2e;  // k_scale folded into the softmax scale
  float m_run = -INFINITY, l_run = 0.f;
  float o0 = 0.f, o1 = 0.f;  // D=128: this lane's d = 2 lane, 2 lane + 1; D=64: d = lane (in units of v_scale)
  // (no barrier here: each wave reads only its own sQb row; the loop's barrier publishes the ring)
  for (int bi = blk0, slot = 0; bi < blk1; ++bi, slot ^= 1) {
    if (bi + 1 < blk1) {
      stage(slot ^ 1, bi + 1);
#if SHAI_DEBUG
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");  // block bi landed, bi+1 in flight
#endif
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // raw barrier: __syncthreads' fence would drain the ring (vmcnt(0)) and serialise the prefetch
    __builtin_amdgcn_s_barrier();
    const uint8_t* sK = ring + slot * SLOT;
    const uint8_t* sV = sK + 64 * D;
    const int key = bi * 64 + lane;  // lane = key
    // QK^T: a 16-code chunk = 4 words; each word widens to two bf16 pairs for two packed dot products
    float sc0 = 0.f, sc1 = 0.f;
#pragma unroll
    for (int ch = 0; ch < CPR; ++ch) {
      const uint4_ kw =
          *reinterpret_cast<const uint4_*>(sK + lane * D + ((ch ^ ((lane >> RSH) & (CPR - 1))) << 4));
      const kv8_bf16x8 qa = __builtin_bit_cast(kv8_bf16x8, *reinterpret_cast<const uint4_*>(sQb + w * D + ch * 16));
      const kv8_bf16x8 qb =
          __builtin_bit_cast(kv8_bf16x8, *reinterpret_cast<const uint4_*>(sQb + w * D + ch * 16 + 8));
#define KV8_QK(word, qv, i)                                                                                        \
  sc0 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, false),             \
                                        KV8_PAIR(qv, i), sc0, false);                                             \
  sc1 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, true),              \
                                        KV8_PAIR(qv, (i) + 1), sc1, false)
      KV8_QK(kw[0], qa, 0);
      KV8_QK(kw[1], qa, 2);
      KV8_QK(kw[2], qb, 0);
      KV8_QK(kw[3], qb, 2);
#undef KV8_QK
    }
    float sc = (sc0 + sc1) * sl2;
    if (key >= ctx) sc = -INFINITY;
    const float mt = wave_max(sc);
    const float m_new = fmaxf(m_run, mt);
    const float alpha = exp2f(m_run - m_new);
    float e = key < ctx ? exp2f(sc - m_new) : 0.f;
    o0 *= alpha;
    o1 *= alpha;
    if constexpr (D == 128) {
      // P goes to LDS as bf16 and the denominator sums the same rounded values; P.V runs as packed bf16 dot
      // products over key pairs: v_perm gathers the codes (V[k][d], V[k+1][d]) of this lane's two dims into the
      // low / high half of one word, which widens to the two bf16 pairs
      const bf16_t eb = f2bf(e);
      e = bf2f(eb);
      l_run = l_run * alpha + wave_sum(e);
      m_run = m_new;
      bf16_t* sPb = reinterpret_cast<bf16_t*>(sP);
      sPb[w * 64 + lane] = eb;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's P row is written before it is read
      float a0 = 0.f, a1 = 0.f;
#pragma unroll 2
      for (int k = 0; k < 64; k += 8) {
        const kv8_bf16x8 pk = __builtin_bit_cast(kv8_bf16x8, *reinterpret_cast<const uint4_*>(sPb + w * 64 + k));
        auto pvf = [&](int u, kv8_bf16x2 pp, float& c0, float& c1) {
          const uint32_t va = *reinterpret_cast<const uint16_t*>(sV + (k + 2 * u) * D + 2 * lane);
          const uint32_t vb = *reinterpret_cast<const uint16_t*>(sV + (k + 2 * u + 1) * D + 2 * lane);
          // bytes (V[k][2l], V[k+1][2l], V[k][2l+1], V[k+1][2l+1])
          const uint32_t x = __builtin_amdgcn_perm(vb, va, 0x05010400u);
          c0 = __builtin_amdgcn_fdot2_f32_bf16(pp, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x, 1.0f, false), c0,
                                               false);
          c1 = __builtin_amdgcn_fdot2_f32_bf16(pp, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x, 1.0f, true), c1,
                                               false);
        };
        pvf(0, KV8_PAIR(pk, 0), o0, o1);
        pvf(1, KV8_PAIR(pk, 1), a0, a1);
        pvf(2, KV8_PAIR(pk, 2), o0, o1);
        pvf(3, KV8_PAIR(pk, 3), a0, a1);
      }
      o0 += a0;
      o1 += a1;
    } else {
      l_run = l_run * alpha + wave_sum(e);
      m_run = m_new;
      sP[w * 64 + lane] = e;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's sP row is written before it is read
#pragma unroll 4
      for (int k = 0; k < 64; k += 4) {
        const float4_ pk = *reinterpret_cast<const float4_*>(sP + w * 64 + k);
#pragma unroll
        for (int u = 0; u < 4; ++u) o0 += pk[u] * __builtin_amdgcn_cvt_f32_fp8((int)sV[(k + u) * D + lane], 0);
      }
    }
    __builtin_amdgcn_s_barrier();  // every wave is done with this slot before it is refilled (block bi+2)
  }
  if (new_tok) {
    // this step's token: roped k rounded to bf16 and then to its fp8 code, v to its code -- the values every
    // later reader of the cache will see -- as one more online-softmax key; wave 0 writes the codes into the
    // cache (no workgroup of this launch reads that row: the block DMA range-checks it out)
    const int slot_new = p.slots[b];
    uint32_t kq = 0u;
    float part_s = 0.f;
    if (lane < D / 2) {
      float ra, rb;
      kv8_rope_k(kn0, kn1, kc0, ks0, ra, rb);
      const float kr0 = bf2f(f2bf(ra)), kr1 = bf2f(f2bf(rb));
      kq = kv8_q2(kr0, kr1, p.k_inv);
      const kv8_f32x2 kd = kv8_dq2(kq);
      part_s = kd[0] * bf2f(sQb[w * D + lane]) + kd[1] * bf2f(sQb[w * D + lane + D / 2]);
    }
    const float sc = wave_sum(part_s) * sl2;
    const float m_new = fmaxf(m_run, sc);
    const float alpha = exp2f(m_run - m_new);
    float e = exp2f(sc - m_new);
    if constexpr (D == 128) e = bf2f(f2bf(e));  // P is bf16 on the cache path too
    l_run = l_run * alpha + e;
    m_run = m_new;
    uint32_t vq;
    if constexpr (D == 128) {
      vq = kv8_q2(bf2f(vn_pair & 0xffff), bf2f(vn_pair >> 16), p.v_inv);
      const kv8_f32x2 vd = kv8_dq2(vq);
      o0 = o0 * alpha + e * vd[0];
      o1 = o1 * alpha + e * vd[1];
    } else {
      vq = kv8_q2(vn_one, 0.f, p.v_inv);
      o0 = o0 * alpha + e * kv8_dq2(vq)[0];
    }
    if (w == 0) {
      const long dst = (((long)(slot_new >> 6) * p.Hkv + hk) * 64 + (slot_new & 63)) * D;
      uint8_t* kc = const_cast<uint8_t*>(kc8);
      uint8_t* vc = const_cast<uint8_t*>(vc8);
      if (lane < D / 2) {
        kc[dst + lane] = (uint8_t)(kq & 0xffu);
        kc[dst + lane + D / 2] = (uint8_t)(kq >> 8);
      }
      if constexpr (D == 128) *reinterpret_cast<uint16_t*>(vc + dst + 2 * lane) = (uint16_t)vq;
      else vc[dst + lane] = (uint8_t)(vq & 0xffu);
    }
  }
  if (nsp == 1) {  // one split: normalise (v_scale folded in) and write the output here (the combine skips this row)
    const float inv = l_run > 0.f ? p.v_scale / l_run : 0.f;
    bf16_t* op = p.o + (long)b * p.o_bs + (long)hq * D;
    if constexpr (D == 128) {
      *reinterpret_cast<uint32_t*>(op + 2 * lane) = pack2(o0 * inv, o1 * inv);
    } else {
      op[lane] = f2bf(o0 * inv);
    }
    return;
  }
  // partial results: ws[b][hq][split] = {m, l, o[D]}, o in true units (the combine knows no scale)
  float* dst = p.ws + (((long)b * p.Hq + hq) * p.num_splits + split) * (D + 2);
  if (lane == 0) {
    dst[0] = m_run;
    dst[1] = l_run;
  }
  if constexpr (D == 128) {
    dst[2 + 2 * lane] = o0 * p.v_scale;
    dst[3 + 2 * lane] = o1 * p.v_scale;
  } else {
    dst[2 + lane] = o0 * p.v_scale;
  }
}

// one workgroup per item, or the persistent walk of about two workgroups per CU (see decode_attn_kernel)
template <int D, int NI>
__global__ void __launch_bounds__(512) decode_attn8_kernel(const DecodeAttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  const int total = p.B * p.Hkv * p.num_splits;
  const int S = p.num_splits;
  const bool rotate = (int)gridDim.x < total;
  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    const int sidx = item % S, r = item / S;
    const int b = r / p.Hkv, hk = r - b * p.Hkv;
    const int split = rotate ? (sidx - b % S + S) % S : sidx;  // a sequence's splits rotated by b, as the bf16 kernel
    decode_attn8_item<D, NI>(p, dsm, b, hk, split);
    __syncthreads();  // the next item restages ring slot 0
  }
}

void launch_decode_attn_kv8(const DecodeAttnArgs& a, hipStream_t s) {
  const int G = a.Hq / a.Hkv;
  static const int width = [] {  // two workgroups per CU
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      cus = 256;
    return 2 * cus;
  }();
  static const int force = [] {  // SHAI_DECODE_PERSIST=0 / 1 forces either form (A/B), as for the bf16 kernel
    const char* e = getenv("SHAI_DECODE_PERSIST");
    return e ? (e[0] == '1' ? 1 : 0) : -1;
  }();
  const long items = (long)a.B * a.Hkv * a.num_splits;
  const bool persist = force >= 0 ? force == 1 : a.num_splits > 8;
  dim3 grid((unsigned)(persist ? std::min<long>(items, width) : items));
  const size_t lds = (size_t)4 * 64 * a.D + (size_t)8 * a.D * sizeof(bf16_t) + 8 * 64 * 4;
  // NI = wave DMA instructions per block per wave = (2 * 64 * D / 1024) / G
#define DA8(D_, NI_) decode_attn8_kernel<D_, NI_><<<grid, G * 64, lds, s>>>(a)
  if (a.D == 128) {
    switch (G) {
      case 1: DA8(128, 16); break;
      case 2: DA8(128, 8); break;
      case 4: DA8(128, 4); break;
      default: DA8(128, 2); break;  // G = 8
    }
  } else {
    switch (G) {
      case 1: DA8(64, 8); break;
      case 2: DA8(64, 4); break;
      case 4: DA8(64, 2); break;
      default: DA8(64, 1); break;
    }
  }
#undef DA8
  if (a.num_splits > 1) launch_decode_combine(a, s);
}

// ----------------------------------------------------------------------------
// Writers.  Cache layout [num_blocks, Hkv, 64, D] bytes; slot = block * 64 + offset; slot < 0 is skipped.
// ----------------------------------------------------------------------------
// one item = 16 elements of one (token, head): two 16-byte loads, one 16-byte store of 16 codes, for K and V
__global__ void kv_write_f8_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                   uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, const int* __restrict__ slots,
                                   int T, int Hkv, int D, long k_ts, long v_ts, float k_inv, float v_inv) {
  const int CPR = D / 16;
  const long total = (long)T * Hkv * CPR;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % CPR);
    const int h = (int)((i / CPR) % Hkv);
    const int t = (int)(i / ((long)CPR * Hkv));
    const int slot = slots[t];
    if (slot < 0) continue;
    const long dst = (((long)(slot >> 6) * Hkv + h) * 64 + (slot & 63)) * D + ch * 16;
    const bf16_t* ks = k + (long)t * k_ts + (long)h * D + ch * 16;
    const bf16_t* vs = v + (long)t * v_ts + (long)h * D + ch * 16;
    const uint2_ ka = kv8_q8(*reinterpret_cast<const uint4_*>(ks), k_inv);
    const uint2_ kb = kv8_q8(*reinterpret_cast<const uint4_*>(ks + 8), k_inv);
    const uint2_ va = kv8_q8(*reinterpret_cast<const uint4_*>(vs), v_inv);
    const uint2_ vb = kv8_q8(*reinterpret_cast<const uint4_*>(vs + 8), v_inv);
    *reinterpret_cast<uint4_*>(kc + dst) = uint4_{ka[0], ka[1], kb[0], kb[1]};
    *reinterpret_cast<uint4_*>(vc + dst) = uint4_{va[0], va[1], vb[0], vb[1]};
  }
}

void launch_kv_write_f8(const bf16_t* k, const bf16_t* v, uint8_t* k_cache, uint8_t* v_cache, const int* slot_mapping,
                        int T, int Hkv, int D, long k_ts, long v_ts, float k_inv, float v_inv, hipStream_t s) {
  const long total = (long)T * Hkv * (D / 16);
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  kv_write_f8_kernel<<<(int)blocks, 256, 0, s>>>(k, v, k_cache, v_cache, slot_mapping, T, Hkv, D, k_ts, v_ts, k_inv,
                                                 v_inv);
}

// rope_qkv_cache over an fp8 cache: q is roped in place as bf16; k is roped, rounded to bf16 (the value the bf16
// cache would hold) and quantised; v is quantised.  One item = 16 elements as in the bf16 kernel: for q / k heads
// 8 elements of each rotation half (two 8-byte stores of 8 codes), for v heads one 16-byte store of 16 codes.
__global__ void rope_qkv_cache_f8_kernel(bf16_t* __restrict__ qkv, long ld, const int* __restrict__ pos,
                                         const float* __restrict__ cs, const float* __restrict__ sn,
                                         uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                         const int* __restrict__ slots, int T, int H, int Hkv, int D, float k_inv,
                                         float v_inv) {
  const int half = D >> 1;
  const int per_head = D / 16;
  const int heads = H + 2 * Hkv;
  const long total = (long)T * heads * per_head;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const int t = (int)(i / ((long)per_head * heads));
    bf16_t* row = qkv + (long)t * ld;
    const int slot = slots[t];
    if (hh >= H + Hkv) {  // v head: 16 elements -> 16 codes
      if (slot < 0) continue;
      const int h = hh - H - Hkv;
      const bf16_t* src = row + (long)hh * D + c * 16;
      const long dst = (((long)(slot >> 6) * Hkv + h) * 64 + (slot & 63)) * D + c * 16;
      const uint2_ va = kv8_q8(*reinterpret_cast<const uint4_*>(src), v_inv);
      const uint2_ vb = kv8_q8(*reinterpret_cast<const uint4_*>(src + 8), v_inv);
      *reinterpret_cast<uint4_*>(vc + dst) = uint4_{va[0], va[1], vb[0], vb[1]};
      continue;
    }
    bf16_t* xh = row + (long)hh * D;
    const int p = pos[t];
    float a[8], b[8];
    unpack8(*reinterpret_cast<const uint4_*>(xh + 8 * c), a);
    unpack8(*reinterpret_cast<const uint4_*>(xh + half + 8 * c), b);
    const float* cp = cs + (long)p * half + 8 * c;
    const float* sp = sn + (long)p * half + 8 * c;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float co = cp[e], si = sp[e];
      const float x0 = a[e], x1 = b[e];
      if (hh < H) {  // q: the bf16 kernel's expression
        a[e] = x0 * co - x1 * si;
        b[e] = x1 * co + x0 * si;
      } else {
        kv8_rope_k(x0, x1, co, si, a[e], b[e]);
      }
    }
    const uint4_ ua = pack8(a), ub = pack8(b);
    if (hh < H) {
      *reinterpret_cast<uint4_*>(xh + 8 * c) = ua;
      *reinterpret_cast<uint4_*>(xh + half + 8 * c) = ub;
    } else if (slot >= 0) {
      const int h = hh - H;
      const long dst = (((long)(slot >> 6) * Hkv + h) * 64 + (slot & 63)) * D;
      *reinterpret_cast<uint2_*>(kc + dst + 8 * c) = kv8_q8(ua, k_inv);
      *reinterpret_cast<uint2_*>(kc + dst + half + 8 * c) = kv8_q8(ub, k_inv);
    }
  }
}

void launch_rope_qkv_cache_f8(bf16_t* qkv, long ld, const int* pos, const float* cos, const float* sin,
                              uint8_t* k_cache, uint8_t* v_cache, const int* slots, int T, int H, int Hkv, int D,
                              float k_inv, float v_inv, hipStream_t s) {
  const long total = (long)T * (H + 2 * Hkv) * (D / 16);
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  rope_qkv_cache_f8_kernel<<<(int)blocks, 256, 0, s>>>(qkv, ld, pos, cos, sin, k_cache, v_cache, slots, T, H, Hkv, D,
                                                       k_inv, v_inv);
}

// ----------------------------------------------------------------------------
// kv_dequant_blocks: scratch block i = bf16(float(code) * scale) of cache block phys[i], for K and V.  The bf16
// prefill kernels (paged flash attention, varlen) then run on the scratch with a block table remapped to 0 .. n-1.
// One item = 16 codes (one 16-byte load, two 16-byte stores); block_elems = Hkv * 64 * D (a multiple of 16).
// ----------------------------------------------------------------------------
__global__ void kv_dequant_blocks_kernel(const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                         const int* __restrict__ phys, int n, long block_elems,
                                         bf16_t* __restrict__ ko, bf16_t* __restrict__ vo, float k_scale,
                                         float v_scale) {
  const long per = block_elems / 16;
  const long total = 2 * (long)n * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const bool isv = i >= (long)n * per;
    const long r = isv ? i - (long)n * per : i;
    const int blk = (int)(r / per);
    const long e = (r - (long)blk * per) * 16;
    const uint8_t* src = (isv ? vc : kc) + (long)phys[blk] * block_elems + e;
    bf16_t* dst = (isv ? vo : ko) + (long)blk * block_elems + e;
    const float sc = isv ? v_scale : k_scale;
    const uint4_ w = *reinterpret_cast<const uint4_*>(src);
    uint4_ lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const kv8_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
      const kv8_f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
      const uint32_t p0 = pack2(a[0] * sc, a[1] * sc), p1 = pack2(b[0] * sc, b[1] * sc);
      if (j < 2) {
        lo[2 * j] = p0;
        lo[2 * j + 1] = p1;
      } else {
        hi[2 * (j - 2)] = p0;
        hi[2 * (j - 2) + 1] = p1;
      }
    }
    *reinterpret_cast<uint4_*>(dst) = lo;
    *reinterpret_cast<uint4_*>(dst + 8) = hi;
  }
}

void launch_kv_dequant_blocks(const uint8_t* k_cache, const uint8_t* v_cache, const int* phys, int n,
                              long block_elems, bf16_t* k_out, bf16_t* v_out, float k_scale, float v_scale,
                              hipStream_t s) {
  if (n <= 0) return;
  const long total = 2 * (long)n * (block_elems / 16);
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  kv_dequant_blocks_kernel<<<(int)blocks, 256, 0, s>>>(k_cache, v_cache, phys, n, block_elems, k_out, v_out, k_scale,
                                                       v_scale);
}

}  // namespace shai

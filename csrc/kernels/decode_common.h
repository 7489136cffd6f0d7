// The split paged decode attention kernel (one query token per sequence), written once for both cache storage
// formats, and the pieces it shares with the wave-per-block kernel of attention.hip and the fp8 cache writers of
// attention_kv8.hip.
#pragma once
#include "common.h"
#include "launchers.h"

namespace shai {

typedef __attribute__((address_space(3))) void da_lds_void;
typedef __bf16 bf16x2d __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8d __attribute__((ext_vector_type(8)));
typedef float kv8_f32x2 __attribute__((ext_vector_type(2)));
// (pairs taken by shufflevector: bit-casting the elements of a uint32 x4 vector to bf16 x2 miscompiles with this
// hipcc -- every pair reads element 0)
#define DA_PAIR(v, i) __builtin_shufflevector(v, v, 2 * (i), 2 * (i) + 1)

constexpr float kDaLog2e = 1.4426950408889634f;

// Split count of one sequence of nblk 64-token blocks when the launch has num_splits: at least kDaMinSplitBlocks
// blocks per split, so that a batch whose factor was raised for one long context (up to 64 splits at 128k) does
// not give every short sequence 64 mostly-empty workgroups and a 64-way combine.
constexpr int kDaMinSplitBlocks = 4;
__device__ __forceinline__ int da_splits(int nblk, int num_splits) {
  return max(1, min(num_splits, (nblk + kDaMinSplitBlocks - 1) / kDaMinSplitBlocks));
}

// ----------------------------------------------------------------------------
// fp8 (OCP e4m3fn) cache codes.  One rule for every writer (ops/reference.py quantize_kv_fp8 is the oracle):
//   code  = RNE fp8(clamp(float(x_bf16) * inv_scale, -448, 448))      inv_scale = 1 / scale, computed on the host
//   value = float(code) * scale
// x_bf16 is what the bf16 cache would have stored (for K: the roped value rounded to bf16).  The clamp is explicit
// f32 arithmetic: the conversion's own overflow result depends on a mode bit.
// ----------------------------------------------------------------------------
__device__ __forceinline__ float kv8_clamp(float x) { return fminf(fmaxf(x, -448.f), 448.f); }
// two values -> two codes in the low 16 bits (a in byte 0)
__device__ __forceinline__ uint32_t kv8_q2(float a, float b, float inv) {
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a * inv), kv8_clamp(b * inv), 0, false) & 0xffffu;
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
// Cache storage formats of the split kernel: what differs between a bf16 and an fp8 cache, and nothing else.
// E is the stored element; a 16-byte chunk holds EPC of them, a K / V row CPR chunks, a 1-KB wave DMA
// instruction RPI rows.  swz(row) is the XOR a K row's chunk index takes on the source side of the DMA (the
// score loop's lane = key reads undo it); qk adds one 16-byte K chunk times the matching q elements to the two
// score chains; pv2 (D = 128) adds one key pair times this lane's two output dims; v_f32 (D = 64) widens one V
// element.  new_k / new_v give this step's token after the rounding the cache applies -- the values attended --
// and store_k / store_v are what wave 0 writes.  kMaxThreads is the wrapper's launch bound.
// ----------------------------------------------------------------------------
template <int D>
struct KvBf16 {
  typedef bf16_t E;
  static constexpr int EPC = 8, CPR = D / 8, RPI = 1024 / (2 * D);
  static constexpr int kQBytes = 8 * D * 4;   // the q rows' LDS region: sized for f32 rows, holds bf16
  // no bound given: the compiler's default of 1024 threads, a budget of 128 registers (D = 128, G = 1 spills)
  static constexpr int kMaxThreads = 1024;
  static __device__ __forceinline__ int swz(int row) { return row & (CPR - 1); }
  // 4 packed bf16 dot products (v_dot2c_f32_bf16) per 8-element chunk, two independent chains
  static __device__ __forceinline__ void qk(const uint4_ kw, const bf16_t* q, float& sc0, float& sc1) {
    const bf16x8d kv = __builtin_bit_cast(bf16x8d, kw);
    const bf16x8d qv = __builtin_bit_cast(bf16x8d, *reinterpret_cast<const uint4_*>(q));
    sc0 = __builtin_amdgcn_fdot2_f32_bf16(DA_PAIR(kv, 0), DA_PAIR(qv, 0), sc0, false);
    sc1 = __builtin_amdgcn_fdot2_f32_bf16(DA_PAIR(kv, 1), DA_PAIR(qv, 1), sc1, false);
    sc0 = __builtin_amdgcn_fdot2_f32_bf16(DA_PAIR(kv, 2), DA_PAIR(qv, 2), sc0, false);
    sc1 = __builtin_amdgcn_fdot2_f32_bf16(DA_PAIR(kv, 3), DA_PAIR(qv, 3), sc1, false);
  }
  // v_perm gathers (V[k][d], V[k+1][d]) for this lane's two dims d
  static __device__ __forceinline__ void pv2(const E* v0, const E* v1, bf16x2d pp, float& c0, float& c1) {
    const uint32_t va = *reinterpret_cast<const uint32_t*>(v0);
    const uint32_t vb = *reinterpret_cast<const uint32_t*>(v1);
    const uint32_t lo = __builtin_amdgcn_perm(vb, va, 0x05040100u);  // (V[k][2l],   V[k+1][2l])
    const uint32_t hi = __builtin_amdgcn_perm(vb, va, 0x07060302u);  // (V[k][2l+1], V[k+1][2l+1])
    c0 = __builtin_amdgcn_fdot2_f32_bf16(pp, __builtin_bit_cast(bf16x2d, lo), c0, false);
    c1 = __builtin_amdgcn_fdot2_f32_bf16(pp, __builtin_bit_cast(bf16x2d, hi), c1, false);
  }
  static __device__ __forceinline__ float v_f32(E v) { return bf2f(v); }
  static __device__ __forceinline__ float qk_scale(const DecodeAttnArgs& p) { return p.scale; }
  static __device__ __forceinline__ float out_scale(const DecodeAttnArgs&) { return 1.f; }
  // (the paged flash kernel of flash_v1.h takes the same two from its own arguments)
  static __device__ __forceinline__ float qk_scale(const AttnArgs& p) { return p.scale; }
  static __device__ __forceinline__ float out_scale(const AttnArgs&) { return 1.f; }
  // roped k rounded to bf16, as the cache stores it; v is bf16 already: both attended and stored as they are
  static __device__ __forceinline__ void new_k(const DecodeAttnArgs&, float x0, float x1, float c, float sn,
                                               float& k0, float& k1, uint32_t&) {
    k0 = bf2f(f2bf(x0 * c - x1 * sn));
    k1 = bf2f(f2bf(x1 * c + x0 * sn));
  }
  static __device__ __forceinline__ void store_k(E* k, float k0, float k1, uint32_t) {
    k[0] = f2bf(k0);
    k[D / 2] = f2bf(k1);
  }
  static __device__ __forceinline__ void new_v(const DecodeAttnArgs&, uint32_t vn_pair, float vn_one, float& v0,
                                               float& v1, uint32_t&) {
    if constexpr (D == 128) {
      v0 = bf2f(vn_pair & 0xffff);
      v1 = bf2f(vn_pair >> 16);
    } else {
      v0 = vn_one;
    }
  }
  static __device__ __forceinline__ void store_v(E* v, uint32_t vn_pair, float vn_one, uint32_t) {
    if constexpr (D == 128) *reinterpret_cast<uint32_t*>(v) = vn_pair;
    else *v = f2bf(vn_one);
  }
};

// Every e4m3 value is a bf16 value, so codes widen to bf16 pairs (v_cvt_scalef32_pk_bf16_fp8, scale 1: exact) and
// the packed dot products stay.  The scalar scales cost nothing per element: k_scale multiplies the softmax
// scale, v_scale the final normalisation (or the split partial's o).
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
template <int D>
struct KvFp8 {
  typedef uint8_t E;
  static constexpr int EPC = 16, CPR = D / 16, RPI = 1024 / D;
  static constexpr int RSH = D == 128 ? 1 : 2;   // log2 of the rows per 256-byte bank window
  static constexpr int kQBytes = 8 * D * 2;
  static constexpr int kMaxThreads = 512;
  static __device__ __forceinline__ int swz(int row) { return (row >> RSH) & (CPR - 1); }
  // a 16-code chunk = 4 words; each word widens to two bf16 pairs for two packed dot products
  static __device__ __forceinline__ void qk(const uint4_ kw, const bf16_t* q, float& sc0, float& sc1) {
    const bf16x8d qa = __builtin_bit_cast(bf16x8d, *reinterpret_cast<const uint4_*>(q));
    const bf16x8d qb = __builtin_bit_cast(bf16x8d, *reinterpret_cast<const uint4_*>(q + 8));
#define KV8_QK(word, qv, i)                                                                                        \
  sc0 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, false),             \
                                        DA_PAIR(qv, i), sc0, false);                                              \
  sc1 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, true),              \
                                        DA_PAIR(qv, (i) + 1), sc1, false)
    KV8_QK(kw[0], qa, 0);
    KV8_QK(kw[1], qa, 2);
    KV8_QK(kw[2], qb, 0);
    KV8_QK(kw[3], qb, 2);
#undef KV8_QK
  }
  // v_perm gathers the codes (V[k][d], V[k+1][d]) of this lane's two dims into the low / high half of one word,
  // which widens to the two bf16 pairs
  static __device__ __forceinline__ void pv2(const E* v0, const E* v1, bf16x2d pp, float& c0, float& c1) {
    const uint32_t va = *reinterpret_cast<const uint16_t*>(v0);
    const uint32_t vb = *reinterpret_cast<const uint16_t*>(v1);
    // bytes (V[k][2l], V[k+1][2l], V[k][2l+1], V[k+1][2l+1])
    const uint32_t x = __builtin_amdgcn_perm(vb, va, 0x05010400u);
    c0 = __builtin_amdgcn_fdot2_f32_bf16(pp, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x, 1.0f, false), c0, false);
    c1 = __builtin_amdgcn_fdot2_f32_bf16(pp, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x, 1.0f, true), c1, false);
  }
  static __device__ __forceinline__ float v_f32(E v) { return __builtin_amdgcn_cvt_f32_fp8((int)v, 0); }
  static __device__ __forceinline__ float qk_scale(const DecodeAttnArgs& p) { return p.scale * p.k_scale; }
  static __device__ __forceinline__ float out_scale(const DecodeAttnArgs& p) { return p.v_scale; }
  static __device__ __forceinline__ float qk_scale(const AttnArgs& p) { return p.scale * p.k_scale; }
  static __device__ __forceinline__ float out_scale(const AttnArgs& p) { return p.v_scale; }
  // roped k rounded to bf16 and then to its fp8 code, v to its code -- the values every later reader of the cache
  // will see.  The K rotation is kv8_rope_k, not the bf16 expression: the stored codes are checked exactly
  static __device__ __forceinline__ void new_k(const DecodeAttnArgs& p, float x0, float x1, float c, float sn,
                                               float& k0, float& k1, uint32_t& codes) {
    float ra, rb;
    kv8_rope_k(x0, x1, c, sn, ra, rb);
    const float kr0 = bf2f(f2bf(ra)), kr1 = bf2f(f2bf(rb));
    codes = kv8_q2(kr0, kr1, p.k_inv);
    const kv8_f32x2 kd = kv8_dq2(codes);
    k0 = kd[0];
    k1 = kd[1];
  }
  static __device__ __forceinline__ void store_k(E* k, float, float, uint32_t codes) {
    k[0] = (uint8_t)(codes & 0xffu);
    k[D / 2] = (uint8_t)(codes >> 8);
  }
  static __device__ __forceinline__ void new_v(const DecodeAttnArgs& p, uint32_t vn_pair, float vn_one, float& v0,
                                               float& v1, uint32_t& codes) {
    if constexpr (D == 128) {
      codes = kv8_q2(bf2f(vn_pair & 0xffff), bf2f(vn_pair >> 16), p.v_inv);
      const kv8_f32x2 vd = kv8_dq2(codes);
      v0 = vd[0];
      v1 = vd[1];
    } else {
      codes = kv8_q2(vn_one, 0.f, p.v_inv);
      v0 = kv8_dq2(codes)[0];
    }
  }
  static __device__ __forceinline__ void store_v(E* v, uint32_t, float, uint32_t codes) {
    if constexpr (D == 128) *reinterpret_cast<uint16_t*>(v) = (uint16_t)codes;
    else *v = (uint8_t)(codes & 0xffu);
  }
};

// ----------------------------------------------------------------------------
// Split decode attention, one (sequence, KV head, split) item: G = Hq/Hkv waves, one query head each (wave w =
// head hk*G+w).  The 64-token K/V blocks stream global -> LDS by LDS-DMA (buffer_load ... lds) into a two-slot
// ring: block i+1's DMA is in flight while block i is consumed (counted vmcnt of NI instructions per wave per
// block + one barrier), so HBM latency hides behind the dot products.  Per-block buffer descriptors (the cache can
// exceed 4 GiB) range-check the tail rows past the context: zero-filled, since P = 0 times a never-written NaN
// pattern would poison P.V.  Fused form (knew != nullptr): q is roped here, q / k / v come from the QKV rows or
// the skinny GEMM's split-K partials, and the last split attends this step's token and writes it to the cache.
// One split writes o; more leave partials {m, l, o[D]} for decode_combine_kernel.
// ----------------------------------------------------------------------------
template <typename Fmt, int D, int NI>
__device__ __forceinline__ void decode_attn_item(const DecodeAttnArgs& p, char* dsm, const int b, const int hk,
                                                 const int split) {
  typedef typename Fmt::E E;
  constexpr int CPR = Fmt::CPR, RPI = Fmt::RPI, EPC = Fmt::EPC, EB = sizeof(E);
  constexpr int SLOT = 2 * 64 * D;              // elements per ring slot (K then V)
  E* ring = reinterpret_cast<E*>(dsm);  // [2][K 64xD swizzled | V 64xD linear]
  // q stays bf16 (exact: it is the QKV GEMM's bf16 output) for the packed bf16 dot products; the softmax scale
  // is applied to the f32 score
  bf16_t* sQb = reinterpret_cast<bf16_t*>(ring + 2 * SLOT);                            // [G][D]
  float* sP = reinterpret_cast<float*>(reinterpret_cast<char*>(sQb) + Fmt::kQBytes);  // [G][64]
  const E* kc = static_cast<const E*>(p.k_cache);
  const E* vc = static_cast<const E*>(p.v_cache);
  const int G = p.Hq / p.Hkv;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hq = hk * G + w;
  const bool fused = p.knew != nullptr;
  const int ctx = p.ctx_lens[b] - (fused ? 1 : 0);  // tokens read from the cache
  const int nblk = (ctx + 63) / 64;
  // this sequence's own split count (da_splits): a short sequence in a batch whose split factor was raised for a
  // long one uses one split -- its other workgroups leave here, before any load
  const int nsp = da_splits(nblk, p.num_splits);
  if (split >= nsp) return;
  const int per = (nblk + nsp - 1) / nsp;
  const int blk0 = split * per, blk1 = min(nblk, blk0 + per);

  // physical block ids of this split, 64 per lane-distributed chunk (read ahead, so the ring's
  // DMA issue never waits on a block-table load queued behind the previous block's DMA)
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
  // wave w issues instructions j = w + G*t (t < NI) of the block's 2 * 64 * D * EB / 1024 = NI * G
  auto stage = [&](int slot, int bi) {
    const int phys = phys_of(bi);
    const long base = ((long)phys * p.Hkv + hk) * 64 * D;
    const __amdgpu_buffer_rsrc_t rk =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<E*>(kc + base), (short)0, 64 * D * EB, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<E*>(vc + base), (short)0, 64 * D * EB, 0x00020000);
    E* dst = ring + slot * SLOT;
#pragma unroll
    for (int t = 0; t < NI; ++t) {
      const int j = w + G * t;
      const bool isv = j >= NI * G / 2;
      const int jj = isv ? j - NI * G / 2 : j;
      const int row = jj * RPI + lane / CPR;    // this lane's row and LDS chunk position
      const int pos = lane % CPR;
      const int ch = isv ? pos : (pos ^ Fmt::swz(row));  // K: source-side XOR swizzle
      const uint32_t off = (bi * 64 + row < ctx) ? (uint32_t)((row * D + ch * EPC) * EB) : 0x80000000u;
      SHAI_DASSERT_DMA(off, 64 * D * EB, 0x80000000u);
      SHAI_DASSERT(jj * 1024 + 1024 <= 64 * D * EB);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          isv ? rv : rk, (da_lds_void*)(dst + (isv ? 64 * D : 0) + jj * (1024 / EB)), 16, off, 0, 0, 0);
    }
  };

  // first block's DMA before the q prologue: its HBM latency overlaps the q / RoPE-table loads
  if (blk0 < blk1) stage(0, blk0);
  const int rpos = fused ? p.positions[b] : 0;
  // this step's k / v (fused path, last split) loaded now and consumed after the loop, so their latency is hidden
  const bool new_tok = fused && split == nsp - 1 && p.slots[b] >= 0;
  // QKV fold fused in: element col of this row = bf16(sum of the kg partial slabs (in slab order, as the fold
  // adds them) x the folded RMSNorm scale)
  // This lane's six elements (q halves, k halves, two v) and the row's sum of squares, four slabs per round with
  // every load issued before the first add (a dependent load-add chain per slab costs ~5 us per layer).
  // (Kept in line here and in decode_attn_wb_kernel: as a helper its arrays are promoted to registers in another
  // order, and all 17 decode kernels come out with other register counts -- profiles/decode_split_unified.md)
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
  const float sl2 = Fmt::qk_scale(p) * kDaLog2e;
  float m_run = -INFINITY, l_run = 0.f;
  float o0 = 0.f, o1 = 0.f;  // D=128: this lane's d = 2 lane, 2 lane + 1; D=64: d = lane (in units of out_scale)
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
    const E* sK = ring + slot * SLOT;
    const E* sV = sK + 64 * D;
    const int key = bi * 64 + lane;  // lane = key
    // QK^T: one 16-byte K chunk per step, two independent chains
    float sc0 = 0.f, sc1 = 0.f;
#pragma unroll
    for (int ch = 0; ch < CPR; ++ch) {
      const uint4_ kw = *reinterpret_cast<const uint4_*>(sK + lane * D + (ch ^ Fmt::swz(lane)) * EPC);
      Fmt::qk(kw, sQb + w * D + ch * EPC, sc0, sc1);
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
      // products over key pairs
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
        // P[k .. k+7] as 4 bf16 pairs
        const bf16x8d pk = __builtin_bit_cast(bf16x8d, *reinterpret_cast<const uint4_*>(sPb + w * 64 + k));
        auto pvf = [&](int u, bf16x2d pp, float& c0, float& c1) {
          Fmt::pv2(sV + (k + 2 * u) * D + 2 * lane, sV + (k + 2 * u + 1) * D + 2 * lane, pp, c0, c1);
        };
        pvf(0, DA_PAIR(pk, 0), o0, o1);
        pvf(1, DA_PAIR(pk, 1), a0, a1);
        pvf(2, DA_PAIR(pk, 2), o0, o1);
        pvf(3, DA_PAIR(pk, 3), a0, a1);
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
        for (int u = 0; u < 4; ++u) o0 += pk[u] * Fmt::v_f32(sV[(k + u) * D + lane]);
      }
    }
    __builtin_amdgcn_s_barrier();  // every wave is done with this slot before it is refilled (block bi+2)
  }
  if (new_tok) {
    // this step's token, after the rounding the cache applies, as one more online-softmax key; wave 0 writes it
    // into the cache (no workgroup of this launch reads that row: the block DMA range-checks it out)
    const int slot_new = p.slots[b];
    float k0 = 0.f, k1 = 0.f, part_s = 0.f;
    uint32_t kq = 0u, vq = 0u;
    if (lane < D / 2) {
      Fmt::new_k(p, kn0, kn1, kc0, ks0, k0, k1, kq);
      part_s = k0 * bf2f(sQb[w * D + lane]) + k1 * bf2f(sQb[w * D + lane + D / 2]);
    }
    const float sc = wave_sum(part_s) * sl2;
    const float m_new = fmaxf(m_run, sc);
    const float alpha = exp2f(m_run - m_new);
    float e = exp2f(sc - m_new);
    if constexpr (D == 128) e = bf2f(f2bf(e));  // P is bf16 on the cache path too
    l_run = l_run * alpha + e;
    m_run = m_new;
    float v0 = 0.f, v1 = 0.f;
    Fmt::new_v(p, vn_pair, vn_one, v0, v1, vq);
    o0 = o0 * alpha + e * v0;
    if constexpr (D == 128) o1 = o1 * alpha + e * v1;
    if (w == 0) {
      const long dst = (((long)(slot_new >> 6) * p.Hkv + hk) * 64 + (slot_new & 63)) * D;
      if (lane < D / 2) Fmt::store_k(const_cast<E*>(kc) + dst + lane, k0, k1, kq);
      Fmt::store_v(const_cast<E*>(vc) + dst + (D == 128 ? 2 * lane : lane), vn_pair, vn_one, vq);
    }
  }
  if (nsp == 1) {  // one split: normalise (out_scale folded in) and write the output here (the combine skips this row)
    const float inv = l_run > 0.f ? Fmt::out_scale(p) / l_run : 0.f;
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
    dst[2 + 2 * lane] = o0 * Fmt::out_scale(p);
    dst[3 + 2 * lane] = o1 * Fmt::out_scale(p);
  } else {
    dst[2 + lane] = o0 * Fmt::out_scale(p);
  }
}

// One workgroup per item, or the persistent form: a grid of about two workgroups per CU walks the (sequence, KV
// head, split) items, split fastest, so one long context's 8 x 64 split items land on 512 different workgroups
// while the empty items of short sequences (da_splits) cost a ctx_lens read each instead of a workgroup launch
// with 70 KB of LDS: a batch with one 64k-token sequence launched 16,384 workgroups per layer, 97 % of them
// empty, and the launch / LDS allocation of the empty ones took longer (1.17 ms per layer) than the attention
// itself.
template <typename Fmt, int D, int NI>
__global__ void __launch_bounds__(Fmt::kMaxThreads) decode_attn_kernel(const DecodeAttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char dsm[];
  const int total = p.B * p.Hkv * p.num_splits;
  const int S = p.num_splits;
  const bool rotate = (int)gridDim.x < total;  // persistent walk only (one workgroup per item needs no spreading)
  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    // a sequence's splits sit at slots rotated by b: a short sequence's one real item lands on slot b % S instead
    // of slot 0, so the short sequences' items spread over the grid instead of piling onto the few workgroups
    // whose stride hits slot 0 (measured: 16 short sequences beside a 128k one made the launch 2.7x slower)
    const int sidx = item % S, r = item / S;
    const int b = r / p.Hkv, hk = r - b * p.Hkv;
    const int split = rotate ? (sidx - b % S + S) % S : sidx;
    decode_attn_item<Fmt, D, NI>(p, dsm, b, hk, split);
    __syncthreads();  // the next item restages ring slot 0
  }
}

}  // namespace shai

// FP8 (OCP e4m3fn) paged KV cache for gfx950: the cache writers, the native paged prefill attention (the fp8
// instantiations of flash_v1.h's kernel body) and the block widener that lets the bf16 prefill kernels run over a
// bf16 scratch copy of the blocks a step needs (the "widen" route).  (Decode attention reads the codes directly: the
// split kernel of decode_common.h with its KvFp8 format, where the quantisation rule and its helpers live.)
#include "common.h"
#include "decode_common.h"
#include "flash_v1.h"
#include "launchers.h"

namespace shai {

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

// ----------------------------------------------------------------------------
// Native fp8 paged prefill attention: the v1 flash body of flash_v1.h with the KvFp8 format -- the codes are loaded
// 16 per chunk, widened once per tile at staging and attended from the same swizzled bf16 LDS tiles, so no scratch
// copy of the cache exists.  Padded ([B, S] q with a block table) and packed (q_start) layouts, causal, GQA.
// ----------------------------------------------------------------------------
void launch_flash_attn_kv8(const AttnArgs& a, hipStream_t s) {
  dim3 grid((a.Sq + 127) / 128, a.Hq, a.B);
  const size_t lds = (size_t)4 * 64 * a.D * sizeof(bf16_t);
  if (a.D == 128) flash_fwd_kernel<KvFp8<128>, 128><<<grid, 256, lds, s>>>(a);
  else flash_fwd_kernel<KvFp8<64>, 64><<<grid, 256, lds, s>>>(a);
}

}  // namespace shai

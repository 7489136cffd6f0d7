// MXFP4 (OCP e2m1 codes + one e8m0 scale byte per 32 elements) paged KV cache for gfx950: the launch of the split
// decode kernel's KvFp4 instantiations, the cache writers and the block widener that lets the bf16 prefill kernels
// run over a bf16 scratch copy of the blocks a step needs (the "widen" route).  The format, the quantisation rule
// and its helpers live in decode_common.h beside the decode kernel that reads the codes directly.
//
// Cache layout: bytes [num_blocks, Hkv, kRegion], kRegion = 64 * (D/2 + D/32): per (block, KV head) the code plane
// (row r at r * D/2; element d in byte d / 2, even d in the low nibble), then the scale plane (row r at 64 * D/2 +
// r * D/32).  slot = block * 64 + row; slot < 0 is skipped.
//
// Writers: one 32-element group per lane group -- 4 lanes x 8 elements (one 16-byte load each) where a lane holds
// consecutive elements, 2 lanes x 16 for the V rows of the fused RoPE writer -- amax by a cross-lane max of the
// |x| patterns, codes by explicit compares (kv4_code: the oracle's thresholds and tie rule, no negative zero; not
// the hardware convert, see decode_common.h), 8 codes per dword store, the group's first lane stores the scale.
#include "common.h"
#include "decode_common.h"
#include "launchers.h"

namespace shai {

// ----------------------------------------------------------------------------
// The split decode kernel over an MXFP4 cache: NI = ceil(kNT / G) DMA instructions per wave per block (a wave's own
// count is NI or NI - 1), two ring slots + the q rows + the P rows of LDS (D = 128: 24 KB, D = 64: 15 KB).
// ----------------------------------------------------------------------------
template <int D>
static void launch_decode_kv4(const DecodeAttnArgs& a, unsigned grid, int G, hipStream_t s) {
  typedef KvFp4<D> F;
  const size_t lds = (size_t)2 * F::kSlot + F::kQBytes + 8 * 64 * 4;
#define DA4(G_) decode_attn_kernel<F, D, (F::kNT + G_ - 1) / G_><<<dim3(grid), G_ * 64, lds, s>>>(a)
  switch (G) {
    case 1: DA4(1); break;
    case 2: DA4(2); break;
    case 4: DA4(4); break;
    case 8: DA4(8); break;
    default: break;  // (the bindings reject other groups)
  }
#undef DA4
}

void launch_decode_split_kv4(const DecodeAttnArgs& a, unsigned grid, hipStream_t s) {
  const int G = a.Hq / a.Hkv;
  if (a.D == 128) launch_decode_kv4<128>(a, grid, G, s);
  else launch_decode_kv4<64>(a, grid, G, s);
}

// ----------------------------------------------------------------------------
// Quantise this lane's N * 8 bf16 values (consecutive elements of one group held by W lanes, W * N * 8 = 32): the
// group's scale byte and N words of 8 codes (element e in nibble e).
// ----------------------------------------------------------------------------
template <int W, int N>
__device__ __forceinline__ uint32_t kv4_quant(const uint4_ (&v)[N], uint32_t (&words)[N]) {
  float f[N][8];
  uint32_t amax = 0u;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    unpack8(v[n], f[n]);
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = max(amax, kv4_abs_bits(f[n][e]));
  }
  const uint32_t byte = kv4_scale_byte(kv4_group_max<W>(amax));
  const float inv = kv4_inv(byte);
#pragma unroll
  for (int n = 0; n < N; ++n) {
    uint32_t w = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) w |= kv4_code(f[n][e], inv) << (4 * e);
    words[n] = w;
  }
  return byte;
}

// one item = 8 elements of one (token, head), for K and for V; items 4 g .. 4 g + 3 of a row are group g
__global__ void kv_write_f4_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                   uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, const int* __restrict__ slots,
                                   int T, int Hkv, int D, long k_ts, long v_ts) {
  const int IPR = D / 8;
  const long region = 64L * (D / 2 + D / 32);
  const long total = (long)T * Hkv * IPR;   // a multiple of 4, as the grid stride: a group's lanes stay together
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % IPR);
    const int h = (int)((i / IPR) % Hkv);
    const int t = (int)(i / ((long)IPR * Hkv));
    const int slot = slots[t];
    if (slot < 0) continue;
    const long reg = ((long)(slot >> 6) * Hkv + h) * region;
    const int row = slot & 63;
    const uint4_ kv[1] = {*reinterpret_cast<const uint4_*>(k + (long)t * k_ts + (long)h * D + c * 8)};
    const uint4_ vv[1] = {*reinterpret_cast<const uint4_*>(v + (long)t * v_ts + (long)h * D + c * 8)};
    uint32_t kw[1], vw[1];
    const uint32_t kb = kv4_quant<4, 1>(kv, kw);
    const uint32_t vb = kv4_quant<4, 1>(vv, vw);
    *reinterpret_cast<uint32_t*>(kc + reg + row * (D / 2) + c * 4) = kw[0];
    *reinterpret_cast<uint32_t*>(vc + reg + row * (D / 2) + c * 4) = vw[0];
    if ((c & 3) == 0) {
      kc[reg + 32 * D + row * (D / 32) + (c >> 2)] = (uint8_t)kb;
      vc[reg + 32 * D + row * (D / 32) + (c >> 2)] = (uint8_t)vb;
    }
  }
}

void launch_kv_write_f4(const bf16_t* k, const bf16_t* v, uint8_t* k_cache, uint8_t* v_cache, const int* slot_mapping,
                        int T, int Hkv, int D, long k_ts, long v_ts, hipStream_t s) {
  const long total = (long)T * Hkv * (D / 8);
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  kv_write_f4_kernel<<<(int)blocks, 256, 0, s>>>(k, v, k_cache, v_cache, slot_mapping, T, Hkv, D, k_ts, v_ts);
}

// rope_qkv_cache over an MXFP4 cache: q is roped in place as bf16 (the bf16 kernel's expression); k is roped by
// kv8_rope_k, rounded to bf16 (the value the bf16 cache would hold) and quantised; v is quantised.  One item = 16
// elements as in the bf16 / fp8 kernels: for q / k heads 8 elements of each rotation half -- items 4 g .. 4 g + 3
// hold group g of the first half and group g + D/64 of the second -- for v heads 16 consecutive elements, two
// items per group.
__global__ void rope_qkv_cache_f4_kernel(bf16_t* __restrict__ qkv, long ld, const int* __restrict__ pos,
                                         const float* __restrict__ cs, const float* __restrict__ sn,
                                         uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                         const int* __restrict__ slots, int T, int H, int Hkv, int D) {
  const int half = D >> 1;
  const int per_head = D / 16;   // 4 or 8: the 4- and 2-lane groups below never straddle a head
  const int heads = H + 2 * Hkv;
  const long region = 64L * (D / 2 + D / 32);
  const long total = (long)T * heads * per_head;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const int t = (int)(i / ((long)per_head * heads));
    bf16_t* row = qkv + (long)t * ld;
    const int slot = slots[t];
    if (hh >= H + Hkv) {  // v head: 16 elements -> 16 codes (8 bytes)
      if (slot < 0) continue;
      const int h = hh - H - Hkv;
      const bf16_t* src = row + (long)hh * D + c * 16;
      const uint4_ vv[2] = {*reinterpret_cast<const uint4_*>(src), *reinterpret_cast<const uint4_*>(src + 8)};
      uint32_t vw[2];
      const uint32_t vb = kv4_quant<2, 2>(vv, vw);
      const long reg = ((long)(slot >> 6) * Hkv + h) * region;
      *reinterpret_cast<uint2_*>(vc + reg + (slot & 63) * half + c * 8) = uint2_{vw[0], vw[1]};
      if ((c & 1) == 0) vc[reg + 32 * D + (slot & 63) * (D / 32) + (c >> 1)] = (uint8_t)vb;
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
      const uint4_ k0[1] = {ua}, k1[1] = {ub};
      uint32_t w0[1], w1[1];
      const uint32_t b0 = kv4_quant<4, 1>(k0, w0);
      const uint32_t b1 = kv4_quant<4, 1>(k1, w1);
      const long reg = ((long)(slot >> 6) * Hkv + h) * region;
      uint8_t* kr = kc + reg + (slot & 63) * half;
      *reinterpret_cast<uint32_t*>(kr + 4 * c) = w0[0];
      *reinterpret_cast<uint32_t*>(kr + D / 4 + 4 * c) = w1[0];
      if ((c & 3) == 0) {
        uint8_t* ks = kc + reg + 32 * D + (slot & 63) * (D / 32);
        ks[c >> 2] = (uint8_t)b0;
        ks[D / 64 + (c >> 2)] = (uint8_t)b1;
      }
    }
  }
}

void launch_rope_qkv_cache_f4(bf16_t* qkv, long ld, const int* pos, const float* cos, const float* sin,
                              uint8_t* k_cache, uint8_t* v_cache, const int* slots, int T, int H, int Hkv, int D,
                              hipStream_t s) {
  const long total = (long)T * (H + 2 * Hkv) * (D / 16);
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  rope_qkv_cache_f4_kernel<<<(int)blocks, 256, 0, s>>>(qkv, ld, pos, cos, sin, k_cache, v_cache, slots, T, H, Hkv, D);
}

// ----------------------------------------------------------------------------
// kv_dequant_blocks over an MXFP4 cache: scratch block i (bf16 [n, Hkv, 64, D]) = code * 2^(scale - 127) of cache
// block phys[i], for K and V.  Exact: every product is a bf16 value.  One item = one scale group: a 16-byte load of
// 32 codes and its scale byte, four 16-byte stores.
// ----------------------------------------------------------------------------
__global__ void kv_dequant_blocks_f4_kernel(const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                            const int* __restrict__ phys, int n, int Hkv, int D,
                                            bf16_t* __restrict__ ko, bf16_t* __restrict__ vo) {
  const int GPR = D / 32;
  const long region = 64L * (D / 2 + D / 32);
  const long per = (long)n * Hkv * 64 * GPR;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < 2 * per; i += (long)gridDim.x * blockDim.x) {
    const bool isv = i >= per;
    long r = isv ? i - per : i;
    const int g = (int)(r % GPR);
    r /= GPR;
    const int row = (int)(r & 63);
    r >>= 6;
    const int h = (int)(r % Hkv);
    const int blk = (int)(r / Hkv);
    const uint8_t* src = (isv ? vc : kc) + ((long)phys[blk] * Hkv + h) * region;
    const uint4_ cw = *reinterpret_cast<const uint4_*>(src + row * (D / 2) + g * 16);
    const float sc = kv4_scale(src[32 * D + row * GPR + g]);
    bf16_t* dst = (isv ? vo : ko) + (((long)blk * Hkv + h) * 64 + row) * D + g * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint4_ o;
      o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(cw[j], sc, 0));
      o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(cw[j], sc, 1));
      o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(cw[j], sc, 2));
      o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(cw[j], sc, 3));
      *reinterpret_cast<uint4_*>(dst + 8 * j) = o;
    }
  }
}

void launch_kv_dequant_blocks_f4(const uint8_t* k_cache, const uint8_t* v_cache, const int* phys, int n, int Hkv,
                                 int D, bf16_t* k_out, bf16_t* v_out, hipStream_t s) {
  if (n <= 0) return;
  const long total = 2L * n * Hkv * 64 * (D / 32);
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  kv_dequant_blocks_f4_kernel<<<(int)blocks, 256, 0, s>>>(k_cache, v_cache, phys, n, Hkv, D, k_out, v_out);
}

}  // namespace shai

// Skinny GEMM over MXFP4 weights for decode-shaped problems (M <= 64 activation rows):
//
//   C[m, n] = act(alpha * rstd[m] * sum_k X[m, k] * What[n, k] + bias[n]) (+ res_alpha * R[m, n]),  GLU optional
//
// What = code * 2^(scale - 127): OCP e2m1 codes, two per byte (even k in the low nibble), W [N, K / 2] bytes row-major,
// and one e8m0 scale byte per (row, 32 consecutive k), stored tiled per K step: S [ceil(K / 128), N, 4] bytes, entry
// (s, n, g) = the scale of row n's group 4 s + g (groups past K / 32 hold 127 = 1.0).  ops.quantize_mxfp4 produces this
// layout, ops.dequant_mxfp4 (dequant_mxfp4_kernel below) inverts it.
//
// Decode is weight-bandwidth bound (gemv.hip), and at 4 bits the 64 x 64 step of gemv.hip would be a 2 KB weight tile
// beside a 4 / 8 KB activation tile: the CU's DMA issue and LDS writes would mostly carry X (gemv2.hip names that
// ratio as what limits M = 64).  Geometry chosen here:
//
// * Workgroup = 4 waves, tile = 128 W rows x all M rows of X, K step = 128 (exactly 4 scale groups).  A step moves
//   8 KB of codes (128 rows x 64 B), 512 B of scales and 8 KB (M <= 32) or 16 KB (M <= 64) of X: X : W bytes = 1 : 1
//   and 2 : 1, the ratio the fp8 form of gemv.hip has, at half its weight bytes.  256 rows would halve the ratio again
//   but leave N = 4096 with 16 tiles (split-K slabs of 256 x M floats, K groups of 1-2 steps) and 57344 rows with 224
//   tiles for 256 CUs; 128 rows keep the tile counts of gemv2.hip.
// * Ring of 4 stages x 17 KB (M <= 32) or 3 x 25 KB (M <= 64): two workgroups per CU either way, so a CU holds
//   2 x 3 x 8 = 48 KB / 2 x 2 x 8 = 32 KB of weight bytes in flight.  That is under gemv.hip's 64 KB estimate and
//   beside its fp8 form's 60 / 36 KB: the X tile riding along bounds the ring (160 KB of LDS per CU), and a 64-row
//   tile would have halved these figures.  Measured (profiles/mxfp4_decode.md): 3.5 TB/s of fp4 bytes at
//   57344 x 8192, 0.61-0.79 of the fp8 kernel's time at the large shapes.  One workgroup per CU with a 9-deep ring
//   (64 KB in flight at M <= 32) is the untried alternative.
// * The body is skinny_rows_kernel (skinny_common.h), shared with the bf16 wide kernel of gemv2.hip: wave w consumes
//   the WHOLE step of its 32 rows (no cross-wave reduction), counted vmcnt + one s_barrier per step, epilogue from the
//   accumulators (bias / act / GLU / residual / folded RMSNorm) in quads, split-K over kg workgroups per tile in both
//   forms of gemv.hip: fp32 partials [kg][M][N] (+ row sums of squares) folded by launch_splitk_epilogue, or slabs
//   written through (sc1) with an arrival ticket per tile and the last arriver summing them in K-group order.  This
//   file holds the MXFP4 format policy WMxfp4, the instantiations, the launcher and the dequantise kernel.
// * Everything arrives by LDS-DMA (buffer_load ... lds, range check = zero fill for rows >= N / M and K tails): wave w
//   fetches the codes (2 instructions of 16 rows x 64 B, 16-B chunk c at position c ^ (row >> 2) & 3) and the scales
//   (one 4-B instruction, lanes 0-31 = its rows, lanes 32-63 out of range) of its own rows [32 w, 32 w + 32), and a
//   quarter of the X tile (4 rows x 256 B per instruction, 16-B chunk c at position c ^ row & 15).
// * Lane (fr, fh) reads the two 16-B code chunks 2 fh, 2 fh + 1 of row fr (each = one scale group), widens every
//   dword (8 codes) to 8 bf16 with v_cvt_scalef32_pk_bf16_fp4 -- the group scale 2^(byte - 127) goes into the convert
//   as an fp32 power of two built from the byte, so products are exact whichever way the instruction applies a scale
//   -- and the body issues 8 x (M / 32) v_mfma_f32_32x32x16_bf16 against the X chunks holding the same k (K is
//   consumed in a permuted order inside the step; fp32 accumulation).
#include "skinny_common.h"

namespace shai {

struct WMxfp4 {
  static constexpr int BK = 128, SLICES = 8;  // K per step (4 scale groups), its k16 slices
  static constexpr bool FOLD = true, QUAD_STORES = true;
  static constexpr int W_BYTES = SR_BN * BK / 2;  // 8 KB of codes
  static constexpr int S_BYTES = 4 * 256;         // one 64-lane x 4-B DMA per wave (upper 32 lanes zero fill)
  static constexpr int stage_bytes(int MB) { return W_BYTES + S_BYTES + MB * BK * 2; }  // codes, scales, X
  static constexpr int per(int MB) { return 2 + 1 + 2 * (MB / 32); }                    // DMA instructions per wave

  template <int MB>
  struct Lane {
    static constexpr int XJ = 2 * (MB / 32);  // X DMA instructions per wave
    __amdgpu_buffer_rsrc_t rW, rS, rX;
    uint32_t woff[2], wk[2], soff, xoff[XJ], xk[XJ];

    // DMA geometry (LDS images are lane-linear per wave instruction; the swizzle is on the source address)
    __device__ __forceinline__ void init(const GemmArgs& p, int n0, int w, int lane, int ksteps) {
      rW = buf_rsrc(p.W, (long)p.N * p.ldw);  // ldw: bytes
      rS = buf_rsrc(p.w_mx_scale, (long)ksteps * p.N * 4);
      rX = buf_rsrc(p.A, (long)p.M * p.lda * 2);
      // codes: instruction j of wave w fills tile rows 32 w + 16 j + (lane >> 2), chunk position lane & 3
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = 32 * w + 16 * j + (lane >> 2), n = n0 + row;
        const int c = (lane & 3) ^ ((row >> 2) & 3);
        wk[j] = (uint32_t)(c * 32);  // first k of the chunk inside the step
        woff[j] = n < p.N ? (uint32_t)((long)n * p.ldw + c * 16) : kDmaOob;
      }
      // scales: lanes 0-31 fetch the 4 scale bytes of tile row 32 w + lane
      soff = (lane < 32 && n0 + 32 * w + lane < p.N) ? (uint32_t)((n0 + 32 * w + lane) * 4) : kDmaOob;
      // X: instruction i = XJ w + j fills rows 4 i + (lane >> 4), chunk position lane & 15
#pragma unroll
      for (int j = 0; j < XJ; ++j) {
        const int row = 4 * (XJ * w + j) + (lane >> 4);
        const int c = (lane & 15) ^ (row & 15);
        xk[j] = (uint32_t)(c * 8);
        xoff[j] = row < p.M ? (uint32_t)(((long)row * p.lda + c * 8) * 2) : kDmaOob;
      }
    }

    __device__ __forceinline__ void stage(const GemmArgs& p, uint8_t* st, int w, int kstep) const {
      uint8_t* sw = st;
      uint8_t* ss = sw + W_BYTES;
      uint8_t* sx = ss + S_BYTES;
      const uint32_t k0 = (uint32_t)kstep * BK;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // K tail: whole 32-code chunks past K read as zeros (K % 32 == 0)
        const uint32_t off = (woff[j] != kDmaOob && k0 + wk[j] < (uint32_t)p.K) ? woff[j] + (k0 >> 1) : kDmaOob;
        SHAI_DASSERT_DMA(off, (long)p.N * p.ldw, kDmaOob);
        // weights are read once per decode step by one CU: nt (aux 2), as in gemv.hip
        if (p.w_nt) __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (32 * w + 16 * j) * 64), 16, off, 0, 0, 2);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (32 * w + 16 * j) * 64), 16, off, 0, 0, 0);
      }
      {
        const uint32_t off = soff != kDmaOob ? soff + (uint32_t)kstep * (uint32_t)p.N * 4u : kDmaOob;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rS, (lds_void*)(ss + w * 256), 4, off, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < XJ; ++j) {
        const uint32_t off = (xoff[j] != kDmaOob && k0 + xk[j] < (uint32_t)p.K) ? xoff[j] + k0 * 2 : kDmaOob;
        SHAI_DASSERT_DMA(off, (long)p.M * p.lda * 2, kDmaOob);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (lds_void*)(sx + (XJ * w + j) * 1024), 16, off, 0, 0, 0);
      }
    }

    // k16 slice s = 4 i + j: dword j of code chunk c = 2 fh + i (one scale group; k = 32 c + 8 j .. + 7), widened,
    // against X chunk 4 c + j.  (The scale dword and the 16-B chunk are read per slice in the source; the unrolled
    // body reads each once.)
    __device__ __forceinline__ bf16x8 w_frag(const uint8_t* st, int w, int fr, int fh, int s, int& xc) const {
      const uint8_t* sw = st;
      const uint8_t* ss = sw + W_BYTES;
      const int wrow = 32 * w + fr, wswz = (wrow >> 2) & 3;
      const uint32_t sc4 = *reinterpret_cast<const uint32_t*>(ss + w * 256 + fr * 4);
      const int c = 2 * fh + (s >> 2), j = s & 3;
      SHAI_DASSERT(wrow * 64 + ((c ^ wswz) << 4) + 16 <= W_BYTES);
      const uint4_ cw = *reinterpret_cast<const uint4_*>(sw + wrow * 64 + ((c ^ wswz) << 4));
      xc = 4 * c + j;
      return fp4x8_widen(cw[j], e8m0_scale((sc4 >> (8 * c)) & 0xffu));
    }
    static __device__ __forceinline__ bf16x8 x_frag(const uint8_t* st, int row, int xc) {
      return *reinterpret_cast<const bf16x8*>(st + W_BYTES + S_BYTES + row * 256 + ((xc ^ (row & 15)) << 4));
    }
  };
};

// ring depth: 4 stages (M <= 32) / 3 (M <= 64), two workgroups per CU either way
template <int MB>
struct Q4Geom {
  static constexpr int STAGES = MB == 32 ? 4 : 3;
  static constexpr size_t LDS = (size_t)STAGES * WMxfp4::stage_bytes(MB);
  static constexpr int SLAB = SR_BN * MB + MB;  // floats of one (tile, K group) slab of the fixup
};

// MXFP4 codes + tiled scales -> bf16 [N, K] (prefill-shaped problems run the bf16 GEMMs on it): one thread per
// scale group (16 B of codes -> 64 B of bf16)
__global__ void __launch_bounds__(256) dequant_mxfp4_kernel(const uint8_t* __restrict__ wq,
                                                            const uint8_t* __restrict__ scales,
                                                            bf16_t* __restrict__ out, long groups, int KG32, long N) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < groups; i += (long)gridDim.x * blockDim.x) {
    const long n = i / KG32;
    const int g = (int)(i - n * KG32);
    const float scale = e8m0_scale(scales[((long)(g >> 2) * N + n) * 4 + (g & 3)]);
    const uint4_ cw = reinterpret_cast<const uint4_*>(wq)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8 wf = fp4x8_widen(cw[j], scale);
      reinterpret_cast<uint4_*>(out)[i * 4 + j] = __builtin_bit_cast(uint4_, wf);
    }
  }
}

void launch_dequant_mxfp4(const uint8_t* wq, const uint8_t* scales, bf16_t* out, long N, int K, hipStream_t s) {
  const long groups = N * (long)(K / 32);
  if (groups == 0) return;
  long blocks = (groups + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  dequant_mxfp4_kernel<<<(int)blocks, 256, 0, s>>>(wq, scales, out, groups, K / 32, N);
}

// ---------------------------------------------------------------------------- host side
// a.W: codes [N, K / 2] bytes at a row stride of a.ldw BYTES; a.w_mx_scale: [ceil(K / 128), N, 4] bytes
bool skinny_fp4_supported(const GemmArgs& a) {
  if (a.res_rows != 0) return false;  // no broadcast residual
  return a.w_mx_scale != nullptr && a.w_scale == nullptr && !a.conv && a.batch <= 1 && a.w_slice_rows == 0 &&
         a.M >= 1 && a.M <= 64 && a.K >= 32 && a.K % 32 == 0 && a.N >= 1 && a.N % 2 == 0 && (!a.glu || a.N % 4 == 0) &&
         a.bias2d == nullptr && a.gate == nullptr && a.in_scale == nullptr && a.row_mr == nullptr &&
         a.col_part == nullptr && a.row_part == nullptr && a.lda % 8 == 0 && a.ldw % 16 == 0 && a.ldw >= a.K / 2 &&
         (long)a.N * a.ldw < 0x7fffffffL && (long)a.M * a.lda * 2 < 0x7fffffffL &&
         (long)((a.K + WMxfp4::BK - 1) / WMxfp4::BK) * a.N * 4 < 0x7fffffffL;
}

// K groups: about one workgroup per CU (two fit), each group at least 4 K steps
int skinny_fp4_kgroups(const GemmArgs& a) {
  const int tiles = (a.N + SR_BN - 1) / SR_BN, ksteps = (a.K + WMxfp4::BK - 1) / WMxfp4::BK;
  int kg = 1;
  while (tiles * kg < 256 && ksteps / (kg * 2) >= 4) kg *= 2;
  return kg;
}

int skinny_fp4_max_kgroups(const GemmArgs& a) { return max_kgroups((a.K + WMxfp4::BK - 1) / WMxfp4::BK); }

size_t skinny_fp4_workspace_bytes(const GemmArgs& a, int kg) {
  if (kg <= 1) return 0;
  const size_t fold = (size_t)kg * a.M * a.N + (size_t)kg * a.M;  // [kg][M][N] + row sums of squares
  const int slab = a.M <= 32 ? Q4Geom<32>::SLAB : Q4Geom<64>::SLAB;
  const size_t fix = (size_t)((a.N + SR_BN - 1) / SR_BN) * kg * (size_t)slab;  // [tile][kg] slabs
  return (fold > fix ? fold : fix) * sizeof(float);
}

template <int MB>
static void launch_fp4_mb(const GemmArgs& a, float* ws, KSplit ks, unsigned* cnt, hipStream_t s) {
  const dim3 grid((a.N + SR_BN - 1) / SR_BN, ks.kg), block(256);
  using G = Q4Geom<MB>;
  dispatch_epilogue<kActsAll>(a, [&](auto glu, auto act, auto rms) {
    skinny_rows_kernel<WMxfp4, MB, glu(), act(), rms(), G::STAGES><<<grid, block, G::LDS, s>>>(a, ws, ks.kg_steps, cnt);
  });
}

// kg K groups (needs ws of skinny_fp4_workspace_bytes, else kg = 1); fixup: reduce the split-K partials inside the
// launch when a ticket slice is available, else (and without fixup) the separate fold kernel
void launch_skinny_fp4(const GemmArgs& a_in, float* ws, int kg, bool fixup, hipStream_t s) {
  GemmArgs a = a_in;
  a.w_nt = skinny_nt();
  const int tiles = (a.N + SR_BN - 1) / SR_BN;
  const KSplit ks = split_ksteps((a.K + WMxfp4::BK - 1) / WMxfp4::BK, ws != nullptr ? kg : 1);
  unsigned* cnt = nullptr;
  const int slab = a.M <= 32 ? Q4Geom<32>::SLAB : Q4Geom<64>::SLAB;
  // (the slabs are addressed through one buffer descriptor: past 2 GiB the fold kernel takes the split)
  if (ks.kg > 1 && fixup && (long)tiles * ks.kg * slab * 4 < 0x7fffffffL) cnt = skinny_ticket_slice(s, tiles);
  if (a.M <= 32) launch_fp4_mb<32>(a, ws, ks, cnt, s);
  else launch_fp4_mb<64>(a, ws, ks, cnt, s);
  if (ks.kg > 1 && cnt == nullptr) launch_splitk_epilogue(a, ws, ks.kg, s);
}

}  // namespace shai

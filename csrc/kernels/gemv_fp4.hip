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
//   (64 KB in flight at M <= 32) is the untried alternative.  Counted vmcnt + one s_barrier per step, the protocol
//   of gemv.hip.
// * Everything arrives by LDS-DMA (buffer_load ... lds, range check = zero fill for rows >= N / M and K tails): wave w
//   fetches the codes (2 instructions of 16 rows x 64 B, 16-B chunk c at position c ^ (row >> 2) & 3) and the scales
//   (one 4-B instruction, lanes 0-31 = its rows, lanes 32-63 out of range) of its own rows [32 w, 32 w + 32), and a
//   quarter of the X tile (4 rows x 256 B per instruction, 16-B chunk c at position c ^ row & 15).
// * Wave w consumes the WHOLE step of its 32 rows (no cross-wave reduction, as gemv2.hip): lane (fr, fh) reads the
//   two 16-B code chunks 2 fh, 2 fh + 1 of row fr (each = one scale group), widens every dword (8 codes) to 8 bf16
//   with v_cvt_scalef32_pk_bf16_fp4 -- the group scale 2^(byte - 127) goes into the convert as an fp32 power of two
//   built from the byte, so products are exact whichever way the instruction applies a scale -- and issues
//   8 x (M / 32) v_mfma_f32_32x32x16_bf16 against the X chunks holding the same k (K is consumed in a permuted order
//   inside the step; fp32 accumulation).
// * Epilogue from the accumulators (bias / act / GLU / residual / folded RMSNorm: every wave sums the squares of the
//   X fragments it reads anyway).  Split-K over kg workgroups per tile, both forms of gemv.hip: fp32 partials
//   [kg][M][N] (+ row sums of squares) folded by launch_splitk_epilogue, or slabs written through (sc1) with an
//   arrival ticket per tile (skinny_ticket_slice) and the last arriver summing them in K-group order.
#include "common.h"
#include "launchers.h"
#include "gemm_epilogue.h"

#include <cstdlib>

namespace shai {

typedef __bf16 bf16x8q __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2q __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void q4_lds_void;

constexpr int Q4_BN = 128;                      // W rows per workgroup
constexpr int Q4_BK = 128;                      // K per step (4 scale groups)
constexpr int Q4_WAVES = 4;
constexpr int Q4_W_BYTES = Q4_BN * Q4_BK / 2;   // 8 KB of codes
constexpr int Q4_S_BYTES = Q4_WAVES * 256;      // one 64-lane x 4-B DMA per wave (upper 32 lanes zero fill)
constexpr uint32_t Q4_OOB = 0x80000000u;

template <int MB>
struct Q4Geom {
  static constexpr int XG = MB / 32;                       // 32-row X groups
  static constexpr int STAGES = MB == 32 ? 4 : 3;
  static constexpr int X_BYTES = MB * Q4_BK * 2;
  static constexpr int STAGE_BYTES = Q4_W_BYTES + Q4_S_BYTES + X_BYTES;  // codes, scales, X
  static constexpr int PER = 2 + 1 + 2 * XG;               // DMA instructions per wave per step
  static constexpr size_t LDS = (size_t)STAGES * STAGE_BYTES;
  static constexpr int SLAB = Q4_BN * MB + MB;             // floats of one (tile, K group) slab of the fixup
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t q4_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}

// write-through (sc1) stores / loads of the in-launch split-K hand-off (cache policy bit sc1 = 16)
__device__ __forceinline__ void q4_store_wt(__amdgpu_buffer_rsrc_t r, uint32_t off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)off, 0, 16);
}
__device__ __forceinline__ float q4_load_wt(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 16));
}
__device__ __forceinline__ void q4_store4_wt(__amdgpu_buffer_rsrc_t r, uint32_t off, const float* v) {
  const uint4_ u = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
  __builtin_amdgcn_raw_buffer_store_b128(u, r, (int)off, 0, 16);
}
__device__ __forceinline__ void q4_load4_wt(__amdgpu_buffer_rsrc_t r, uint32_t off, float* v) {
  const uint4_ u = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(u[i]);
}

template <int PER, int N>
__device__ __forceinline__ void q4_wait_upto(int pending) {
  // s_waitcnt needs an immediate: allow `pending` DMA groups (of PER loads) to stay in flight
  if constexpr (N == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    if (pending >= N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N * PER) : "memory");
    else q4_wait_upto<PER, N - 1>(pending);
  }
}

// 2^(byte - 127) as fp32.  The quantiser keeps bytes in [2, 252]; a zero-filled byte (rows >= N) reads as 2^-126.
__device__ __forceinline__ float q4_scale(uint32_t byte) { return __uint_as_float(max(byte, 1u) << 23); }

// 8 e2m1 codes (one dword, even k in the low nibbles) x scale -> 8 bf16 (exact: code * power of two)
__device__ __forceinline__ bf16x8q q4_widen(uint32_t codes, float scale) {
  bf16x8q r;
  const bf16x2q a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 0);
  const bf16x2q b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 1);
  const bf16x2q c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 2);
  const bf16x2q d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 3);
  r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1];
  r[4] = c[0]; r[5] = c[1]; r[6] = d[0]; r[7] = d[1];
  return r;
}

// one output element (pair): bias, activation (GLU: value * act(gate)), residual, bf16 store -- tiles cut by N
template <bool GLU, int ACT>
__device__ __forceinline__ void q4_store(const GemmArgs& p, int n, int m, float v0, float v1) {
  if (n >= p.N) return;
  if constexpr (GLU) {
    const float a = v0 * p.alpha + (p.bias ? bf2f(p.bias[n]) : 0.f);
    const float g = v1 * p.alpha + (p.bias ? bf2f(p.bias[n + 1]) : 0.f);
    float o = a * apply_act<ACT>(g);
    const int nc = n >> 1;
    if (p.residual) o += bf2f(p.residual[(long)m * p.ldr + nc]) * p.res_alpha;
    p.C[(long)m * p.ldc + nc] = f2bf(o);
  } else {
    float o = apply_act<ACT>(v0 * p.alpha + (p.bias ? bf2f(p.bias[n]) : 0.f));
    if (p.residual) o += bf2f(p.residual[(long)m * p.ldr + n]) * p.res_alpha;
    p.C[(long)m * p.ldc + n] = f2bf(o);
  }
}

// fused epilogue of the quad (m, n .. n + 3): 2 GLU pairs / 4 outputs, 8-B stores where the quad is whole
template <bool GLU, int ACT>
__device__ __forceinline__ void q4_quad_out(const GemmArgs& p, int m, int n, float v[4]) {
  if (m >= p.M || n >= p.N) return;
  if (n + 3 < p.N) {
    epilogue4<GLU, ACT>(p, p.C, p.residual, m, n, v);
  } else if constexpr (GLU) {
    for (int e = 0; e < 4 && n + e + 1 < p.N; e += 2) q4_store<GLU, ACT>(p, n + e, m, v[e], v[e + 1]);
  } else {
    for (int e = 0; e < 4; ++e) q4_store<GLU, ACT>(p, n + e, m, v[e], 0.f);
  }
}

// Accumulator layout of v_mfma_f32_32x32x16 with W rows as A and X rows as B: lane (fr = lane & 31, fh = lane >> 5)
// holds D[n][m] for m = 32 g + fr and n = 8 q + 4 fh + e in registers 4 q + e (q, e = 0..3): quads of 4 consecutive n.
template <int MB, bool GLU, int ACT, bool RMS>
__global__ void __launch_bounds__(Q4_WAVES * 64) skinny_fp4_kernel(const GemmArgs p, float* __restrict__ ws,
                                                                   int kg_steps, unsigned* __restrict__ cnt) {
  using G = Q4Geom<MB>;
  constexpr int XG = G::XG;
  // ALL LDS of the kernel is this one array (the last-arriver flag of the fixup reuses the dead ring): a second
  // __shared__ object beside an LDS-DMA ring can make the compiler drain vmcnt before every step's first ds_read
  extern __shared__ __attribute__((aligned(16))) uint8_t q4_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, kg = blockIdx.y, KG = gridDim.y;
  const int n0 = tile * Q4_BN;
  const int ksteps = (p.K + Q4_BK - 1) / Q4_BK;
  const int t0 = kg * kg_steps;
  const int nk = max(0, min(ksteps, t0 + kg_steps) - t0);

  const __amdgpu_buffer_rsrc_t rW = q4_rsrc(p.W, (uint32_t)min((long)p.N * p.ldw, 0x7fffffffL));  // ldw: bytes
  const __amdgpu_buffer_rsrc_t rS = q4_rsrc(p.w_mx_scale, (uint32_t)min((long)ksteps * p.N * 4, 0x7fffffffL));
  const __amdgpu_buffer_rsrc_t rX = q4_rsrc(p.A, (uint32_t)min((long)p.M * p.lda * 2, 0x7fffffffL));

  // DMA geometry (LDS images are lane-linear per wave instruction; the swizzle is on the source address).
  // codes: instruction j of wave w fills tile rows 32 w + 16 j + (lane >> 2), chunk position lane & 3
  uint32_t woff[2], wk[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = 32 * w + 16 * j + (lane >> 2), n = n0 + row;
    const int c = (lane & 3) ^ ((row >> 2) & 3);
    wk[j] = (uint32_t)(c * 32);                                     // first k of the chunk inside the step
    woff[j] = n < p.N ? (uint32_t)((long)n * p.ldw + c * 16) : Q4_OOB;
  }
  // scales: lanes 0-31 fetch the 4 scale bytes of tile row 32 w + lane
  const uint32_t soff = (lane < 32 && n0 + 32 * w + lane < p.N) ? (uint32_t)((n0 + 32 * w + lane) * 4) : Q4_OOB;
  // X: instruction i = 2 XG w + j fills rows 4 i + (lane >> 4), chunk position lane & 15
  uint32_t xoff[2 * XG], xk[2 * XG];
#pragma unroll
  for (int j = 0; j < 2 * XG; ++j) {
    const int row = 4 * (2 * XG * w + j) + (lane >> 4);
    const int c = (lane & 15) ^ (row & 15);
    xk[j] = (uint32_t)(c * 8);
    xoff[j] = row < p.M ? (uint32_t)(((long)row * p.lda + c * 8) * 2) : Q4_OOB;
  }
  auto stage = [&](int buf, int step) {
    uint8_t* sw = q4_smem + buf * G::STAGE_BYTES;
    uint8_t* ss = sw + Q4_W_BYTES;
    uint8_t* sx = ss + Q4_S_BYTES;
    const uint32_t k0 = (uint32_t)(t0 + step) * Q4_BK;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      // K tail: whole 32-code chunks past K read as zeros (K % 32 == 0)
      const uint32_t off = (woff[j] != Q4_OOB && k0 + wk[j] < (uint32_t)p.K) ? woff[j] + (k0 >> 1) : Q4_OOB;
      SHAI_DASSERT_DMA(off, (long)p.N * p.ldw, Q4_OOB);
      // weights are read once per decode step by one CU: nt (aux 2), as in gemv.hip
      if (p.w_nt) __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (q4_lds_void*)(sw + (32 * w + 16 * j) * 64), 16, off, 0, 0, 2);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (q4_lds_void*)(sw + (32 * w + 16 * j) * 64), 16, off, 0, 0, 0);
    }
    {
      const uint32_t off = soff != Q4_OOB ? soff + (uint32_t)(t0 + step) * (uint32_t)p.N * 4u : Q4_OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rS, (q4_lds_void*)(ss + w * 256), 4, off, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2 * XG; ++j) {
      const uint32_t off = (xoff[j] != Q4_OOB && k0 + xk[j] < (uint32_t)p.K) ? xoff[j] + k0 * 2 : Q4_OOB;
      SHAI_DASSERT_DMA(off, (long)p.M * p.lda * 2, Q4_OOB);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (q4_lds_void*)(sx + (2 * XG * w + j) * 1024), 16, off, 0, 0, 0);
    }
  };

  float16_ acc[XG];
#pragma unroll
  for (int g = 0; g < XG; ++g)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[g][i] = 0.f;
  float ss2[XG];  // folded RMSNorm: this lane's share of sum_k X[m, k]^2 (m = 32 g + fr; lanes fr, fr + 32 together
                  // read every X element of every step once)
#pragma unroll
  for (int g = 0; g < XG; ++g) ss2[g] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;
  const int wrow = 32 * w + fr, wswz = (wrow >> 2) & 3;
#pragma unroll
  for (int i = 0; i < G::STAGES - 1; ++i)
    if (i < nk) stage(i, i);
  int buf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    q4_wait_upto<G::PER, G::STAGES - 2>(min(G::STAGES - 2, nk - 1 - kt));
    __builtin_amdgcn_s_barrier();
    if (kt + G::STAGES - 1 < nk) {
      const int nb = buf == 0 ? G::STAGES - 1 : buf - 1;  // buffer of step kt-1: every wave is past it
      stage(nb, kt + G::STAGES - 1);
    }
    const uint8_t* sw = q4_smem + buf * G::STAGE_BYTES;
    const uint8_t* ss = sw + Q4_W_BYTES;
    const uint8_t* sx = ss + Q4_S_BYTES;
    const uint32_t sc4 = *reinterpret_cast<const uint32_t*>(ss + w * 256 + fr * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = 2 * fh + i;  // 16-B code chunk = scale group of the step
      SHAI_DASSERT(wrow * 64 + ((c ^ wswz) << 4) + 16 <= Q4_W_BYTES);
      const uint4_ cw = *reinterpret_cast<const uint4_*>(sw + wrow * 64 + ((c ^ wswz) << 4));
      const float scale = q4_scale((sc4 >> (8 * c)) & 0xffu);
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // dword j of the chunk: k = 32 c + 8 j .. + 7 = X chunk 4 c + j
        const bf16x8q wf = q4_widen(cw[j], scale);
        const int xc = 4 * c + j;
#pragma unroll
        for (int g = 0; g < XG; ++g) {
          const int xrow = 32 * g + fr;
          const bf16x8q xf = *reinterpret_cast<const bf16x8q*>(sx + xrow * 256 + ((xc ^ (xrow & 15)) << 4));
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[g], 0, 0, 0);
          if constexpr (RMS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float f = (float)xf[e];
              ss2[g] = fmaf(f, f, ss2[g]);
            }
          }
        }
      }
    }
    buf = buf == G::STAGES - 1 ? 0 : buf + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (RMS) {  // both K halves of row m: lanes fr and fr + 32
#pragma unroll
    for (int g = 0; g < XG; ++g) ss2[g] += __shfl_xor(ss2[g], 32, 64);
  }
  const int nbase = n0 + 32 * w + 4 * fh;  // quad q of this lane: columns nbase + 8 q .. + 3
  if (KG == 1) {
#pragma unroll
    for (int g = 0; g < XG; ++g) {
      const float rs = RMS ? rsqrtf(ss2[g] / p.K + p.rms_eps) : 1.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[g][4 * q + e] * rs;
        q4_quad_out<GLU, ACT>(p, 32 * g + fr, nbase + 8 * q, v);
      }
    }
    return;
  }
  if (cnt == nullptr) {
    // ---- split-K over workgroups, separate fold: fp32 partials [kg][M][N] then [kg][M] row sums of squares;
    // launch_splitk_epilogue reduces them and runs the epilogue
    float* part = ws + (long)kg * p.M * p.N;
#pragma unroll
    for (int g = 0; g < XG; ++g) {
      const int m = 32 * g + fr;
      if (m >= p.M) continue;
      if constexpr (RMS) {
        if (tile == 0 && w == 0 && fh == 0) ws[(long)KG * p.M * p.N + (long)kg * p.M + m] = ss2[g];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = nbase + 8 * q;
        if (n >= p.N) continue;
        if (n + 3 < p.N && (p.N & 3) == 0) {
          *reinterpret_cast<float4_*>(part + (long)m * p.N + n) =
              float4_{acc[g][4 * q], acc[g][4 * q + 1], acc[g][4 * q + 2], acc[g][4 * q + 3]};
        } else {
          for (int e = 0; e < 4 && n + e < p.N; ++e) part[(long)m * p.N + n + e] = acc[g][4 * q + e];
        }
      }
    }
    return;
  }
  // ---- split-K fixed up in this launch: slab [tile][kg] = 4 XG chunks of 256 lanes x 4 floats (chunk = one quad
  // register group: coalesced 16-B stores / loads) + MB row sums of squares.  The write-through publish form of
  // gemv.hip: every slab byte stored sc1, EVERY wave drains vmcnt(0) before the workgroup barrier, one relaxed
  // agent-scope ticket; the last arriver re-arms the ticket and reads the slabs only with sc1 loads into registers.
  float v[XG][16];
#pragma unroll
  for (int g = 0; g < XG; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) v[g][r] = acc[g][r];
  const __amdgpu_buffer_rsrc_t rws = q4_rsrc(ws, 0x7fffffffu);
  const uint32_t tile_base = (uint32_t)((long)tile * KG * G::SLAB * 4);
  const uint32_t my_base = tile_base + (uint32_t)(kg * G::SLAB * 4);
  constexpr int NCH = 4 * XG;
  auto chunk_off = [&](int c) { return (uint32_t)((c * 256 + tid) * 16); };
#pragma unroll
  for (int c = 0; c < NCH; ++c) q4_store4_wt(rws, my_base + chunk_off(c), &v[c >> 2][(c & 3) * 4]);
  if constexpr (RMS) {
    if (w == 0 && fh == 0) {
#pragma unroll
      for (int g = 0; g < XG; ++g) q4_store_wt(rws, my_base + (uint32_t)((Q4_BN * MB + 32 * g + fr) * 4), ss2[g]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // also: every wave is done with the ring, its first word now carries the last-arriver flag
  unsigned* q4_last = reinterpret_cast<unsigned*>(q4_smem);
  if (tid == 0) {
    const unsigned old = __hip_atomic_fetch_add(&cnt[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    *q4_last = old == (unsigned)(KG - 1);
  }
  __syncthreads();
  if (*q4_last == 0u) return;
  if (tid == 0) __hip_atomic_store(&cnt[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // sum the KG slabs in K-group order (own slab from registers; two slabs' loads in flight before their adds): the
  // result does not depend on arrival order
  float sum[XG][16], ssum[XG];
#pragma unroll
  for (int g = 0; g < XG; ++g) {
    ssum[g] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[g][r] = 0.f;
  }
  for (int q0 = 0; q0 < KG; q0 += 2) {
    float t[2][XG][16], ts[2][XG];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = q0 + u < KG ? q0 + u : kg;  // past KG / own slot: re-read own slab, dropped below
      const uint32_t b = tile_base + (uint32_t)(q * G::SLAB * 4);
#pragma unroll
      for (int c = 0; c < NCH; ++c) q4_load4_wt(rws, b + chunk_off(c), &t[u][c >> 2][(c & 3) * 4]);
#pragma unroll
      for (int g = 0; g < XG; ++g) {
        ts[u][g] = 0.f;
        if constexpr (RMS) ts[u][g] = q4_load_wt(rws, b + (uint32_t)((Q4_BN * MB + 32 * g + fr) * 4));
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = q0 + u;
      if (q >= KG) continue;
      const bool mine = q == kg;
#pragma unroll
      for (int g = 0; g < XG; ++g) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sum[g][r] += mine ? v[g][r] : t[u][g][r];
        ssum[g] += mine ? ss2[g] : ts[u][g];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < XG; ++g) {
    const float rs = RMS ? rsqrtf(ssum[g] / p.K + p.rms_eps) : 1.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = sum[g][4 * q + e] * rs;
      q4_quad_out<GLU, ACT>(p, 32 * g + fr, nbase + 8 * q, o);
    }
  }
}

// MXFP4 codes + tiled scales -> bf16 [N, K] (prefill-shaped problems run the bf16 GEMMs on it): one thread per
// scale group (16 B of codes -> 64 B of bf16)
__global__ void __launch_bounds__(256) dequant_mxfp4_kernel(const uint8_t* __restrict__ wq,
                                                            const uint8_t* __restrict__ scales,
                                                            bf16_t* __restrict__ out, long groups, int KG32, long N) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < groups; i += (long)gridDim.x * blockDim.x) {
    const long n = i / KG32;
    const int g = (int)(i - n * KG32);
    const float scale = q4_scale(scales[((long)(g >> 2) * N + n) * 4 + (g & 3)]);
    const uint4_ cw = reinterpret_cast<const uint4_*>(wq)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x8q wf = q4_widen(cw[j], scale);
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
  return a.w_mx_scale != nullptr && a.w_scale == nullptr && !a.conv && a.batch <= 1 && a.w_slice_rows == 0 &&
         a.M >= 1 && a.M <= 64 && a.K >= 32 && a.K % 32 == 0 && a.N >= 1 && a.N % 2 == 0 && (!a.glu || a.N % 4 == 0) &&
         a.bias2d == nullptr && a.gate == nullptr && a.in_scale == nullptr && a.row_mr == nullptr &&
         a.col_part == nullptr && a.row_part == nullptr && a.lda % 8 == 0 && a.ldw % 16 == 0 && a.ldw >= a.K / 2 &&
         (long)a.N * a.ldw < 0x7fffffffL && (long)a.M * a.lda * 2 < 0x7fffffffL &&
         (long)((a.K + Q4_BK - 1) / Q4_BK) * a.N * 4 < 0x7fffffffL;
}

// K groups: about one workgroup per CU (two fit), each group at least 4 K steps
int skinny_fp4_kgroups(const GemmArgs& a) {
  const int tiles = (a.N + Q4_BN - 1) / Q4_BN, ksteps = (a.K + Q4_BK - 1) / Q4_BK;
  int kg = 1;
  while (tiles * kg < 256 && ksteps / (kg * 2) >= 4) kg *= 2;
  return kg;
}

int skinny_fp4_max_kgroups(const GemmArgs& a) {
  const int ksteps = (a.K + Q4_BK - 1) / Q4_BK;
  int kg = 1;
  while (kg < 16 && ksteps / (kg * 2) >= 2) kg *= 2;
  return kg;
}

size_t skinny_fp4_workspace_bytes(const GemmArgs& a, int kg) {
  if (kg <= 1) return 0;
  const size_t fold = (size_t)kg * a.M * a.N + (size_t)kg * a.M;  // [kg][M][N] + row sums of squares
  const int MB = a.M <= 32 ? 32 : 64;
  const size_t fix = (size_t)((a.N + Q4_BN - 1) / Q4_BN) * kg * (size_t)(Q4_BN * MB + MB);  // [tile][kg] slabs
  return (fold > fix ? fold : fix) * sizeof(float);
}

template <int MB>
static void launch_fp4_mb(const GemmArgs& a, float* ws, int kg, int kg_steps, unsigned* cnt, hipStream_t s) {
  dim3 grid((a.N + Q4_BN - 1) / Q4_BN, kg), block(Q4_WAVES * 64);
  const size_t lds = Q4Geom<MB>::LDS;
#define Q4(G, A)                                                                                  \
  do {                                                                                            \
    if (a.rms) skinny_fp4_kernel<MB, G, A, true><<<grid, block, lds, s>>>(a, ws, kg_steps, cnt);  \
    else skinny_fp4_kernel<MB, G, A, false><<<grid, block, lds, s>>>(a, ws, kg_steps, cnt);       \
  } while (0)
#define Q4_ACT(G)                                      \
  switch (a.act) {                                     \
    case ACT_SILU: Q4(G, ACT_SILU); break;             \
    case ACT_GELU: Q4(G, ACT_GELU); break;             \
    case ACT_GELU_TANH: Q4(G, ACT_GELU_TANH); break;   \
    case ACT_QUICK_GELU: Q4(G, ACT_QUICK_GELU); break; \
    case ACT_RELU: Q4(G, ACT_RELU); break;             \
    default: Q4(G, ACT_NONE); break;                   \
  }
  if (a.glu) {
    Q4_ACT(true)
  } else {
    Q4_ACT(false)
  }
#undef Q4_ACT
#undef Q4
}

// kg K groups (needs ws of skinny_fp4_workspace_bytes, else kg = 1); fixup: reduce the split-K partials inside the
// launch when a ticket slice is available, else (and without fixup) the separate fold kernel
void launch_skinny_fp4(const GemmArgs& a_in, float* ws, int kg, bool fixup, hipStream_t s) {
  static const int nt = [] {
    const char* e = getenv("SHAI_SKINNY_NT");
    return e ? atoi(e) : 1;
  }();
  GemmArgs a = a_in;
  a.w_nt = nt;
  const int ksteps = (a.K + Q4_BK - 1) / Q4_BK;
  const int tiles = (a.N + Q4_BN - 1) / Q4_BN;
  if (ws == nullptr || kg < 1) kg = 1;
  if (kg > ksteps) kg = ksteps;
  const int kg_steps = (ksteps + kg - 1) / kg;
  kg = (ksteps + kg_steps - 1) / kg_steps;  // no empty K groups
  unsigned* cnt = nullptr;
  const int slab = a.M <= 32 ? Q4Geom<32>::SLAB : Q4Geom<64>::SLAB;
  // (the slabs are addressed through one buffer descriptor: past 2 GiB the fold kernel takes the split)
  if (kg > 1 && fixup && (long)tiles * kg * slab * 4 < 0x7fffffffL) cnt = skinny_ticket_slice(s, tiles);
  if (a.M <= 32) launch_fp4_mb<32>(a, ws, kg, kg_steps, cnt, s);
  else launch_fp4_mb<64>(a, ws, kg, kg_steps, cnt, s);
  if (kg > 1 && cnt == nullptr) launch_splitk_epilogue(a, ws, kg, s);
}

}  // namespace shai

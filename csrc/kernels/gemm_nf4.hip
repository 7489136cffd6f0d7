// Tile GEMM over NF4 weights (the bitsandbytes 4-bit format) for problems of more than 64 activation rows (prefill,
// mixed steps, decode above 64 sequences):
//
//   C[m, n] = act(alpha * sum_k A[m, k] * What[n, k] + bias[n]) (+ res_alpha * R[m, n]),  GLU optional
//
// A is bf16 [M, K]; What = bf16_rne(fp32(NF4_TABLE[code]) * fp32(absmax)), the contract of gemv_nf4.hip: codes
// [N, K / 2] bytes (even k in the low nibble), absmax fp32 tiled [ceil(K / 128), N, 2], K % 64 == 0.  The kernel reads
// codes and absmax from HBM and never writes a bf16 weight: a code is widened in registers between ds_read and
// v_mfma_f32_32x32x16_bf16 (fp32 accumulation), so this kernel, the skinny kernel and the dequantise route multiply
// the same bf16 weights and differ in summation order only.
//
// Ring, DMA images and epilogue are those of gemm_fp4.hip: K step 128, everything by LDS-DMA through range-checked
// descriptors (rows >= M / N and whole chunks past K read as zeros), A rows of 16 chunks with chunk c at position
// c ^ row & 15, code rows of 4 chunks with chunk c at c ^ (row >> 2) & 3, counted vmcnt + one raw s_barrier per step,
// XCD-aware remap, grouped M order, epilogue4, split-K slabs [split][M][N] folded by launch_splitk_epilogue in split
// order.  Trip counts are uniform per workgroup.
//
// What differs is the wave layout, because the widening differs.  MXFP4 widens 8 codes with 4 converts; NF4 needs per
// code a table lookup, a shift, a v_mul_f32 by the fp32 absmax and half a v_cvt_pk_bf16_f32, and the lookup was the
// suspected limiter of the skinny kernel (profiles/nf4_decode.md).  So:
//
// * Waves striped over N, 1 x 4: wave w owns W rows [32 w, 32 w + 32) of a BM x 128 tile and ALL BM activation rows
//   (JN = 1, IM = BM / 32).  Every code of the tile is widened exactly once per workgroup, and a widened bf16x8
//   fragment feeds IM MFMAs: 4 at BM = 128, 8 at BM = 256 (the 2 x 2 layout of gemm_fp4.hip widens every code twice
//   and feeds 2 / 4).  The price is A fragment traffic: every wave reads the whole A image of the step.
//   By instruction count (a count, not a measurement), per CU and K step:
//       1 x 4:  256 wave64 lookups,  4 x BM x 256 B of A fragment reads (BM = 128: 128 KB, 1024 cycles at 128 B/cycle)
//       2 x 2:  512 wave64 lookups,  2 x BM x 256 B                      (BM = 128:  64 KB,  512 cycles)
//   The two tie if a wave64 lookup occupies the LDS pipe for 2 cycles and 1 x 4 wins if it takes more; the skinny
//   kernel's step time suggested about 10.  Neither confirmed nor contradicted so far: no 2 x 2 NF4 kernel and no
//   counter run exist to set beside this one (profiles/nf4_prefill.md).
// * Block ownership of the skinny kernel: K step 128 = two NF4 blocks, lane (fr, fh) of the MFMA layout owns block fh
//   of W row 32 w + fr, so ONE absmax serves its 64 codes of a step.  The wave's absmax arrive with one 4-B DMA
//   instruction, all 64 lanes live: lane l = (row 32 w + (l >> 1), block l & 1).
// * Lane (fr, fh) reads the code chunks 2 fh, 2 fh + 1 of its row; slice g = 4 i + j widens dword j of chunk
//   c = 2 fh + i (k = 32 c + 8 j .. + 7) against A chunk 4 c + j of rows 32 im + fr: K is consumed in a permuted order
//   inside the step, as in gemv_nf4.hip.
// * The widening is software-pipelined against the MFMAs: the 8 lookups of slice g + 1 (and its A fragments) are
//   issued before slice g's IM MFMAs, their multiply / convert after, so the lookup's round trip hides under 4-8
//   MFMAs (one wave per SIMD: nobody else hides it).
// * The lookup reads a 16-dword fp32 table at the start of this kernel's LDS object with ds_read_b32 (equal codes
//   broadcast, different codes hit different banks); the ring starts behind it.  A zero-filled code (rows >= N, K
//   tail) widens to TABLE[0] * absmax = -absmax with a zero-filled / stored-zero absmax, beside zero-filled A.
//
// Tile configs (the LDS budget of gemm_fp4.hip):
//   tile 0  128 x 128, 3 stages x (32 KB A + 8 KB codes + 1 KB absmax) = 123 KB, 64 accumulators per lane, IM = 4
//   tile 1  256 x 128, 2 stages x (64 + 8 + 1 KB) = 146 KB, 128 accumulators per lane, IM = 8
// Resource table and measurements: profiles/nf4_prefill.md.
#include "q4_tile.h"

namespace shai {

constexpr int GN_BK = 128;                 // K per step (two NF4 blocks)
constexpr int GN_BN = 128;                 // W rows per tile: 4 waves x 32
constexpr int GN_A_ROW = GN_BK * 2;        // bytes of A per row and step
constexpr int GN_W_ROW = GN_BK / 2;        // bytes of codes per row and step
constexpr int GN_TAB = 64;                 // the fp32 lookup table in front of the ring

template <int BM, int STAGES>
struct GnGeom {
  static constexpr int A_BYTES = BM * GN_A_ROW;
  static constexpr int W_BYTES = GN_BN * GN_W_ROW;
  static constexpr int S_BYTES = 4 * 256;       // one 64-lane x 4-B DMA per wave: 32 rows x 2 blocks of fp32
  static constexpr int STAGE = A_BYTES + W_BYTES + S_BYTES;
  static constexpr size_t LDS = GN_TAB + (size_t)STAGES * STAGE;
};

// the eight lookups of one code dword (even k in the low nibbles): byte address code * 4 into the LDS table
__device__ __forceinline__ void nf4x8_lookup(const uint8_t* tab, uint32_t codes, float v[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t addr = (i == 0 ? codes << 2 : codes >> (4 * i - 2)) & 0x3cu;
    v[i] = *reinterpret_cast<const float*>(tab + addr);
  }
}
// ... and their fp32 product with the block's absmax, rounded once to bf16
__device__ __forceinline__ bf16x8 nf4x8_scale(const float v[8], float absmax) {
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = (__bf16)(v[i] * absmax);
  return r;
}

// Accumulator layout (W rows as A, activation rows as B): lane (fr = lane & 31, fh = lane >> 5) holds D[n][m] for
// m = fr and n = 8 q + 4 fh + e in register 4 q + e: quads of 4 consecutive n, the layout epilogue4 takes.
// RMS (folded RMSNorm, C = rstd[m] * ...): wave w sums the squares of the A fragments of row blocks im = w (mod 4) as
// it reads them (lanes fr, fr + 32 together see every element of a row once per step), the waves exchange the row sums
// through the dead ring after the K loop, and rstd is applied in fp32 in front of the epilogue -- the activations are
// never rounded a second time.  Split-K: the partial row sums follow the [split][M][N] block, as the skinny kernel has it.
template <int BM, int STAGES, bool GLU, int ACT, bool RMS, bool SPLITK>
__global__ void __launch_bounds__(256) gemm_nf4_kernel(const GemmArgs p, float* __restrict__ ws, int kg_steps) {
  using G = GnGeom<BM, STAGES>;
  constexpr int IM = BM / 32;
  constexpr int SQ = IM / 4;  // row blocks whose sum of squares this wave accumulates
  static_assert(IM % 4 == 0, "the row blocks divide over the four waves");
  constexpr int JA = BM / 16, JW = 2;  // A / code DMA wave-instructions per wave and K step
  constexpr int PER = JA + JW + 1;
  static_assert(IM >= 4 && (JA * 4) % 16 == 0, "a wave's A rows start on a swizzle period");
  static_assert(G::LDS <= 160 * 1024 && PER * (STAGES - 1) < 64, "LDS budget, vmcnt range");
  // one LDS object only (gemv_fp4.hip: a second one beside a DMA ring can make the compiler drain vmcnt per step)
  extern __shared__ __attribute__((aligned(16))) uint8_t gn_smem[];
  uint8_t* const ring = gn_smem + GN_TAB;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + GN_BN - 1) / GN_BN;
  const int total = tiles_m * tiles_n;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = total >> 3, r = total & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  constexpr int GROUP = 8;
  const int group = bid / (GROUP * tiles_n);
  const int first_m = group * GROUP;
  const int gsize = min(tiles_m - first_m, GROUP);
  const int in_group = bid - group * GROUP * tiles_n;
  const int m0 = (first_m + in_group % gsize) * BM;
  const int n0 = (in_group / gsize) * GN_BN;

  const int ksteps = (p.K + GN_BK - 1) / GN_BK;
  const int t0 = SPLITK ? (int)blockIdx.y * kg_steps : 0;
  const int nk = SPLITK ? max(0, min(ksteps, t0 + kg_steps) - t0) : ksteps;

  const long a_bytes = (long)p.M * p.lda * 2, w_bytes = (long)p.N * p.ldw, s_bytes = (long)ksteps * p.N * 8;
  const __amdgpu_buffer_rsrc_t rA = buf_rsrc(p.A, a_bytes);
  const __amdgpu_buffer_rsrc_t rW = buf_rsrc(p.W, w_bytes);  // ldw: bytes
  const __amdgpu_buffer_rsrc_t rS = buf_rsrc(p.w_nf4_absmax, s_bytes);

  if (tid < 16) reinterpret_cast<float*>(gn_smem)[tid] = nf4_table_entry(tid);  // published by the first barrier

  // DMA geometry: LDS images are lane-linear per wave instruction, the swizzle is on the source address
  uint32_t a_off[JA], w_off[JW];
#pragma unroll
  for (int j = 0; j < JA; ++j) {  // instruction wid JA + j: tile rows 4 (wid JA + j) + (lane >> 4), position lane & 15
    const int r = 4 * (wid * JA + j) + (lane >> 4), m = m0 + r;
    const int c = (lane & 15) ^ (r & 15);
    a_off[j] = m < p.M ? (uint32_t)(((long)m * p.lda + c * 8) * 2) : kDmaOob;
  }
#pragma unroll
  for (int j = 0; j < JW; ++j) {  // instruction wid JW + j: tile rows 16 (wid JW + j) + (lane >> 2), position lane & 3
    const int r = 16 * (wid * JW + j) + (lane >> 2), n = n0 + r;
    const int c = (lane & 3) ^ ((r >> 2) & 3);
    w_off[j] = n < p.N ? (uint32_t)((long)n * p.ldw + c * 16) : kDmaOob;
  }
  // absmax: lane l fetches block l & 1 of tile row 32 wid + (l >> 1)
  const uint32_t s_off =
      n0 + 32 * wid + (lane >> 1) < p.N ? (uint32_t)((n0 + 32 * wid + (lane >> 1)) * 8 + (lane & 1) * 4) : kDmaOob;

  auto stage = [&](int buf, int step) {
    SHAI_DASSERT(buf >= 0 && buf < STAGES);
    uint8_t* sa = ring + buf * G::STAGE;
    uint8_t* sw = sa + G::A_BYTES;
    uint8_t* ss = sw + G::W_BYTES;
    const uint32_t k0 = (uint32_t)(t0 + step) * GN_BK;
#pragma unroll
    for (int j = 0; j < JW; ++j) {  // K tail: whole 32-code chunks past K read as zeros (K % 64 == 0)
      const int c = (lane & 3) ^ (((16 * (wid * JW + j) + (lane >> 2)) >> 2) & 3);
      const uint32_t off = (w_off[j] != kDmaOob && k0 + c * 32 < (uint32_t)p.K) ? w_off[j] + (k0 >> 1) : kDmaOob;
      SHAI_DASSERT_DMA(off, w_bytes, kDmaOob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (wid * JW + j) * 1024), 16, off, 0, 0, 0);
    }
    {
      const uint32_t off = s_off != kDmaOob ? s_off + (uint32_t)(t0 + step) * (uint32_t)p.N * 8u : kDmaOob;
      SHAI_DASSERT(off >= kDmaOob || (long)off + 4 <= s_bytes);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rS, (lds_void*)(ss + wid * 256), 4, off, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < JA; ++j) {
      const int c = (lane & 15) ^ ((4 * j + (lane >> 4)) & 15);  // (4 wid JA) % 16 == 0
      const uint32_t off = (a_off[j] != kDmaOob && k0 + c * 8 < (uint32_t)p.K) ? a_off[j] + k0 * 2 : kDmaOob;
      SHAI_DASSERT_DMA(off, a_bytes, kDmaOob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_void*)(sa + (wid * JA + j) * 1024), 16, off, 0, 0, 0);
    }
  };

  float16_ acc[IM];
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  float sq[SQ];  // RMS: this lane's share of sum_k A[m, k]^2 for m = 32 (4 q + wid) + fr
#pragma unroll
  for (int q = 0; q < SQ; ++q) sq[q] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;
  auto compute = [&](int buf) {
    SHAI_DASSERT(buf >= 0 && buf < STAGES);
    const uint8_t* sa = ring + buf * G::STAGE;
    const uint8_t* sw = sa + G::A_BYTES;
    const uint8_t* ss = sw + G::W_BYTES;
    const int wrow = 32 * wid + fr, wswz = (wrow >> 2) & 3;
    const float am = *reinterpret_cast<const float*>(ss + wid * 256 + fr * 8 + fh * 4);  // block fh of the step
    uint4_ cw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = 2 * fh + i;  // 16-B code chunk, half of the lane's block
      SHAI_DASSERT(wrow * GN_W_ROW + ((c ^ wswz) << 4) + 16 <= G::W_BYTES);
      cw[i] = *reinterpret_cast<const uint4_*>(sw + wrow * GN_W_ROW + ((c ^ wswz) << 4));
    }
    auto load_x = [&](int g, bf16x8* xf) {
      const int xc = 4 * (2 * fh + (g >> 2)) + (g & 3);
#pragma unroll
      for (int im = 0; im < IM; ++im) {
        const int xrow = im * 32 + fr;
        SHAI_DASSERT(xrow * GN_A_ROW + ((xc ^ (xrow & 15)) << 4) + 16 <= G::A_BYTES);
        xf[im] = *reinterpret_cast<const bf16x8*>(sa + xrow * GN_A_ROW + ((xc ^ (xrow & 15)) << 4));
      }
    };
    // 8 slices of IM MFMAs.  Slice g + 1's lookups and A fragments are issued before slice g's MFMAs, its multiply /
    // convert after them.
    float v[8];
    bf16x8 xf[2][IM];
    nf4x8_lookup(gn_smem, cw[0][0], v);
    load_x(0, xf[0]);
    bf16x8 wf = nf4x8_scale(v, am);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (g + 1 < 8) {
        nf4x8_lookup(gn_smem, cw[(g + 1) >> 2][(g + 1) & 3], v);
        load_x(g + 1, xf[(g + 1) & 1]);
      }
#pragma unroll
      for (int im = 0; im < IM; ++im)
        acc[im] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf[g & 1][im], acc[im], 0, 0, 0);
      if constexpr (RMS) {
#pragma unroll
        for (int im = 0; im < IM; ++im)
          if ((im & 3) == wid) {
            const bf16x8 x = xf[g & 1][im];
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
              const bf16x2 x2 = {x[e], x[e + 1]};
              sq[im >> 2] = __builtin_amdgcn_fdot2_f32_bf16(x2, x2, sq[im >> 2], false);
            }
          }
      }
      if (g + 1 < 8) wf = nf4x8_scale(v, am);
    }
  };

  if constexpr (STAGES == 3) {
    // steps t+1 and t+2 in flight while step t is consumed (counted vmcnt retires this wave's DMA of step t; the raw
    // barrier publishes every wave's part and frees step t-1's buffer for step t+2)
    if (nk > 0) stage(0, 0);
    if (nk > 1) stage(1, 1);
    int buf = 0;
    for (int kt = 0; kt < nk; ++kt) {
      // (lgkmcnt(0): this wave's fragment reads of step t-1 have returned before its buffer is handed back; at the
      // first step it retires the table's store)
      if (kt + 1 < nk && !SHAI_DEBUG) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PER) : "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 2 < nk) stage(buf == 0 ? 2 : buf - 1, kt + 2);
      compute(buf);
      buf = buf == 2 ? 0 : buf + 1;
    }
  } else {
    // two stages (the 256-row tile: 146 KB): step t+1's DMA issued before step t's MFMAs
    static_assert(STAGES == 2, "2 or 3 stages");
    if (nk > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // (lgkmcnt: the table's store)
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
      compute(kt & 1);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // DMA landed, fragment reads returned
      __builtin_amdgcn_s_barrier();
    }
  }

  float rowsq[IM];  // RMS: sum_k A[m, k]^2 of this workgroup's K range, m = 32 i + fr
  if constexpr (RMS) {
    __syncthreads();  // every wave is past its last fragment read: the ring is free
    float* xs = reinterpret_cast<float*>(ring);
#pragma unroll
    for (int q = 0; q < SQ; ++q) {
      const float t = sq[q] + __shfl_xor(sq[q], 32, 64);  // both K halves of the row
      if (fh == 0) xs[(4 * q + wid) * 32 + fr] = t;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IM; ++i) rowsq[i] = xs[i * 32 + fr];
  }

  // epilogue: lane owns row m, 4 quads of 4 consecutive n of the wave's 32 W rows
#pragma unroll
  for (int i = 0; i < IM; ++i) {
    const int m = m0 + i * 32 + fr;
    if (m >= p.M) continue;
    float rs = 1.f;
    if constexpr (RMS) {
      if constexpr (SPLITK) {  // [split][M] partial row sums behind the [split][M][N] block
        if (n0 == 0 && wid == 0 && fh == 0) ws[(long)gridDim.y * p.M * p.N + (long)blockIdx.y * p.M + m] = rowsq[i];
      } else {
        rs = rsqrtf(rowsq[i] / p.K + p.rms_eps);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = n0 + 32 * wid + 8 * g + 4 * fh;
      if (n >= p.N) continue;
      if constexpr (SPLITK) {  // fp32 partials [split][M][N]
        float* part = ws + ((long)blockIdx.y * p.M + m) * p.N + n;
        if (n + 3 < p.N && (p.N & 3) == 0) {
          *reinterpret_cast<float4_*>(part) = float4_{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
        } else {
          for (int e = 0; e < 4 && n + e < p.N; ++e) part[e] = acc[i][4 * g + e];
        }
      } else {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][4 * g + e] * rs;
        epilogue4<GLU, ACT>(p, p.C, p.residual, m, n, v, 0);
      }
    }
  }
}

// ---------------------------------------------------------------------------- host side
// a.W: codes [N, K / 2] bytes at a row stride of a.ldw BYTES; a.w_nf4_absmax: [ceil(K / 128), N, 2] fp32.  Epilogues:
// bias, activation, GLU (SILU / GELU / GELU_TANH), residual, alpha, row strides, folded RMSNorm (a.rms: rstd in fp32 in
// front of the epilogue; an explicit row-norm pass would round the normalised activations to bf16, 1.3 ulp of error in
// a GLU output where the skinny kernel's rule allows 1).
static bool gemm_nf4_supported(const GemmArgs& a) {
  return a.w_nf4_absmax != nullptr && a.w_mx_scale == nullptr && q4t_supported(a, 64, 8);
}

static size_t gemm_nf4_workspace_bytes(const GemmArgs& a, int splits) {
  // [split][M][N], then [split][M] partial row sums of squares under a folded RMSNorm
  return splits > 1 ? ((size_t)splits * a.M * a.N + (a.rms ? (size_t)splits * a.M : 0)) * sizeof(float) : 0;
}

template <int BM, int STAGES>
static void launch_gn_tile(const GemmArgs& a, float* ws, int splits, int kg_steps, hipStream_t s) {
  const int tiles = ((a.M + BM - 1) / BM) * ((a.N + GN_BN - 1) / GN_BN);
  const size_t lds = GnGeom<BM, STAGES>::LDS;
  if (splits > 1) {
    const dim3 grid(tiles, splits);
    if (a.rms) gemm_nf4_kernel<BM, STAGES, false, ACT_NONE, true, true><<<grid, 256, lds, s>>>(a, ws, kg_steps);
    else gemm_nf4_kernel<BM, STAGES, false, ACT_NONE, false, true><<<grid, 256, lds, s>>>(a, ws, kg_steps);
    return;
  }
  // GLU: tile_act_supported admits SILU / GELU / GELU_TANH only
  constexpr unsigned kGluActs = act_bit(ACT_SILU) | act_bit(ACT_GELU) | act_bit(ACT_GELU_TANH);
  dispatch_epilogue<kActsAll, kGluActs, ACT_GELU>(a, [&](auto glu, auto act, auto rms) {
    gemm_nf4_kernel<BM, STAGES, glu(), act(), rms(), false><<<dim3(tiles), 256, lds, s>>>(a, nullptr, 0);
  });
}

static void launch_gemm_nf4(const GemmArgs& a, float* ws, int tile, int splits, hipStream_t s) {
  q4t_launch(a, ws, tile, splits, s, [&](int t, int kg, int kg_steps) {
    if (t == 1) launch_gn_tile<256, 2>(a, ws, kg, kg_steps, s);
    else launch_gn_tile<128, 3>(a, ws, kg, kg_steps, s);
  });
}

const Q4TileOps& nf4_tile_ops() {
  static const Q4TileOps ops = {gemm_nf4_supported,       q4t_tile,       q4t_splits, q4t_max_splits,
                                gemm_nf4_workspace_bytes, launch_gemm_nf4};
  return ops;
}

}  // namespace shai

// Tile GEMM over MXFP4 weights for problems of more than 64 activation rows (prefill, decode above 64 sequences):
//
//   C[m, n] = act(alpha * sum_k A[m, k] * What[n, k] + bias[n]) (+ res_alpha * R[m, n]),  GLU optional
//
// A is bf16 [M, K]; What = code * 2^(scale - 127) in the format of gemv_fp4.hip (e2m1 codes [N, K / 2] bytes, even k in
// the low nibble; e8m0 scales tiled [ceil(K / 128), N, 4]).  Weight-only and exact: every code is widened to bf16
// with its group scale (code * power of two is exact in bf16) and multiplied with the bf16 activations on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- the arithmetic of gemv_fp4.hip and of the dequantise route, so
// the three differ in summation order only.  The kernel reads codes and scales from HBM and never writes a bf16
// weight: widening happens in registers between ds_read and MFMA.
//
// Structure (the LDS-DMA tile GEMM of gemm_f8.hip with the fragment of gemv_fp4.hip):
// * K step = 128 = 4 scale groups.  Per step and row: A 256 B, codes 64 B, scales one dword.  A stage of a
//   BM x BN tile is BM * 256 + BN * 64 + 1 KB: the bf16 activations are 4 / 5 of the LDS image, which is what bounds
//   the tile (160 KB of LDS per CU), not the weights.
// * Everything arrives by LDS-DMA (range-checked descriptors: rows >= M / N and whole 16-B chunks past K read as
//   zeros, K % 32 == 0).  LDS images are those of gemv_fp4.hip: A rows of 16 chunks, chunk c at position c ^ row & 15
//   (4 rows per wave instruction); code rows of 4 chunks, chunk c at position c ^ (row >> 2) & 3 (16 rows per
//   instruction); wave w fetches the scale dwords of W rows [32 w, 32 w + 32) with one 4-B instruction (lanes 32-63
//   out of range).  The scale tile is padded to whole dwords by the quantiser, so the last step's dword exists.
// * Wave tile TM x TN of 32 x 32 blocks, W rows as the MFMA's A operand: lane (fr, fh) reads the code chunks 2 fh,
//   2 fh + 1 of its W row (each one scale group) and widens each dword (8 codes = its 8 k of one 32x32x16 fragment)
//   with four v_cvt_scalef32_pk_bf16_fp4; the A fragment holding the same k is one 16-B chunk.  K is consumed in a
//   permuted order inside the step, as in gemv_fp4.hip.  A step is 8 groups of IM x JN MFMAs; the A fragments of the
//   next group are read before the current group's MFMAs (one wave per SIMD: nobody else hides the LDS latency).
// * Ring of STAGES stages, counted vmcnt + raw s_barrier (gemm_f8.hip; lgkmcnt(0) rides on the wait, so a buffer is
//   handed back only after this wave's fragment reads returned), XCD-aware remap, grouped M order.
// * Split-K over gridDim.y: fp32 partials [split][M][N] folded by launch_splitk_epilogue in split order.
//
// Tile configs (4 waves as 2 x 2; converts : MFMAs counts v_cvt_scalef32_pk_bf16_fp4 against v_mfma per wave):
//   tile 0  128 x 128, wave tile  64 x 64, 3 stages x 41 KB = 123 KB: every widened fragment feeds 2 MFMAs,
//           converts : MFMAs = 2 : 1, 0.69 ds_read per MFMA.  The fill-bound config: M 65..256 x N 4096 = 32-64 tiles,
//           split-K fills the 256 CUs.
//   tile 1  256 x 128, wave tile 128 x 64, 2 stages x 73 KB = 146 KB: every widened fragment feeds 4 MFMAs,
//           converts : MFMAs = 1 : 1, 0.59 ds_read per MFMA.  Long prefill.
// (A 256 x 256 tile would need 2 x 81 KB of LDS; wider N at BM = 128 doubles the converts per CU for the same MFMAs.)
// Resource table and measurements: profiles/mxfp4_prefill.md.
// (buffer descriptor, zero-fill sentinel, e8m0_scale and fp4x8_widen: skinny_common.h, shared with gemv_fp4.hip)
#include "skinny_common.h"

namespace shai {

constexpr int G4_BK = 128;                 // K per step (4 scale groups)
constexpr int G4_A_ROW = G4_BK * 2;        // bytes of A per row and step
constexpr int G4_W_ROW = G4_BK / 2;        // bytes of codes per row and step

template <int BM, int BN, int WM, int WN, int STAGES>
struct G4Geom {
  static constexpr int NW = WM * WN;
  static constexpr int A_BYTES = BM * G4_A_ROW;
  static constexpr int W_BYTES = BN * G4_W_ROW;
  static constexpr int S_BYTES = NW * 256;      // one 64-lane x 4-B DMA per wave (upper 32 lanes zero fill)
  static constexpr int STAGE = A_BYTES + W_BYTES + S_BYTES;
  static constexpr size_t LDS = (size_t)STAGES * STAGE;
};

// Accumulator layout (W rows as A, activation rows as B): lane (fr = lane & 31, fh = lane >> 5) holds D[n][m] for
// m = fr and n = 8 q + 4 fh + e in register 4 q + e: quads of 4 consecutive n, the layout epilogue4 takes.
template <int BM, int BN, int WM, int WN, int STAGES, bool GLU, int ACT, bool SPLITK>
__global__ void __launch_bounds__(WM * WN * 64) gemm_fp4_kernel(const GemmArgs p, float* __restrict__ ws,
                                                                int kg_steps) {
  using G = G4Geom<BM, BN, WM, WN, STAGES>;
  constexpr int NW = G::NW;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int IM = TM / 32, JN = TN / 32;
  constexpr int JA = BM / 4 / NW, JW = BN / 16 / NW;  // A / code DMA wave-instructions per K step
  constexpr int PER = JA + JW + 1;
  static_assert(BN == 32 * NW, "one scale DMA per wave covers 32 W rows");
  static_assert(JA >= 1 && JW >= 1 && IM >= 2 && JN >= 1, "bad tile config (a widened fragment feeds >= 2 MFMAs)");
  static_assert((JA * 4) % 16 == 0, "a wave's A rows start on a swizzle period");
  // one LDS object only (gemv_fp4.hip: a second one beside a DMA ring can make the compiler drain vmcnt per step)
  extern __shared__ __attribute__((aligned(16))) uint8_t g4_smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;

  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
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
  const int n0 = (in_group / gsize) * BN;

  const int ksteps = (p.K + G4_BK - 1) / G4_BK;
  const int t0 = SPLITK ? (int)blockIdx.y * kg_steps : 0;
  const int nk = SPLITK ? max(0, min(ksteps, t0 + kg_steps) - t0) : ksteps;

  const long a_bytes = (long)p.M * p.lda * 2, w_bytes = (long)p.N * p.ldw, s_bytes = (long)ksteps * p.N * 4;
  const __amdgpu_buffer_rsrc_t rA = buf_rsrc(p.A, a_bytes);
  const __amdgpu_buffer_rsrc_t rW = buf_rsrc(p.W, w_bytes);  // ldw: bytes
  const __amdgpu_buffer_rsrc_t rS = buf_rsrc(p.w_mx_scale, s_bytes);

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
  // scales: lanes 0-31 fetch the dword of tile row 32 wid + lane
  const uint32_t s_off = (lane < 32 && n0 + 32 * wid + lane < p.N) ? (uint32_t)((n0 + 32 * wid + lane) * 4) : kDmaOob;

  auto stage = [&](int buf, int step) {
    SHAI_DASSERT(buf >= 0 && buf < STAGES);
    uint8_t* sa = g4_smem + buf * G::STAGE;
    uint8_t* sw = sa + G::A_BYTES;
    uint8_t* ss = sw + G::W_BYTES;
    const uint32_t k0 = (uint32_t)(t0 + step) * G4_BK;
#pragma unroll
    for (int j = 0; j < JW; ++j) {  // K tail: whole 32-code chunks past K read as zeros
      const int c = (lane & 3) ^ (((16 * (wid * JW + j) + (lane >> 2)) >> 2) & 3);
      const uint32_t off = (w_off[j] != kDmaOob && k0 + c * 32 < (uint32_t)p.K) ? w_off[j] + (k0 >> 1) : kDmaOob;
      SHAI_DASSERT_DMA(off, w_bytes, kDmaOob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (wid * JW + j) * 1024), 16, off, 0, 0, 0);
    }
    {
      const uint32_t off = s_off != kDmaOob ? s_off + (uint32_t)(t0 + step) * (uint32_t)p.N * 4u : kDmaOob;
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

  float16_ acc[IM][JN];
#pragma unroll
  for (int i = 0; i < IM; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;
  auto compute = [&](int buf) {
    SHAI_DASSERT(buf >= 0 && buf < STAGES);
    const uint8_t* sa = g4_smem + buf * G::STAGE;
    const uint8_t* sw = sa + G::A_BYTES;
    const uint8_t* ss = sw + G::W_BYTES;
    uint4_ cw[JN][2];
    float sc[JN][2];
#pragma unroll
    for (int jn = 0; jn < JN; ++jn) {
      const int wrow = wn * TN + jn * 32 + fr, wswz = (wrow >> 2) & 3;
      const uint32_t sc4 = *reinterpret_cast<const uint32_t*>(ss + (wrow >> 5) * 256 + (wrow & 31) * 4);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = 2 * fh + i;  // 16-B code chunk = scale group of the step
        SHAI_DASSERT(wrow * G4_W_ROW + ((c ^ wswz) << 4) + 16 <= G::W_BYTES);
        cw[jn][i] = *reinterpret_cast<const uint4_*>(sw + wrow * G4_W_ROW + ((c ^ wswz) << 4));
        sc[jn][i] = e8m0_scale((sc4 >> (8 * c)) & 0xffu);
      }
    }
    // 8 groups of IM x JN MFMAs: group g = 4 i + j takes dword j of code chunk c = 2 fh + i (k = 32 c + 8 j .. + 7)
    // against A chunk 4 c + j.  The A fragments of group g + 1 are read before group g's MFMAs issue, so one wave per
    // SIMD does not sit out the LDS latency between groups.
    auto load_x = [&](int g, bf16x8* xf) {
      const int xc = 4 * (2 * fh + (g >> 2)) + (g & 3);
#pragma unroll
      for (int im = 0; im < IM; ++im) {
        const int xrow = wm * TM + im * 32 + fr;
        SHAI_DASSERT(xrow * G4_A_ROW + ((xc ^ (xrow & 15)) << 4) + 16 <= G::A_BYTES);
        xf[im] = *reinterpret_cast<const bf16x8*>(sa + xrow * G4_A_ROW + ((xc ^ (xrow & 15)) << 4));
      }
    };
    bf16x8 xf[2][IM];
    load_x(0, xf[0]);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (g + 1 < 8) load_x(g + 1, xf[(g + 1) & 1]);
#pragma unroll
      for (int jn = 0; jn < JN; ++jn) {
        const bf16x8 wf = fp4x8_widen(cw[jn][g >> 2][g & 3], sc[jn][g >> 2]);
#pragma unroll
        for (int im = 0; im < IM; ++im)
          acc[im][jn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf[g & 1][im], acc[im][jn], 0, 0, 0);
      }
    }
  };

  if constexpr (STAGES == 3) {
    // steps t+1 and t+2 in flight while step t is consumed (counted vmcnt retires this wave's DMA of step t; the raw
    // barrier publishes every wave's part and frees step t-1's buffer for step t+2)
    if (nk > 0) stage(0, 0);
    if (nk > 1) stage(1, 1);
    int buf = 0;
    for (int kt = 0; kt < nk; ++kt) {
      // (lgkmcnt(0): this wave's fragment reads of step t-1 have returned before its buffer is handed back)
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
      compute(kt & 1);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // DMA landed, fragment reads returned
      __builtin_amdgcn_s_barrier();
    }
  }

  // epilogue: lane owns row m, 4 quads of 4 consecutive n per 32 x 32 block
#pragma unroll
  for (int i = 0; i < IM; ++i) {
    const int m = m0 + wm * TM + i * 32 + fr;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * TN + j * 32 + 8 * g + 4 * fh;
        if (n >= p.N) continue;
        if constexpr (SPLITK) {  // fp32 partials [split][M][N]
          float* part = ws + ((long)blockIdx.y * p.M + m) * p.N + n;
          if (n + 3 < p.N && (p.N & 3) == 0) {
            *reinterpret_cast<float4_*>(part) =
                float4_{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          } else {
            for (int e = 0; e < 4 && n + e < p.N; ++e) part[e] = acc[i][j][4 * g + e];
          }
        } else {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e];
          epilogue4<GLU, ACT>(p, p.C, p.residual, m, n, v, 0);
        }
      }
  }
}

// ---------------------------------------------------------------------------- host side
// a.W: codes [N, K / 2] bytes at a row stride of a.ldw BYTES; a.w_mx_scale: [ceil(K / 128), N, 4] bytes.  Epilogues:
// bias, activation, GLU (SILU / GELU / GELU_TANH), residual, alpha, row strides.  A folded RMSNorm (a.rms) is not
// taken: the caller runs the unweighted row-norm pass first, as the bf16 tile kernels have it.
bool gemm_fp4_supported(const GemmArgs& a) {
  if (a.res_rows != 0) return false;  // no broadcast residual
  return a.w_mx_scale != nullptr && a.w_scale == nullptr && !a.conv && a.batch <= 1 && a.w_slice_rows == 0 &&
         a.M > 64 && a.K >= 32 && a.K % 32 == 0 && a.N >= 1 && a.N % 2 == 0 && (!a.glu || a.N % 4 == 0) &&
         tile_act_supported(a) && !a.rms && a.bias2d == nullptr && a.gate == nullptr && a.in_scale == nullptr &&
         a.A2 == nullptr && a.row_mr == nullptr && a.col_part == nullptr && a.row_part == nullptr &&
         a.lda % 8 == 0 && a.ldw % 16 == 0 && a.ldw >= a.K / 2 && (long)a.N * a.ldw < 0x7fffffffL &&
         (long)a.M * a.lda * 2 < 0x7fffffffL && (long)((a.K + G4_BK - 1) / G4_BK) * a.N * 4 < 0x7fffffffL;
}

int gemm_fp4_num_tiles() { return 2; }

static void g4_tile_dims(int tile, int* bm, int* bn) {
  *bm = tile == 1 ? 256 : 128;
  *bn = 128;
}

// heuristic tile: the 256-row tile once it alone gives every CU a workgroup
int gemm_fp4_tile(const GemmArgs& a) { return (long)((a.M + 255) / 256) * ((a.N + 127) / 128) >= 256 ? 1 : 0; }

// heuristic split count: up to one workgroup per CU (one fits), each split at least 4 K steps
int gemm_fp4_splits(const GemmArgs& a, int tile) {
  int bm, bn;
  g4_tile_dims(tile, &bm, &bn);
  const long tiles = (long)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn);
  const int ksteps = (a.K + G4_BK - 1) / G4_BK;
  int s = 1;
  while (s < 16 && tiles * s * 2 <= 256 && ksteps / (s * 2) >= 4) s *= 2;
  return s;
}

int gemm_fp4_max_splits(const GemmArgs& a) { return max_kgroups((a.K + G4_BK - 1) / G4_BK); }

size_t gemm_fp4_workspace_bytes(const GemmArgs& a, int splits) {
  return splits > 1 ? (size_t)splits * a.M * a.N * sizeof(float) : 0;  // [split][M][N]
}

template <int BM, int BN, int WM, int WN, int STAGES>
static void launch_g4_tile(const GemmArgs& a, float* ws, int splits, int kg_steps, hipStream_t s) {
  const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
  const size_t lds = G4Geom<BM, BN, WM, WN, STAGES>::LDS;
  const dim3 block(WM * WN * 64);
  if (splits > 1) {
    gemm_fp4_kernel<BM, BN, WM, WN, STAGES, false, ACT_NONE, true><<<dim3(tiles, splits), block, lds, s>>>(a, ws, kg_steps);
    return;
  }
  // GLU: tile_act_supported admits SILU / GELU / GELU_TANH only; no folded-RMSNorm forms
  constexpr unsigned kGluActs = act_bit(ACT_SILU) | act_bit(ACT_GELU) | act_bit(ACT_GELU_TANH);
  dispatch_epilogue<kActsAll, kGluActs, ACT_GELU, false>(a, [&](auto glu, auto act, auto) {
    gemm_fp4_kernel<BM, BN, WM, WN, STAGES, glu(), act(), false><<<dim3(tiles), block, lds, s>>>(a, nullptr, 0);
  });
}

// tile: 0 = 128 x 128, 1 = 256 x 128; splits K groups (needs ws of gemm_fp4_workspace_bytes, else unsplit), folded by
// launch_splitk_epilogue in split order
void launch_gemm_fp4(const GemmArgs& a, float* ws, int tile, int splits, hipStream_t s) {
  const KSplit ks = split_ksteps((a.K + G4_BK - 1) / G4_BK, ws != nullptr ? splits : 1);
  if (tile == 1) launch_g4_tile<256, 128, 2, 2, 2>(a, ws, ks.kg, ks.kg_steps, s);
  else launch_g4_tile<128, 128, 2, 2, 3>(a, ws, ks.kg, ks.kg_steps, s);
  if (ks.kg > 1) launch_splitk_epilogue(a, ws, ks.kg, s);
}

}  // namespace shai

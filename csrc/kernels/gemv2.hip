// Wide skinny GEMM for decode-shaped problems (M <= 64 activation rows), "skinny2":
//
//   C[m, n] = act(alpha * rstd[m] * sum_k X[m, k] * W[n, k] + bias[n]) (+ res_alpha * R[m, n]),  GLU optional
//
// Decode is weight-bandwidth bound; what limits the first skinny kernel (gemv.hip) at M = 64 is the LDS-DMA
// traffic per weight byte: its 64-row W tile streams together with a 64-row X tile (X : W bytes = M : BN
// = 1 : 1), so half of every CU's DMA issue and LDS writes carry activations that are the same for every
// workgroup, and its four waves split each K-step (cross-wave reduction at the end).  Here:
//
// * Workgroup = 4 waves, tile = 128 W rows (wave w owns rows [32 w, 32 w + 32)) x all M rows; every wave
//   consumes the WHOLE 64-wide K-step of its own rows -- 4 k16 slices x 2 X groups = 8 v_mfma_f32_32x32x16_bf16
//   per step, no cross-wave reduction: each wave's accumulators are its final (or split-K partial) outputs.
//   That body -- ring loop, counted vmcnt + one s_barrier per step, folded RMSNorm, epilogue, split-K fixup -- is
//   skinny_rows_kernel in skinny_common.h, shared with the MXFP4 kernel (gemv_fp4.hip); this file holds the bf16
//   format policy WBf16 (what a step's bytes are and how they become fragments), the instantiations and the launcher.
// * Per step: W tile 128 x 64 (16 KB) + X tile 64 x 64 (8 KB) by LDS-DMA (buffer_load ... lds, 16 B per
//   lane, range-checked zero fill for rows >= N / M and K tails), X : W = 1 : 2.  A ring of 3 x 24 KB, so two
//   workgroups fit a CU (four stages of W in flight per CU), or 6 x 24 KB for one.  The weight stream carries the nt
//   cache policy (read once per decode step).
// * Folded RMSNorm (GemmArgs::rms), split-K over kg workgroups per tile fixed up inside the launch (fp32 slabs
//   written through, an arrival ticket per tile from this launch's ticket slice, the last arriver sums the kg slabs in
//   K-group order and runs the fused epilogue): skinny_common.h.  There is no separate-fold form: without a ticket
//   slice the launch runs unsplit.  The epilogue stores element-wise (the MXFP4 kernel in quads).
#include "skinny_common.h"

namespace shai {

struct WBf16 {
  static constexpr int BK = 64, SLICES = 4;  // K per step, its k16 slices
  static constexpr bool FOLD = false, QUAD_STORES = false;
  static constexpr int W_ELEMS = SR_BN * BK;  // 8192 bf16 = 16 KB
  static constexpr int stage_bytes(int MB) { return (W_ELEMS + MB * BK) * 2; }  // W tile then X tile
  static constexpr int per(int MB) { return 4 + MB / 32; }                      // 4 W + 2 X DMA instructions

  // LDS images: rows of 8 16-B chunks, chunk ch of a row at position ch ^ (row >> 1) & 7 (source-side swizzle,
  // conflict-free ds_read_b128)
  static __device__ __forceinline__ int swz(int row, int ch) { return row * BK + ((ch ^ ((row >> 1) & 7)) << 3); }

  template <int MB>
  struct Lane {
    static_assert(MB == 64, "the bf16 wide kernel is built for two 32-row X groups only");
    static constexpr int XJ = MB / 32;  // X DMA instructions per wave
    __amdgpu_buffer_rsrc_t rW, rX;
    uint32_t woff[4], xoff[XJ];
    int wrow[4], xrow[XJ], lpos;

    // DMA geometry: a wave instruction fills 8 LDS rows x 128 B lane-linearly; the lane at chunk position lpos
    // fetches global chunk lpos ^ swz(row)
    __device__ __forceinline__ void init(const GemmArgs& p, int n0, int w, int lane, int) {
      rW = buf_rsrc(p.W, (long)p.N * p.ldw * 2);
      rX = buf_rsrc(p.A, (long)p.M * p.lda * 2);
      const int lrow = lane >> 3;
      lpos = lane & 7;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wrow[j] = (w * 4 + j) * 8 + lrow;  // W tile rows 32 w .. 32 w + 31
        const int n = n0 + wrow[j], ch = lpos ^ ((wrow[j] >> 1) & 7);
        woff[j] = n < p.N ? (uint32_t)(((long)n * p.ldw + ch * 8) * 2) : kDmaOob;
      }
#pragma unroll
      for (int j = 0; j < XJ; ++j) {
        xrow[j] = (w * XJ + j) * 8 + lrow;  // X rows 16 w .. 16 w + 15
        const int ch = lpos ^ ((xrow[j] >> 1) & 7);
        xoff[j] = xrow[j] < p.M ? (uint32_t)(((long)xrow[j] * p.lda + ch * 8) * 2) : kDmaOob;
      }
    }

    __device__ __forceinline__ void stage(const GemmArgs& p, uint8_t* st, int w, int kstep) const {
      bf16_t* sw = reinterpret_cast<bf16_t*>(st);
      bf16_t* sx = sw + W_ELEMS;
      const int k0 = kstep * BK;
      const bool kin = k0 < p.K;  // K tail: whole chunks past K read as zeros (K % 8 == 0)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ch = lpos ^ ((wrow[j] >> 1) & 7);
        const uint32_t off = (woff[j] != kDmaOob && kin && k0 + ch * 8 < p.K) ? woff[j] + (uint32_t)(k0 * 2) : kDmaOob;
        SHAI_DASSERT_DMA(off, (long)p.N * p.ldw * 2, kDmaOob);
        if (p.w_nt) __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (w * 4 + j) * 8 * BK), 16, off, 0, 0, 2);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (w * 4 + j) * 8 * BK), 16, off, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < XJ; ++j) {
        const int ch = lpos ^ ((xrow[j] >> 1) & 7);
        const uint32_t off = (xoff[j] != kDmaOob && kin && k0 + ch * 8 < p.K) ? xoff[j] + (uint32_t)(k0 * 2) : kDmaOob;
        SHAI_DASSERT_DMA(off, (long)p.M * p.lda * 2, kDmaOob);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (lds_void*)(sx + (w * XJ + j) * 8 * BK), 16, off, 0, 0, 0);
      }
    }

    // k16 slice s of the step: lane (fr, fh) takes chunk 2 s + fh of its W row against the same X chunk
    __device__ __forceinline__ bf16x8 w_frag(const uint8_t* st, int w, int fr, int fh, int s, int& xc) const {
      xc = 2 * s + fh;
      return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(st) + swz(32 * w + fr, xc));
    }
    static __device__ __forceinline__ bf16x8 x_frag(const uint8_t* st, int row, int ch) {
      return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(st) + W_ELEMS + swz(row, ch));
    }
  };
};

constexpr int S2_MB = 64;  // X rows (two 32-row groups)
// ring depth: 3 stages (72 KB, two workgroups per CU) or 6 stages (144 KB, one workgroup per CU with five
// steps of W in flight -- for grids of about one tile per CU, e.g. lm_head / gate_up without split-K)
constexpr size_t s2_lds(int stages) { return (size_t)stages * WBf16::stage_bytes(S2_MB); }

bool skinny2_supported(const GemmArgs& a) {
  if (a.res_rows != 0) return false;  // no broadcast residual
  // (QUICK_GELU is not instantiated by launch_skinny2: such problems stay on the other kernels)
  return a.M >= 1 && a.M <= S2_MB && !a.conv && a.batch <= 1 && a.w_slice_rows == 0 && !quantized_w(a) &&
         a.bias2d == nullptr &&
         a.act != ACT_QUICK_GELU &&
         a.gate == nullptr && a.row_mr == nullptr && a.K % 8 == 0 && a.lda % 8 == 0 && a.ldw % 8 == 0 && (!a.glu || a.N % 2 == 0) &&
         (long)a.N * a.ldw * 2 < 0x7fffffffL && (long)a.M * a.lda * 2 < 0x7fffffffL;
}

int skinny2_max_kgroups(const GemmArgs& a) { return max_kgroups((a.K + WBf16::BK - 1) / WBf16::BK); }

size_t skinny2_workspace_bytes(const GemmArgs& a, int kg) {
  if (kg <= 1) return 0;
  const size_t tiles = (a.N + SR_BN - 1) / SR_BN;
  return tiles * kg * (size_t)(SR_BN * S2_MB + S2_MB) * sizeof(float);  // [tile][kg] slabs
}

// kg > 1 needs ws (skinny2_workspace_bytes) and a ticket slice; without either it runs with kg = 1.
void launch_skinny2(const GemmArgs& a_in, float* ws, int kg, bool deep, hipStream_t s) {
  GemmArgs a = a_in;
  a.w_nt = skinny_nt();
  const int ksteps = (a.K + WBf16::BK - 1) / WBf16::BK;
  const int tiles = (a.N + SR_BN - 1) / SR_BN;
  KSplit ks = split_ksteps(ksteps, ws != nullptr ? kg : 1);
  unsigned* cnt = ks.kg > 1 ? skinny_ticket_slice(s, tiles) : nullptr;
  if (cnt == nullptr) ks = KSplit{1, ksteps};
  const dim3 grid(tiles, ks.kg), block(256);
  constexpr unsigned kActs = kActsAll & ~act_bit(ACT_QUICK_GELU);
  dispatch_epilogue<kActs>(a, [&](auto glu, auto act, auto rms) {
    if (deep) skinny_rows_kernel<WBf16, S2_MB, glu(), act(), rms(), 6><<<grid, block, s2_lds(6), s>>>(a, ws, ks.kg_steps, cnt);
    else skinny_rows_kernel<WBf16, S2_MB, glu(), act(), rms(), 3><<<grid, block, s2_lds(3), s>>>(a, ws, ks.kg_steps, cnt);
  });
}

}  // namespace shai

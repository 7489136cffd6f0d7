// Skinny GEMM over NF4 weights (the bitsandbytes 4-bit format) for decode-shaped problems (M <= 64 activation rows):
//
//   C[m, n] = act(alpha * rstd[m] * sum_k X[m, k] * What[n, k] + bias[n]) (+ res_alpha * R[m, n]),  GLU optional
//
// What = bf16_rne(fp32(NF4_TABLE[code]) * fp32(absmax)): 4-bit codes into the 16-quantile normal-float table, two per
// byte (even k in the low nibble), W [N, K / 2] bytes row-major, and one fp32 absmax per (row, 64 consecutive k),
// stored tiled per K step: A [ceil(K / 128), N, 2] fp32, entry (s, n, b) = the absmax of row n's block 2 s + b (a
// block past K / 64 holds 0).  ops.quantize_nf4 produces this layout, ops.dequant_nf4 (dequant_nf4_kernel below)
// inverts it.  4.5 bits per weight.
//
// The body is skinny_rows_kernel (skinny_common.h), shared with the bf16 and MXFP4 kernels: 128 W rows per workgroup,
// wave w consumes the whole K step of its 32 rows, counted vmcnt + one s_barrier per step, every epilogue and both
// split-K forms.  This file holds the NF4 format policy WNf4, the instantiations, the launcher and the dequantise
// kernel.  Nothing in the shared body changes: the lookup table lives in a register of the policy's Lane.
//
// The widening.  gfx950 has no convert for NF4, and the contract above needs the fp32 table value (24-bit
// mantissas) times the fp32 absmax, rounded once to bf16: per code one lookup, one v_mul_f32, half a
// v_cvt_pk_bf16_f32.  Candidates for the lookup, per 128-row x 128-k step = 64 codes per lane (8 dwords):
//
//   * byte-plane v_perm_b32: a 16-entry table of one byte plane is 4 dwords = 2 v_perm_b32 (8 entries each) + a
//     v_bfi on code bit 3 for 4 codes; 4 planes and 4 more perms to interleave the planes back into fp32, plus the
//     selector preparation: ~5 VALU per code, ~320 + 96 (mul, cvt) = ~416 VALU per lane and step.  At 4 cycles per
//     wave64 VALU instruction that is ~1660 cycles per wave and step, with two waves per SIMD: more than the ~1300
//     cycles in which HBM delivers a step's 8.5 KB of weight bytes to a CU (3.5-4 TB/s over 256 CUs at 2.4 GHz =
//     ~6.5 B per cycle and CU).  VALU bound: rejected.
//   * a 16-dword fp32 table in LDS read with ds_read_b32: conflict free (equal codes broadcast, different codes hit
//     different banks), but a byte address wants (dword >> (4 i - 2)) & 0x3c = 2 VALU per code, 64 B of LDS that the
//     ring's single LDS object would have to carry and a per-workgroup preamble hook in the shared body.
//   * ds_bpermute_b32 from lanes holding the table -- chosen.  It takes the same slot of the LDS pipe as a
//     ds_read_b32 (a wave64 dword gather) without touching the banks, and it uses only bits [7:2] of its address (the
//     source lane, mod 64): with lane l holding TABLE[l & 15], the address dword >> (4 i - 2) (dword << 2 for i = 0)
//     selects lane (code_i + 16 * the low two bits of code_{i+1}), i.e. TABLE[code_i], WITHOUT masking: 1 VALU per
//     code.  No LDS bytes, no preamble: the table is one VGPR built from literals in Lane::init.
//
//   Per lane and step with the choice: 64 v_lshrrev + 64 v_mul_f32 + 32 v_cvt_pk = 160 VALU (~640 cycles per wave,
//   two waves per SIMD: about half of the step's HBM time) and, on the LDS pipe per wave, 64 ds_bpermute_b32 + 2
//   ds_read_b128 of codes + 1 ds_read_b32 of absmax + 8 (M <= 32) / 16 ds_read_b128 of X.  Per workgroup and step
//   at 128 B per cycle: gathers 4 x 64 x 2 = 512 cycles, X reads 256 / 512, code reads 64, DMA writes of the 17 /
//   25 KB stage 136 / 200: ~970 (M <= 32) / ~1290 (M <= 64) cycles against the ~1300 of HBM.  The MFMAs (8 / 16 per
//   wave and step) are free and the CU's memory issue is the limit (profiles/decode_gemm_lab_round6.md), so the
//   expectation was: beside MXFP4 at M <= 32, LDS-pipe bound and behind it at M = 64.
//
//   NOT VALIDATED: the first measurements (profiles/nf4_decode.md) contradict this count by a factor of three per
//   step; the 2-cycle gather rate is the suspected error.  The geometry below was derived from the count as it
//   stands and inherits that doubt: it is a starting point, to be re-derived once the gather's real rate is known.
//
// Geometry, from that count:
//
// * K step = 128 = two NF4 blocks.  Lane (fr, fh) of the MFMA layout owns K half fh of row fr, so ONE absmax serves
//   all 64 codes of a lane and step (one ds_read_b32, one scalar operand of the 64 multiplies).  The absmax DMA of a
//   wave is one 4-B instruction with all 64 lanes live: lane l = (row 32 w + (l >> 1), block l & 1), 256 B.  (A
//   256-wide step would carry 16 B of absmax per row, the other granule that fits, but its 34 KB stage at M <= 32
//   leaves one workgroup per CU or a two-deep ring.)
// * The lookup is latency (a DS round trip per gather) hidden by independent work: the 64 gathers of a step are
//   independent of each other, and a second workgroup on the CU lets one wave per SIMD widen while the other waits
//   at its barrier.  So two workgroups per CU, each with the deepest ring that fits 80 KB: stage = 8 KB codes + 1 KB
//   absmax + 8 / 16 KB X = 17 / 25 KB, 4 stages (M <= 32, 68 KB) / 3 stages (M <= 64, 75 KB).  Three workgroups of
//   3 x 17 KB would fit at M <= 32, but the K-group heuristic below launches about one workgroup per CU (two at
//   most), where the third slot stays empty and the ring depth is what keeps bytes in flight.  The stage holds the
//   same bytes as MXFP4's (its absmax kilobyte is all payload where MXFP4's scale kilobyte is half zero fill), so the
//   arithmetic ends at the ring depths of gemv_fp4.hip (an outcome of equal stage bytes under an 80 KB budget, not
//   a measured optimum for a kernel whose limiter is the lookup).
// * Everything arrives by LDS-DMA (buffer_load ... lds, range check = zero fill for rows >= N / M and K tails in
//   whole 32-code chunks; K % 64 == 0): codes in 2 instructions of 16 rows x 64 B (16-B chunk c at position
//   c ^ (row >> 2) & 3, nt hint), X as in gemv_fp4.hip (4 rows x 256 B per instruction, chunk c at c ^ row & 15).
// * Lane (fr, fh) reads the two 16-B code chunks 2 fh, 2 fh + 1 of row fr (together block fh of the step), widens
//   dword j of chunk c (k = 32 c + 8 j .. + 7) and multiplies it against X chunk 4 c + j: K is consumed in a permuted
//   order inside the step, fp32 accumulation in v_mfma_f32_32x32x16_bf16.
// * A zero-filled code (rows >= N, K tail) widens to TABLE[0] * absmax = -absmax: its absmax is zero filled (rows)
//   or a stored 0 (the block past K), and its X chunk is zero filled too.
#include "skinny_common.h"

namespace shai {

// (the table, nf4_table_entry and nf4x8_widen: skinny_common.h, shared with gemm_nf4.hip)
struct WNf4 {
  static constexpr int BK = 128, SLICES = 8;  // K per step (2 blocks of 64), its k16 slices
  static constexpr int K_MULT = 64, S_ROW = 8;  // K % 64 == 0 (a block); absmax bytes per W row and step
  static constexpr bool FOLD = true, QUAD_STORES = true;
  static constexpr int W_BYTES = SR_BN * BK / 2;  // 8 KB of codes
  static constexpr int A_BYTES = 4 * 256;         // one 64-lane x 4-B DMA per wave: 32 rows x 2 blocks of fp32
  static constexpr int stage_bytes(int MB) { return W_BYTES + A_BYTES + MB * BK * 2; }  // codes, absmax, X
  static constexpr int per(int MB) { return 2 + 1 + 2 * (MB / 32); }                    // DMA instructions per wave

  template <int MB>
  struct Lane {
    static constexpr int XJ = 2 * (MB / 32);  // X DMA instructions per wave
    __amdgpu_buffer_rsrc_t rW, rA, rX;
    uint32_t woff[2], wk[2], aoff, xoff[XJ], xk[XJ];
    float tab;  // TABLE[lane & 15]

    // DMA geometry (LDS images are lane-linear per wave instruction; the swizzle is on the source address)
    __device__ __forceinline__ void init(const GemmArgs& p, int n0, int w, int lane, int ksteps) {
      tab = nf4_table_entry(lane);
      rW = buf_rsrc(p.W, (long)p.N * p.ldw);  // ldw: bytes
      rA = buf_rsrc(p.w_nf4_absmax, (long)ksteps * p.N * 8);
      rX = buf_rsrc(p.A, (long)p.M * p.lda * 2);
      // codes: instruction j of wave w fills tile rows 32 w + 16 j + (lane >> 2), chunk position lane & 3
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = 32 * w + 16 * j + (lane >> 2), n = n0 + row;
        const int c = (lane & 3) ^ ((row >> 2) & 3);
        wk[j] = (uint32_t)(c * 32);  // first k of the chunk inside the step
        woff[j] = n < p.N ? (uint32_t)((long)n * p.ldw + c * 16) : kDmaOob;
      }
      // absmax: lane l fetches block l & 1 of tile row 32 w + (l >> 1)
      {
        const int n = n0 + 32 * w + (lane >> 1);
        aoff = n < p.N ? (uint32_t)(n * 8 + (lane & 1) * 4) : kDmaOob;
      }
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
      uint8_t* sa = sw + W_BYTES;
      uint8_t* sx = sa + A_BYTES;
      const uint32_t k0 = (uint32_t)kstep * BK;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // K tail: whole 32-code chunks past K read as zeros (K % 64 == 0)
        const uint32_t off = (woff[j] != kDmaOob && k0 + wk[j] < (uint32_t)p.K) ? woff[j] + (k0 >> 1) : kDmaOob;
        SHAI_DASSERT_DMA(off, (long)p.N * p.ldw, kDmaOob);
        // weights are read once per decode step by one CU: nt (aux 2), as in gemv.hip
        if (p.w_nt) __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (32 * w + 16 * j) * 64), 16, off, 0, 0, 2);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (32 * w + 16 * j) * 64), 16, off, 0, 0, 0);
      }
      {
        const uint32_t off = aoff != kDmaOob ? aoff + (uint32_t)kstep * (uint32_t)p.N * 8u : kDmaOob;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_void*)(sa + w * 256), 4, off, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < XJ; ++j) {
        const uint32_t off = (xoff[j] != kDmaOob && k0 + xk[j] < (uint32_t)p.K) ? xoff[j] + k0 * 2 : kDmaOob;
        SHAI_DASSERT_DMA(off, (long)p.M * p.lda * 2, kDmaOob);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (lds_void*)(sx + (XJ * w + j) * 1024), 16, off, 0, 0, 0);
      }
    }

    // k16 slice s = 4 i + j: dword j of code chunk c = 2 fh + i (k = 32 c + 8 j .. + 7, block fh of the step),
    // widened, against X chunk 4 c + j.  (The absmax and the 16-B chunk are read per slice in the source; the
    // unrolled body reads each once.)
    __device__ __forceinline__ bf16x8 w_frag(const uint8_t* st, int w, int fr, int fh, int s, int& xc) const {
      const uint8_t* sw = st;
      const uint8_t* sa = sw + W_BYTES;
      const int wrow = 32 * w + fr, wswz = (wrow >> 2) & 3;
      const float am = *reinterpret_cast<const float*>(sa + w * 256 + fr * 8 + fh * 4);
      const int c = 2 * fh + (s >> 2), j = s & 3;
      SHAI_DASSERT(wrow * 64 + ((c ^ wswz) << 4) + 16 <= W_BYTES);
      const uint4_ cw = *reinterpret_cast<const uint4_*>(sw + wrow * 64 + ((c ^ wswz) << 4));
      xc = 4 * c + j;
      return nf4x8_widen(cw[j], am, tab);
    }
    static __device__ __forceinline__ bf16x8 x_frag(const uint8_t* st, int row, int xc) {
      return *reinterpret_cast<const bf16x8*>(st + W_BYTES + A_BYTES + row * 256 + ((xc ^ (row & 15)) << 4));
    }
  };
};

// NF4 codes + tiled absmax -> bf16 [N, K] (problems above 64 rows, gated / LayerNorm-folded / batched calls run the
// bf16 GEMMs on it): one thread per half block (16 B of codes -> 64 B of bf16), the table in LDS (equal codes
// broadcast, different codes hit different banks)
__global__ void __launch_bounds__(256) dequant_nf4_kernel(const uint8_t* __restrict__ wq,
                                                          const float* __restrict__ absmax,
                                                          bf16_t* __restrict__ out, long halves, int KH, long N) {
  __shared__ float tab[16];
  if (threadIdx.x < 16) tab[threadIdx.x] = nf4_table_entry(threadIdx.x);
  __syncthreads();
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < halves; i += (long)gridDim.x * blockDim.x) {
    const long n = i / KH;
    const int blk = (int)(i - n * KH) >> 1;  // KH = K / 32 half blocks per row
    const float am = absmax[((long)(blk >> 1) * N + n) * 2 + (blk & 1)];
    const uint4_ cw = reinterpret_cast<const uint4_*>(wq)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x8 wf;
#pragma unroll
      for (int e = 0; e < 8; ++e) wf[e] = (__bf16)(tab[(cw[j] >> (4 * e)) & 15u] * am);
      reinterpret_cast<uint4_*>(out)[i * 4 + j] = __builtin_bit_cast(uint4_, wf);
    }
  }
}

void launch_dequant_nf4(const uint8_t* wq, const float* absmax, bf16_t* out, long N, int K, hipStream_t s) {
  const long halves = N * (long)(K / 32);
  if (halves == 0) return;
  long blocks = (halves + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  dequant_nf4_kernel<<<(int)blocks, 256, 0, s>>>(wq, absmax, out, halves, K / 32, N);
}

// ---------------------------------------------------------------------------- host side
// a.W: codes [N, K / 2] bytes at a row stride of a.ldw BYTES; a.w_nf4_absmax: [ceil(K / 128), N, 2] fp32
// (K groups, workspace, launch and the ring depth of the header: the q4_skinny_* templates of skinny_common.h, shared
// with gemv_fp4.hip)
static bool skinny_nf4_supported(const GemmArgs& a) {
  return a.w_nf4_absmax != nullptr && a.w_mx_scale == nullptr && q4_skinny_supported<WNf4>(a);
}

const Q4SkinnyOps& nf4_skinny_ops() {
  static const Q4SkinnyOps ops = q4_skinny_ops<WNf4>(skinny_nf4_supported);
  return ops;
}

}  // namespace shai

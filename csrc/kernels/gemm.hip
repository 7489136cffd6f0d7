// bf16 MFMA GEMM / implicit-GEMM convolution for gfx950 with fused epilogues.
//
//   C[b,m,n] = act(alpha * sum_k A[b,m,k] * W[b,n,k] + bias[n] + bias2d[m/R, n]) + res_alpha * R[b,m,n]
//
// A is either a row-major activation [M, K] or (conv=1) an NHWC image that is
// gathered on the fly (implicit im2col, K = KH*KW*Cin ordered (kh, kw, c)).
// The gather can (a) apply a GroupNorm scale/shift + SiLU per (image, channel)
// ("normalise on load", so GroupNorm+SiLU never round-trips HBM), (b) read a
// nearest-2x upsampled view of the input (Upsample2D fused) and (c) read the
// channel range [Cin1, Cin) from a second tensor (skip-connection concat fused).
//
// Tile 128x128x64, 256 threads = 4 waves (2x2), each wave 64x64 built from
// v_mfma_f32_32x32x16_bf16.  The MFMA is issued as W*X^T (swapped operands) so
// each lane ends up owning one output ROW and 4 groups of 4 consecutive
// columns: epilogue loads/stores are 8-byte vectors along N.
// Staging: global -> registers (issued one K-tile ahead, written to LDS after
// the compute of the current tile, T14 split) -> XOR-swizzled LDS (conflict
// free ds_read_b128, see SWZ below), double-buffered, one barrier per K-tile.
// Blocks are remapped XCD-aware (bijective) and grouped along M for L2 reuse.
//
// Replaces the GEMM/conv work the reference delegates to cuBLAS/cuDNN/Inductor
// (app/run-sd.py:104-135) and NEFFs (app/compile-sd2.py:16-20).
#include "common.h"
#include "launchers.h"

namespace shai {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_ELEMS = BM * BK;  // per operand per stage

// LDS chunk (16 B) position for (row, chunk) in a [128][64] bf16 tile.
// ds_read_b128 lane groups read 16 distinct rows at one chunk; XOR with
// (row>>1)&7 spreads them over all 16 slots of the 256-B bank row.
__device__ __forceinline__ int swz(int row, int ch) { return row * BK + ((ch ^ ((row >> 1) & 7)) << 3); }

struct ConvRow {
  int n, oh, ow;
  bool valid;
};

template <bool CONV, bool CONV_FAST, bool NORM_IN, bool GLU, int ACT>
__global__ void __launch_bounds__(256, 2) gemm_kernel(const GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  bf16_t* sA = smem;                      // [2][128*64]
  bf16_t* sW = smem + 2 * TILE_ELEMS;     // [2][128*64]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;

  // ---- tile mapping: XCD-aware bijective remap + grouped ordering
  const int tiles_m = (p.M + BM - 1) / BM;
  const int tiles_n = (p.N + BN - 1) / BN;
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
  const int tm = first_m + in_group % gsize;
  const int tn = in_group / gsize;
  const int m0 = tm * BM, n0 = tn * BN;
  const int b = blockIdx.y;

  const bf16_t* A = p.A + (long)b * p.batch_a;
  const bf16_t* Wt = p.W + (long)b * p.batch_w;

  // ---- per-thread staging assignment: rows (tid>>3) + 32*i, chunk tid&7
  const int srow = tid >> 3;
  const int sch = tid & 7;
  ConvRow cr[4];
  if constexpr (CONV) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + srow + 32 * i;
      cr[i].valid = m < p.M;
      const int mm = cr[i].valid ? m : 0;
      const int hw = p.OH * p.OW;
      cr[i].n = mm / hw;
      const int rem = mm - cr[i].n * hw;
      cr[i].oh = rem / p.OW;
      cr[i].ow = rem - cr[i].oh * p.OW;
    }
  }

  uint4_ ra[4], rw[4];
  const uint4_ zero4 = {0u, 0u, 0u, 0u};

  auto load_tile = [&](int k0) {
    // ---- W operand: rows n0 + srow + 32 i, k = k0 + 8*sch
    const int kw_ = k0 + sch * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + srow + 32 * i;
      rw[i] = (n < p.N && kw_ < p.K) ? *reinterpret_cast<const uint4_*>(Wt + (long)n * p.ldw + kw_) : zero4;
    }
    // ---- A operand
    if constexpr (!CONV) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + srow + 32 * i;
        ra[i] = (m < p.M && kw_ < p.K) ? *reinterpret_cast<const uint4_*>(A + (long)m * p.lda + kw_) : zero4;
      }
    } else {
      int tap, c;
      if constexpr (CONV_FAST) {  // whole K tile inside one filter tap (Cin % 64 == 0)
        tap = k0 / p.Cin;
        c = k0 - tap * p.Cin + sch * 8;
      } else {
        tap = kw_ / p.Cin;
        c = kw_ - tap * p.Cin;
      }
      const int kh = tap / p.KW, kwi = tap - (tap / p.KW) * p.KW;
      const bool kok = kw_ < p.K;
      const bool second = p.A2 != nullptr && c >= p.Cin1;
      const int csrc = second ? c - p.Cin1 : c;
      const int cstride = p.A2 != nullptr ? (second ? p.Cin - p.Cin1 : p.Cin1) : p.Cin;
      const bf16_t* src = second ? p.A2 : A;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int ih, iw;
        bool ok = cr[i].valid && kok;
        if (p.upsample) {
          const int uh = cr[i].oh - p.pad + kh, uw = cr[i].ow - p.pad + kwi;
          ok = ok && uh >= 0 && uh < 2 * p.H && uw >= 0 && uw < 2 * p.Wd;
          ih = uh >> 1;
          iw = uw >> 1;
        } else {
          ih = cr[i].oh * p.stride - p.pad + kh;
          iw = cr[i].ow * p.stride - p.pad + kwi;
          ok = ok && ih >= 0 && ih < p.H && iw >= 0 && iw < p.Wd;
        }
        if (ok) {
          const long pix = ((long)cr[i].n * p.H + ih) * p.Wd + iw;
          uint4_ v = *reinterpret_cast<const uint4_*>(src + pix * cstride + csrc);
          if constexpr (NORM_IN) {
            const float* sc = p.in_scale + (long)cr[i].n * p.Cin + c;
            const float* sh = p.in_shift + (long)cr[i].n * p.Cin + c;
            const float4_ a0 = *reinterpret_cast<const float4_*>(sc), a1 = *reinterpret_cast<const float4_*>(sc + 4);
            const float4_ b0 = *reinterpret_cast<const float4_*>(sh), b1 = *reinterpret_cast<const float4_*>(sh + 4);
            float f[8];
            unpack8(v, f);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              f[e] = apply_act_rt(p.in_act, f[e] * a0[e] + b0[e]);
              f[e + 4] = apply_act_rt(p.in_act, f[e + 4] * a1[e] + b1[e]);
            }
            v = pack8(f);
          }
          ra[i] = v;
        } else {
          ra[i] = zero4;
        }
      }
    }
  };

  auto store_tile = [&](int stage) {
    bf16_t* a = sA + stage * TILE_ELEMS;
    bf16_t* w = sW + stage * TILE_ELEMS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = srow + 32 * i;
      *reinterpret_cast<uint4_*>(a + swz(row, sch)) = ra[i];
      *reinterpret_cast<uint4_*>(w + swz(row, sch)) = rw[i];
    }
  };

  float16_ acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = (p.K + BK - 1) / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();

  const int fr = lane & 31, fh = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile((kt + 1) * BK);
    const bf16_t* a = sA + cur * TILE_ELEMS;
    const bf16_t* w = sW + cur * TILE_ELEMS;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 af[2], wf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(a + swz(wm * 64 + i * 32 + fr, 2 * s + fh));
#pragma unroll
      for (int j = 0; j < 2; ++j)
        wf[j] = *reinterpret_cast<const bf16x8*>(w + swz(wn * 64 + j * 32 + fr, 2 * s + fh));
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: lane owns row m; per 32x32 block 4 groups of 4 consecutive n
  bf16_t* C = p.C + (long)b * p.batch_c;
  const bf16_t* R = p.residual ? p.residual + (long)b * p.batch_r : nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wm * 64 + i * 32 + fr;
    if (m >= p.M) continue;
    const bf16_t* b2 = p.bias2d ? p.bias2d + (long)(m / p.rows_per_bias2d) * bias2d_stride(p) : nullptr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 64 + j * 32 + 8 * g + 4 * fh;
        if (n >= p.N) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e] * p.alpha;
        const bool full = n + 3 < p.N && (p.ldc & 3) == 0 && (p.ldr & 3) == 0;
        if (p.bias) {
          if (full) {
            const uint2_ bb = *reinterpret_cast<const uint2_*>(p.bias + n);
            v[0] += bf2f(bb[0] & 0xffff); v[1] += bf2f(bb[0] >> 16);
            v[2] += bf2f(bb[1] & 0xffff); v[3] += bf2f(bb[1] >> 16);
          } else {
            for (int e = 0; e < 4 && n + e < p.N; ++e) v[e] += bf2f(p.bias[n + e]);
          }
        }
        if (b2) {
          if (full) {
            const uint2_ bb = *reinterpret_cast<const uint2_*>(b2 + n);
            v[0] += bf2f(bb[0] & 0xffff); v[1] += bf2f(bb[0] >> 16);
            v[2] += bf2f(bb[1] & 0xffff); v[3] += bf2f(bb[1] >> 16);
          } else {
            for (int e = 0; e < 4 && n + e < p.N; ++e) v[e] += bf2f(b2[n + e]);
          }
        }
        if constexpr (GLU) {
          // interleaved (value, gate) pairs -> 2 outputs at column n/2
          const float o0 = v[0] * apply_act<ACT>(v[1]);
          const float o1 = v[2] * apply_act<ACT>(v[3]);
          const int nc = n >> 1;
          float r0 = 0.f, r1 = 0.f;
          if (R) {
            r0 = bf2f(R[(long)m * p.ldr + nc]) * p.res_alpha;
            r1 = bf2f(R[(long)m * p.ldr + nc + 1]) * p.res_alpha;
          }
          if (((p.ldc | nc) & 1) == 0) {
            *reinterpret_cast<uint32_t*>(C + (long)m * p.ldc + nc) = pack2(o0 + r0, o1 + r1);
          } else {
            C[(long)m * p.ldc + nc] = f2bf(o0 + r0);
            C[(long)m * p.ldc + nc + 1] = f2bf(o1 + r1);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = apply_act<ACT>(v[e]);
          if (full) {
            if (R) {
              const uint2_ rr = *reinterpret_cast<const uint2_*>(R + (long)m * p.ldr + n);
              v[0] += bf2f(rr[0] & 0xffff) * p.res_alpha; v[1] += bf2f(rr[0] >> 16) * p.res_alpha;
              v[2] += bf2f(rr[1] & 0xffff) * p.res_alpha; v[3] += bf2f(rr[1] >> 16) * p.res_alpha;
            }
            uint2_ o;
            o[0] = pack2(v[0], v[1]);
            o[1] = pack2(v[2], v[3]);
            *reinterpret_cast<uint2_*>(C + (long)m * p.ldc + n) = o;
          } else {
            for (int e = 0; e < 4 && n + e < p.N; ++e) {
              float x = v[e];
              if (R) x += bf2f(R[(long)m * p.ldr + n + e]) * p.res_alpha;
              C[(long)m * p.ldc + n + e] = f2bf(x);
            }
          }
        }
      }
    }
  }
}

template <bool CONV, bool FAST, bool NORM, bool GLU>
static void dispatch_act(const GemmArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  switch (a.act) {
    case ACT_SILU: gemm_kernel<CONV, FAST, NORM, GLU, ACT_SILU><<<grid, 256, lds, s>>>(a); break;
    case ACT_GELU: gemm_kernel<CONV, FAST, NORM, GLU, ACT_GELU><<<grid, 256, lds, s>>>(a); break;
    case ACT_GELU_TANH: gemm_kernel<CONV, FAST, NORM, GLU, ACT_GELU_TANH><<<grid, 256, lds, s>>>(a); break;
    case ACT_QUICK_GELU: gemm_kernel<CONV, FAST, NORM, GLU, ACT_QUICK_GELU><<<grid, 256, lds, s>>>(a); break;
    case ACT_RELU: gemm_kernel<CONV, FAST, NORM, GLU, ACT_RELU><<<grid, 256, lds, s>>>(a); break;
    default: gemm_kernel<CONV, FAST, NORM, GLU, ACT_NONE><<<grid, 256, lds, s>>>(a); break;
  }
}

void launch_gemm(const GemmArgs& a, hipStream_t s) {
  const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
  dim3 grid(tiles, a.batch > 0 ? a.batch : 1);
  const size_t lds = (size_t)4 * TILE_ELEMS * sizeof(bf16_t);  // 64 KiB
  if (!a.conv) {
    if (a.glu) dispatch_act<false, false, false, true>(a, grid, lds, s);
    else dispatch_act<false, false, false, false>(a, grid, lds, s);
    return;
  }
  const bool fast = (a.Cin % 64) == 0 && (a.A2 == nullptr || (a.Cin1 % 64) == 0);
  const bool norm = a.in_scale != nullptr;
  // conv kernels: no GLU; activations limited to none / silu to bound instantiations
  if (fast) {
    if (norm) {
      if (a.act == ACT_SILU) gemm_kernel<true, true, true, false, ACT_SILU><<<grid, 256, lds, s>>>(a);
      else gemm_kernel<true, true, true, false, ACT_NONE><<<grid, 256, lds, s>>>(a);
    } else {
      if (a.act == ACT_SILU) gemm_kernel<true, true, false, false, ACT_SILU><<<grid, 256, lds, s>>>(a);
      else gemm_kernel<true, true, false, false, ACT_NONE><<<grid, 256, lds, s>>>(a);
    }
  } else {
    if (norm) gemm_kernel<true, false, true, false, ACT_NONE><<<grid, 256, lds, s>>>(a);
    else gemm_kernel<true, false, false, false, ACT_NONE><<<grid, 256, lds, s>>>(a);
  }
}

}  // namespace shai

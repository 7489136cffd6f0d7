// Sparse mixture-of-experts MLP (Mixtral): router, grouping of rows by expert, the two grouped expert GEMMs, combine.
//
//   y[m] = bf16(residual[m] + sum_j bf16(w[m, j] * W2[e_j] @ h[m, j])),   h[m, j] = bf16(v * silu(g)),
//   (v, g)[i] = rstd[m] * <x[m], W13[e_j][2 i], W13[e_j][2 i + 1]>,        (e_j, w[m, j]) = top-k of the router
//
// Every grid is sized on the host from M, E and k alone; what depends on the routing (how many row tiles exist, which
// expert a tile belongs to, which rows it holds) is read on the device from the plan that moe_align wrote, and a
// workgroup past the tile count exits.  So the five launches can be recorded into a graph, nothing is read back, and
// there is no floating-point atomic: the outputs are a pure function of the inputs.
//
// * moe_route_kernel: one wave streams R = 4 rows of x once; each lane keeps the rows' sums of squares and their E
//   dot products against the fp32 router weight (L2-resident: 128 KB at Mixtral size, loaded once for the 4 rows),
//   then the wave reduces and picks the top k (a tie goes to the lower expert index).
// * moe_align_kernel: one workgroup; a stable counting sort of the S = M k slots (slot = m k + j) by expert from wave
//   ballots: per-wave per-expert counts, a prefix over (expert, wave), then each slot's rank among the earlier slots
//   of its expert.  Experts are padded to the row-tile height TM (padding = -1), so tile t starts at position t TM
//   and only its expert has to be recorded; empty experts get no tile.
// * moe_gemm_kernel<TM, GLU, SPLIT>: one workgroup (4 waves) per (row tile, 128 weight rows, K slab).  Wave w owns
//   weight rows [32 w, 32 w + 32) against all TM rows with v_mfma_f32_32x32x16_bf16 (weights as A, activations as B),
//   fp32 accumulation, no cross-wave reduction.  A K step is 64 wide: the expert's 128 x 64 weight tile and the
//   TM x 64 activation tile arrive by LDS-DMA into a ring of 3 stages (swizzled at the source, conflict-free
//   ds_read_b128); the activation rows of the w13 GEMM are gathered by the DMA's per-lane offset (row = slot / k) and
//   a padding row takes the out-of-range sentinel (zero fill).  GLU epilogue: value and gate times the row's rstd,
//   value * silu(gate), bf16, stored at the sorted position; down epilogue: times the slot's routing weight, bf16
//   (SPLIT: the raw fp32 slab of this K range).
// * moe_combine_kernel: y[m] = bf16(residual[m] + sum_j slot output at pos[m, j]), j ascending; with split K it first
//   sums the slabs in slab order, applies the routing weight and rounds to bf16.
#include "skinny_common.h"

namespace shai {

constexpr int MOE_BN = 128, MOE_BK = 64, MOE_STAGES = 3, MOE_EMAX = 16;

// the plan: [0] tile count, [4 ..) expert of each tile, then the sorted slot list, then pos[slot]
struct MoePlan {
  int t_max, s_cap;
  __host__ __device__ int tiles_off() const { return 4; }
  __host__ __device__ int sorted_off() const { return 4 + ((t_max + 3) & ~3); }
  __host__ __device__ int pos_off() const { return sorted_off() + s_cap; }
};

// ---------------------------------------------------------------------------- router
template <int EP>
__global__ void __launch_bounds__(256) moe_route_kernel(const bf16_t* __restrict__ x, long ldx,
                                                        const float* __restrict__ wg, int* __restrict__ ids,
                                                        float* __restrict__ wts, float* __restrict__ rstd, int M,
                                                        int H, int E, int k, float eps, int rms) {
  constexpr int R = 4;
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
  if (row0 >= M) return;
  float acc[R][EP], ss[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ss[r] = 0.f;
#pragma unroll
    for (int e = 0; e < EP; ++e) acc[r][e] = 0.f;
  }
  for (int c = lane * 8; c < H; c += 512) {
    float xv[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      uint4_ v = {0u, 0u, 0u, 0u};
      if (row0 + r < M) v = *reinterpret_cast<const uint4_*>(x + (long)(row0 + r) * ldx + c);
      unpack8(v, xv[r]);
#pragma unroll
      for (int i = 0; i < 8; ++i) ss[r] = fmaf(xv[r][i], xv[r][i], ss[r]);
    }
#pragma unroll
    for (int e = 0; e < EP; ++e) {
      if (e < E) {
        const float4_ w0 = *reinterpret_cast<const float4_*>(wg + (long)e * H + c);
        const float4_ w1 = *reinterpret_cast<const float4_*>(wg + (long)e * H + c + 4);
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[r][e] = fmaf(xv[r][i], w0[i], acc[r][e]);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[r][e] = fmaf(xv[r][4 + i], w1[i], acc[r][e]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (row0 + r >= M) break;
    const float rs = rms ? rsqrtf(wave_sum(ss[r]) / (float)H + eps) : 1.f;
    // every lane holds every logit after the butterfly: the picks below are wave-uniform, lane 0 stores
    float l0 = 0.f, l1 = 0.f;
    int i0 = 0, i1 = -1;
#pragma unroll
    for (int e = 0; e < EP; ++e) {
      if (e < E) {
        acc[r][e] = wave_sum(acc[r][e]) * rs;
        if (e == 0 || acc[r][e] > l0) {
          l0 = acc[r][e];
          i0 = e;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < EP; ++e) {
      if (e < E && e != i0 && (i1 < 0 || acc[r][e] > l1)) {
        l1 = acc[r][e];
        i1 = e;
      }
    }
    if (lane == 0) {
      const int m = row0 + r;
      rstd[m] = rs;
      if (k == 1) {
        ids[m] = i0;
        wts[m] = 1.f;
      } else {
        const float d = expf(l1 - l0);
        const float inv = 1.f / (1.f + d);
        ids[2 * m] = i0;
        ids[2 * m + 1] = i1;
        wts[2 * m] = inv;
        wts[2 * m + 1] = d * inv;
      }
    }
  }
}

// ---------------------------------------------------------------------------- grouping
template <int TM>
__global__ void __launch_bounds__(256) moe_align_kernel(const int* __restrict__ ids, int* __restrict__ plan, int S,
                                                        int E, MoePlan pl) {
  __shared__ int wc[4][MOE_EMAX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int* tile_expert = plan + pl.tiles_off();
  int* sorted = plan + pl.sorted_off();
  int* pos = plan + pl.pos_off();
  // wave w owns the slots [s0, s1), ascending: the waves' ranges in wave order are the slot order
  const int per_wave = (S + 255) / 256 * 64;
  const int s0 = min(S, w * per_wave), s1 = min(S, s0 + per_wave);
  const uint64_t below = (1ull << lane) - 1ull;
  int cnt[MOE_EMAX];
#pragma unroll
  for (int e = 0; e < MOE_EMAX; ++e) cnt[e] = 0;
  for (int b = s0; b < s1; b += 64) {
    const int id = b + lane < s1 ? ids[b + lane] : -1;
#pragma unroll
    for (int e = 0; e < MOE_EMAX; ++e)
      if (e < E) cnt[e] += __popcll(__ballot(id == e));
  }
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < MOE_EMAX; ++e) wc[w][e] = cnt[e];
  }
  __syncthreads();
  // cnt[e] becomes the position of this wave's first slot of expert e
  int ps = 0;
#pragma unroll
  for (int e = 0; e < MOE_EMAX; ++e) {
    if (e < E) {
      int tot = 0, before = 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int c = wc[v][e];
        tot += c;
        before += v < w ? c : 0;
      }
      cnt[e] = ps + before;
      const int padded = (tot + TM - 1) / TM * TM;
      for (int i = tot + tid; i < padded; i += 256) sorted[ps + i] = -1;
      for (int i = tid; i < padded / TM; i += 256) tile_expert[ps / TM + i] = e;
      ps += padded;
    }
  }
  if (tid == 0) plan[0] = ps / TM;
  for (int b = s0; b < s1; b += 64) {
    const int s = b + lane;
    const int id = s < s1 ? ids[s] : -1;
    int at = -1;
#pragma unroll
    for (int e = 0; e < MOE_EMAX; ++e) {
      if (e < E) {
        const uint64_t mask = __ballot(id == e);
        if (id == e) at = cnt[e] + __popcll(mask & below);
        cnt[e] += __popcll(mask);
      }
    }
    if (s < s1) {
      pos[s] = at;  // -1: an id outside [0, E) takes no part
      if (at >= 0) sorted[at] = s;
    }
  }
}

// ---------------------------------------------------------------------------- grouped GEMMs
struct MoeGemmArgs {
  const bf16_t* X;       // GLU: x [M, ldx]; down: h [s_cap, K]
  const bf16_t* W;       // [E, N, K]
  const int* plan;
  const float* scale;    // GLU: rstd [M] or null; down (unsplit): routing weights [M k]
  void* out;             // GLU: h [s_cap, N / 2] bf16; down: [s_cap, N] bf16, SPLIT: [slabs, s_cap, N] fp32
  long ldx;
  int M, k, N, K, kg_steps;
  MoePlan pl;
};

// LDS images: rows of 8 16-B chunks, chunk ch of a row at position ch ^ (row >> 1) & 7
__device__ __forceinline__ int moe_swz(int row, int ch) { return row * MOE_BK + ((ch ^ ((row >> 1) & 7)) << 3); }

template <int TM, bool GLU, bool SPLIT>
__global__ void __launch_bounds__(256) moe_gemm_kernel(const MoeGemmArgs p) {
  static_assert(!(GLU && SPLIT), "only the down GEMM splits K");
  constexpr int XG = TM / 32;                      // 32-row groups = X DMA instructions per wave
  constexpr int W_ELEMS = MOE_BN * MOE_BK;         // 16 KB
  constexpr int STAGE_ELEMS = W_ELEMS + TM * MOE_BK;
  constexpr int PER = 4 + XG;
  extern __shared__ __attribute__((aligned(16))) uint8_t moe_smem[];
  bf16_t* ring = reinterpret_cast<bf16_t*>(moe_smem);
  const int tile = blockIdx.x;
  if (tile >= p.plan[0]) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int expert = __builtin_amdgcn_readfirstlane(p.plan[p.pl.tiles_off() + tile]);
  const int* sorted = p.plan + p.pl.sorted_off() + tile * TM;  // this tile's TM slots
  const long pos0 = (long)tile * TM;
  const int n0 = blockIdx.y * MOE_BN;
  const int ksteps = p.K / MOE_BK;
  const int t0 = blockIdx.z * p.kg_steps;
  const int nk = max(0, min(ksteps, t0 + p.kg_steps) - t0);

  const long w_bytes = (long)p.N * p.K * 2;
  const long x_bytes = GLU ? (long)p.M * p.ldx * 2 : (long)p.pl.s_cap * p.K * 2;
  const __amdgpu_buffer_rsrc_t rW = buf_rsrc(p.W + (long)expert * p.N * p.K, w_bytes);
  const __amdgpu_buffer_rsrc_t rX = buf_rsrc(p.X, x_bytes);
  // DMA geometry: a wave instruction fills 8 LDS rows x 128 B lane-linearly; the lane at chunk position lpos fetches
  // global chunk lpos ^ swizzle(row)
  const int lrow = lane >> 3, lpos = lane & 7;
  uint32_t woff[4], xoff[XG];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (w * 4 + j) * 8 + lrow, n = n0 + row, ch = lpos ^ ((row >> 1) & 7);
    woff[j] = n < p.N ? (uint32_t)(((long)n * p.K + ch * 8) * 2) : kDmaOob;
  }
#pragma unroll
  for (int j = 0; j < XG; ++j) {
    const int row = (w * XG + j) * 8 + lrow, ch = lpos ^ ((row >> 1) & 7);
    const int slot = sorted[row];
    const long src = GLU ? (long)(p.k == 2 ? slot >> 1 : slot) * p.ldx : (pos0 + row) * p.K;
    xoff[j] = slot >= 0 ? (uint32_t)((src + ch * 8) * 2) : kDmaOob;
  }
  auto stage = [&](int st, int kstep) {
    bf16_t* sw = ring + st * STAGE_ELEMS;
    bf16_t* sx = sw + W_ELEMS;
    const uint32_t k2 = (uint32_t)(kstep * MOE_BK * 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t off = woff[j] != kDmaOob ? woff[j] + k2 : kDmaOob;
      SHAI_DASSERT_DMA(off, w_bytes, kDmaOob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(sw + (w * 4 + j) * 8 * MOE_BK), 16, off, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < XG; ++j) {
      const uint32_t off = xoff[j] != kDmaOob ? xoff[j] + k2 : kDmaOob;
      SHAI_DASSERT_DMA(off, x_bytes, kDmaOob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (lds_void*)(sx + (w * XG + j) * 8 * MOE_BK), 16, off, 0, 0, 0);
    }
  };

  float16_ acc[XG];
#pragma unroll
  for (int g = 0; g < XG; ++g)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[g][i] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int i = 0; i < MOE_STAGES - 1; ++i)
    if (i < nk) stage(i, t0 + i);
  int buf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    wait_upto<PER, MOE_STAGES - 2>(min(MOE_STAGES - 2, nk - 1 - kt));
    __builtin_amdgcn_s_barrier();
    if (kt + MOE_STAGES - 1 < nk)  // into the buffer of step kt - 1: every wave is past it
      stage(buf == 0 ? MOE_STAGES - 1 : buf - 1, t0 + kt + MOE_STAGES - 1);
    const bf16_t* sw = ring + buf * STAGE_ELEMS;
    const bf16_t* sx = sw + W_ELEMS;
#pragma unroll
    for (int sl = 0; sl < MOE_BK / 16; ++sl) {
      const int ch = 2 * sl + fh;
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(sw + moe_swz(32 * w + fr, ch));
#pragma unroll
      for (int g = 0; g < XG; ++g) {
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(sx + moe_swz(32 * g + fr, ch));
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[g], 0, 0, 0);
      }
    }
    buf = buf == MOE_STAGES - 1 ? 0 : buf + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // lane (fr, fh) holds D[n][m] for row m = 32 g + fr and n = nbase + 8 q + e in register 4 q + e
  const int nbase = n0 + 32 * w + 4 * fh;
#pragma unroll
  for (int g = 0; g < XG; ++g) {
    const int m = 32 * g + fr;
    const int slot = sorted[m];
    if (slot < 0) continue;  // padding row
    if constexpr (GLU) {
      const float rs = p.scale ? p.scale[p.k == 2 ? slot >> 1 : slot] : 1.f;
      uint32_t* h = reinterpret_cast<uint32_t*>(static_cast<bf16_t*>(p.out) + (pos0 + m) * (p.N >> 1));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = nbase + 8 * q;  // pairs (value, gate) at n, n + 2 -> columns n / 2, n / 2 + 1
        if (n >= p.N) continue;
        const float o0 = (acc[g][4 * q] * rs) * silu_f(acc[g][4 * q + 1] * rs);
        const float o1 = (acc[g][4 * q + 2] * rs) * silu_f(acc[g][4 * q + 3] * rs);
        h[n >> 2] = pack2(o0, o1);
      }
    } else if constexpr (SPLIT) {
      float* o = static_cast<float*>(p.out) + ((long)blockIdx.z * p.pl.s_cap + pos0 + m) * p.N;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = nbase + 8 * q;
        if (n >= p.N) continue;
        *reinterpret_cast<float4_*>(o + n) =
            float4_{acc[g][4 * q], acc[g][4 * q + 1], acc[g][4 * q + 2], acc[g][4 * q + 3]};
      }
    } else {
      const float wt = p.scale[slot];
      bf16_t* o = static_cast<bf16_t*>(p.out) + (pos0 + m) * p.N;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = nbase + 8 * q;
        if (n >= p.N) continue;
        *reinterpret_cast<uint2_*>(o + n) = uint2_{pack2(acc[g][4 * q] * wt, acc[g][4 * q + 1] * wt),
                                                   pack2(acc[g][4 * q + 2] * wt, acc[g][4 * q + 3] * wt)};
      }
    }
  }
}

// ---------------------------------------------------------------------------- combine
// one thread per (row, 8 columns)
template <bool SPLIT>
__global__ void __launch_bounds__(256) moe_combine_kernel(const void* __restrict__ yslot,
                                                          const int* __restrict__ plan,
                                                          const float* __restrict__ wts,
                                                          const bf16_t* __restrict__ residual, long ldr,
                                                          bf16_t* __restrict__ y, int M, int k, int N, int slabs,
                                                          MoePlan pl) {
  const int chunks = N >> 3;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * chunks) return;
  const int m = (int)(i / chunks), c = (int)(i % chunks) * 8;
  const int* pos = plan + pl.pos_off();
  float sum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sum[e] = 0.f;
  for (int j = 0; j < k; ++j) {
    const int at = pos[m * k + j];
    if (at < 0) continue;
    float t[8];
    if constexpr (SPLIT) {
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = 0.f;
      for (int s = 0; s < slabs; ++s) {
        const float* src = static_cast<const float*>(yslot) + ((long)s * pl.s_cap + at) * N + c;
        const float4_ a = *reinterpret_cast<const float4_*>(src), b = *reinterpret_cast<const float4_*>(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t[e] += a[e];
          t[4 + e] += b[e];
        }
      }
      const float wt = wts[m * k + j];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = bf2f(f2bf(t[e] * wt));
    } else {
      unpack8(*reinterpret_cast<const uint4_*>(static_cast<const bf16_t*>(yslot) + (long)at * N + c), t);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] += t[e];
  }
  if (residual) {
    float r[8];
    unpack8(*reinterpret_cast<const uint4_*>(residual + (long)m * ldr + c), r);
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] += r[e];
  }
  *reinterpret_cast<uint4_*>(y + (long)m * N + c) = pack8(sum);
}

static MoePlan moe_make_plan(int M, int k, int E, int tm) {
  const int S = M * k, active = S < E ? S : E;
  MoePlan pl;
  pl.t_max = (S + active * (tm - 1)) / tm;  // sum over experts of ceil(count / tm) is at most this
  pl.s_cap = pl.t_max * tm;
  return pl;
}

template <int TM, bool GLU, bool SPLIT>
static void moe_launch_gemm(const MoeGemmArgs& a, int slabs, hipStream_t s) {
  const dim3 grid(a.pl.t_max, (a.N + MOE_BN - 1) / MOE_BN, slabs);
  const size_t lds = (size_t)MOE_STAGES * (MOE_BN + TM) * MOE_BK * 2;
  moe_gemm_kernel<TM, GLU, SPLIT><<<grid, 256, lds, s>>>(a);
}

// Row-tile height from M alone.  Measured on one Mixtral-shaped layer (H 4096, I 14336, 8 experts, top-2;
// profiles/moe_mixtral.md): the 128-row tile is faster from M = 32 (535 against 599 us; M = 64: 538 against 591 us)
// and far ahead from 256 rows, where the 32-row tile re-reads an expert's weights once per 32 of its rows; at M = 16
// the two are within 3 %.  Below 32 rows an expert sees a handful of rows and the 32-row tile stays.
int moe_tile_rows(int M) { return M < 32 ? 32 : 128; }

// Split count of the down GEMM from M alone: with one or two rows at most four experts are active, and H / 128
// column tiles each do not give every CU a workgroup.  Measured (same table): M = 1: 228 -> 171 us with 4 slabs,
// M = 2: 312 -> 272 us; from M = 4 the split changes nothing.  Each slab keeps at least 4 K steps.
int moe_down_splits(int M, int I) {
  int s = M <= 2 ? 4 : 1;
  while (s > 1 && I / MOE_BK / s < 4) s >>= 1;
  return s;
}

bool moe_supported(int M, int H, int I, int E, int k, int tm) {
  if (M < 1 || E < 2 || E > MOE_EMAX || k < 1 || k > 2 || H < 64 || I < 64 || H % 64 != 0 || I % 64 != 0) return false;
  if (tm != 32 && tm != 128) return false;
  const MoePlan pl = moe_make_plan(M, k, E, tm);
  // every DMA source sits behind one buffer descriptor (< 2 GiB): x, h, one expert's w13 / w2
  return (long)M * H * 2 < 0x7fffffffL && (long)pl.s_cap * I * 2 < 0x7fffffffL && (long)2 * I * H * 2 < 0x7fffffffL;
}

void moe_plan_dims(int M, int k, int E, int tm, int* s_cap, int* plan_words) {
  const MoePlan pl = moe_make_plan(M, k, E, tm);
  *s_cap = pl.s_cap;
  *plan_words = pl.pos_off() + M * k;
}

void launch_moe_route(const bf16_t* x, long ldx, const float* wg, int* ids, float* wts, float* rstd, int M, int H,
                      int E, int k, float eps, bool rms, hipStream_t s) {
  const int grid = (M + 15) / 16;
  if (E <= 8) moe_route_kernel<8><<<grid, 256, 0, s>>>(x, ldx, wg, ids, wts, rstd, M, H, E, k, eps, rms);
  else moe_route_kernel<16><<<grid, 256, 0, s>>>(x, ldx, wg, ids, wts, rstd, M, H, E, k, eps, rms);
  SHAI_CHECK_LAUNCH();
}

void launch_moe_glu(const bf16_t* x, long ldx, const bf16_t* w13, const int* ids, const float* rstd, int* plan,
                    bf16_t* h, int M, int H, int I, int E, int k, int tm, hipStream_t s) {
  const MoePlan pl = moe_make_plan(M, k, E, tm);
  if (tm == 32) moe_align_kernel<32><<<1, 256, 0, s>>>(ids, plan, M * k, E, pl);
  else moe_align_kernel<128><<<1, 256, 0, s>>>(ids, plan, M * k, E, pl);
  MoeGemmArgs a{x, w13, plan, rstd, h, ldx, M, k, 2 * I, H, H / MOE_BK, pl};
  if (tm == 32) moe_launch_gemm<32, true, false>(a, 1, s);
  else moe_launch_gemm<128, true, false>(a, 1, s);
  SHAI_CHECK_LAUNCH();
}

void launch_moe_down(const bf16_t* h, const bf16_t* w2, const int* plan, const float* wts, void* yslot,
                     const bf16_t* residual, long ldr, bf16_t* y, int M, int H, int I, int E, int k, int tm,
                     int splits, hipStream_t s) {
  const MoePlan pl = moe_make_plan(M, k, E, tm);
  const KSplit ks = split_ksteps(I / MOE_BK, splits);
  MoeGemmArgs a{h, w2, plan, wts, yslot, (long)I, M, k, H, I, ks.kg_steps, pl};
  const int cgrid = (int)(((long)M * (H / 8) + 255) / 256);
  if (splits > 1) {  // (the slab form also when the split count degenerates to 1: yslot is fp32 then)
    if (tm == 32) moe_launch_gemm<32, false, true>(a, ks.kg, s);
    else moe_launch_gemm<128, false, true>(a, ks.kg, s);
    moe_combine_kernel<true><<<cgrid, 256, 0, s>>>(yslot, plan, wts, residual, ldr, y, M, k, H, ks.kg, pl);
  } else {
    if (tm == 32) moe_launch_gemm<32, false, false>(a, 1, s);
    else moe_launch_gemm<128, false, false>(a, 1, s);
    moe_combine_kernel<false><<<cgrid, 256, 0, s>>>(yslot, plan, wts, residual, ldr, y, M, k, H, 1, pl);
  }
  SHAI_CHECK_LAUNCH();
}

}  // namespace shai

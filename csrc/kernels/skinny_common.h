// Shared pieces of the skinny (decode-shaped, M <= 64) GEMM family: gemv.hip (64-row tiles, a K step split over the
// waves), gemv2.hip / gemv_fp4.hip (128-row tiles, bf16 / MXFP4 weights: one body, skinny_rows_kernel below) and the
// fp4 fragment that gemm_fp4.hip shares with gemv_fp4.hip.
//
//   * device primitives: buffer descriptor, the DMA zero-fill sentinel, fragment typedefs, the write-through (sc1)
//     loads / stores and the arrival ticket of the in-launch split-K hand-off, the counted vmcnt wait, the pair / quad
//     epilogues, the e8m0 scale and e2m1 widen of MXFP4;
//   * skinny_rows_kernel<Fmt, MB, GLU, ACT, RMS, STAGES>: the wide body.  Fmt (WBf16 in gemv2.hip, WMxfp4 in
//     gemv_fp4.hip) says how a K step's bytes reach LDS and become bf16 fragments; ring, waits, folded RMSNorm,
//     epilogues and the split-K fixup are written once here;
//   * host helpers: the SHAI_SKINNY_NT switch, K-group arithmetic, the GLU x activation x RMS dispatch.
#pragma once
#include "common.h"
#include "launchers.h"
#include "gemm_epilogue.h"

#include <cstdlib>
#include <type_traits>

namespace shai {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void;

// a DMA / buffer offset at or above this is out of every (<= 2^31 - 1 byte) descriptor's range: zero fill
constexpr uint32_t kDmaOob = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)min(bytes, 0x7fffffffL),
                                           0x00020000);
}

// write-through (sc1) stores / loads of the in-launch split-K hand-off (cache policy bit sc1 = 16), 4 B and 16 B
__device__ __forceinline__ void store_wt(__amdgpu_buffer_rsrc_t r, uint32_t off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)off, 0, 16);
}
__device__ __forceinline__ float load_wt(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 16));
}
__device__ __forceinline__ void store4_wt(__amdgpu_buffer_rsrc_t r, uint32_t off, const float* v) {
  const uint4_ u = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
  __builtin_amdgcn_raw_buffer_store_b128(u, r, (int)off, 0, 16);
}
__device__ __forceinline__ float4_ load4_wt(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(float4_, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 16));
}

// s_waitcnt needs an immediate: allow `pending` (<= N) DMA groups of PER loads to stay in flight
template <int PER, int N>
__device__ __forceinline__ void wait_upto(int pending) {
  if constexpr (N == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    if (pending >= N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N * PER) : "memory");
    else wait_upto<PER, N - 1>(pending);
  }
}

// one output element (GLU: the pair n, n + 1) of row m < M: bias, activation (GLU: value * act(gate)), residual, bf16
// store -- tiles cut by N
template <bool GLU, int ACT>
__device__ __forceinline__ void pair_store(const GemmArgs& p, int n, int m, float v0, float v1) {
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
__device__ __forceinline__ void quad_out(const GemmArgs& p, int m, int n, float v[4]) {
  if (m >= p.M || n >= p.N) return;
  if (n + 3 < p.N) {
    epilogue4<GLU, ACT>(p, p.C, p.residual, m, n, v);
  } else if constexpr (GLU) {
    for (int e = 0; e < 4 && n + e + 1 < p.N; e += 2) pair_store<GLU, ACT>(p, n + e, m, v[e], v[e + 1]);
  } else {
    for (int e = 0; e < 4; ++e) pair_store<GLU, ACT>(p, n + e, m, v[e], 0.f);
  }
}

// The arrival step of the in-launch split-K fixup; true in every thread of the workgroup that arrived last.
// The hand-off follows the write-through publish form (cdna_hip_programming.md Guideline 16, R1 with sc1 consumer
// loads): every slab byte is stored sc1 by its writing wave, EVERY wave drains vmcnt(0) and joins a workgroup barrier
// BEFORE this call, the signal is an agent-scope atomic, and the last arriver reads the slabs ONLY with sc1 loads into
// registers (load_wt / load4_wt) -- no other load of the launch touches bytes another workgroup wrote.  So the ticket
// is relaxed and the acquire is a wavefront-scope fence (no instruction: it only keeps the compiler from hoisting the
// slab loads above the ticket).  An agent-scope acq_rel here (buffer_wbl2 + buffer_inv of the XCD's L2) measured -7 %
// Mistral decode.  The last arriver re-arms the ticket, so the slice serves the next launch on the stream / the next
// replay of the graph.  cnt[tile] is the tile's ticket; `flag` is an LDS word of the caller's that nothing else uses
// from that barrier on.
__device__ __forceinline__ bool last_arriver(unsigned* cnt, int tile, int KG, unsigned* flag, int tid) {
  if (tid == 0) {
    const unsigned old = __hip_atomic_fetch_add(&cnt[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    *flag = old == (unsigned)(KG - 1);
  }
  __syncthreads();
  if (*flag == 0u) return false;
  if (tid == 0) __hip_atomic_store(&cnt[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// MXFP4: 2^(byte - 127) as fp32.  The quantiser keeps bytes in [2, 252]; a zero-filled byte (rows >= N) reads as
// 2^-126 beside zero codes.
__device__ __forceinline__ float e8m0_scale(uint32_t byte) { return __uint_as_float(max(byte, 1u) << 23); }

// 8 e2m1 codes (one dword, even k in the low nibbles) x scale -> 8 bf16 (exact: code * power of two)
__device__ __forceinline__ bf16x8 fp4x8_widen(uint32_t codes, float scale) {
  bf16x8 r;
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 3);
  r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1];
  r[4] = c[0]; r[5] = c[1]; r[6] = d[0]; r[7] = d[1];
  return r;
}

// ---------------------------------------------------------------------------- the wide body
// Workgroup = 4 waves, tile = SR_BN = 128 W rows x all M rows of X (XG = MB / 32 groups of 32).  Wave w owns W rows
// [32 w, 32 w + 32) and consumes the WHOLE K step of them: no cross-wave reduction, its accumulators are its final
// (or split-K partial) outputs.  Accumulator layout of v_mfma_f32_32x32x16 with W rows as A and X rows as B: lane
// (fr = lane & 31, fh = lane >> 5) holds D[n][m] for m = 32 g + fr and n = 8 q + 4 fh + e in register 4 q + e
// (q, e = 0..3): quads of 4 consecutive n.
//
// A format policy Fmt supplies (see WBf16 in gemv2.hip, WMxfp4 in gemv_fp4.hip):
//   BK, SLICES              K per step; k16 slices of a step (BK / 16)
//   stage_bytes(MB), per(MB)  bytes of one ring stage; DMA instructions per wave per step (the counted vmcnt unit)
//   FOLD                    whether the separate-fold split-K form exists (cnt == nullptr, KG > 1)
//   QUAD_STORES             epilogue through quad_out (8-B stores) or element-wise pair_store
//   Lane<MB>                per-lane DMA state: init(p, n0, w, lane, ksteps) builds descriptors and source offsets,
//                           stage(p, st, w, kstep) issues one K step's LDS-DMA into the stage at st,
//                           w_frag(st, w, fr, fh, slice, xc) returns the W fragment of a k16 slice and the index xc
//                           of the X chunk holding the same k,
//                           x_frag(st, row, chunk) reads the X fragment of that chunk
constexpr int SR_BN = 128;  // W rows per workgroup

// rows m = 32 g + fr x this lane's 16 columns (quad q at nbase + 8 q): rstd from the row's sum of squares, then the
// fused epilogue in the format's store form (quads, or element-wise pairs)
template <bool QUADS, int XG, bool GLU, int ACT, bool RMS, class V>
__device__ __forceinline__ void rows_epilogue(const GemmArgs& p, int fr, int nbase, const V (&v)[XG],
                                              const float (&sq)[XG]) {
#pragma unroll
  for (int g = 0; g < XG; ++g) {
    const int m = 32 * g + fr;
    const float rs = RMS ? rsqrtf(sq[g] / p.K + p.rms_eps) : 1.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = nbase + 8 * q;
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = v[g][4 * q + e] * rs;
      if constexpr (QUADS) {
        quad_out<GLU, ACT>(p, m, n, o);
      } else if (m < p.M) {
        if constexpr (GLU) {
          pair_store<true, ACT>(p, n, m, o[0], o[1]);
          pair_store<true, ACT>(p, n + 2, m, o[2], o[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) pair_store<false, ACT>(p, n + e, m, o[e], 0.f);
        }
      }
    }
  }
}

template <class Fmt, int MB, bool GLU, int ACT, bool RMS, int STAGES>
__global__ void __launch_bounds__(256) skinny_rows_kernel(const GemmArgs p, float* __restrict__ ws, int kg_steps,
                                                          unsigned* __restrict__ cnt) {
  constexpr int XG = MB / 32;
  constexpr int STAGE_BYTES = Fmt::stage_bytes(MB), PER = Fmt::per(MB);
  using Lane = typename Fmt::template Lane<MB>;
  // ALL LDS of the kernel is this one array (the last-arriver flag of the fixup reuses the dead ring): a second
  // __shared__ object beside an LDS-DMA ring can make the compiler drain vmcnt before every step's first ds_read
  extern __shared__ __attribute__((aligned(16))) uint8_t sr_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, kg = blockIdx.y, KG = gridDim.y;
  const int n0 = tile * SR_BN;
  const int ksteps = (p.K + Fmt::BK - 1) / Fmt::BK;
  const int t0 = kg * kg_steps;
  const int nk = max(0, min(ksteps, t0 + kg_steps) - t0);

  Lane L;
  L.init(p, n0, w, lane, ksteps);

  float16_ acc[XG];
#pragma unroll
  for (int g = 0; g < XG; ++g)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[g][i] = 0.f;
  float ss[XG];  // folded RMSNorm: this lane's share of sum_k X[m, k]^2 (m = 32 g + fr; lanes fr, fr + 32 together
                 // read every X element of every step once -- the same in every wave, nothing to share)
#pragma unroll
  for (int g = 0; g < XG; ++g) ss[g] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int i = 0; i < STAGES - 1; ++i)
    if (i < nk) L.stage(p, sr_smem + i * STAGE_BYTES, w, t0 + i);
  int buf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    wait_upto<PER, STAGES - 2>(min(STAGES - 2, nk - 1 - kt));
    __builtin_amdgcn_s_barrier();
    if (kt + STAGES - 1 < nk) {
      const int nb = buf == 0 ? STAGES - 1 : buf - 1;  // buffer of step kt-1: every wave is past it
      L.stage(p, sr_smem + nb * STAGE_BYTES, w, t0 + kt + STAGES - 1);
    }
    const uint8_t* st = sr_smem + buf * STAGE_BYTES;
    // (a plain loop over the slices, not a callback handed to the policy: through a callback the bf16 step came out
    // with two MFMAs back to back behind a drained lgkmcnt(0), and 2.4-4.6 % slower at 28672 x 4096)
#pragma unroll
    for (int sl = 0; sl < Fmt::SLICES; ++sl) {
      int xc;
      const bf16x8 wf = L.w_frag(st, w, fr, fh, sl, xc);
#pragma unroll
      for (int g = 0; g < XG; ++g) {
        const bf16x8 xf = Lane::x_frag(st, 32 * g + fr, xc);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[g], 0, 0, 0);
        if constexpr (RMS) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float f = (float)xf[e];
            ss[g] = fmaf(f, f, ss[g]);
          }
        }
      }
    }
    buf = buf == STAGES - 1 ? 0 : buf + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (RMS) {  // both K halves of row m: lanes fr and fr + 32
#pragma unroll
    for (int g = 0; g < XG; ++g) ss[g] += __shfl_xor(ss[g], 32, 64);
  }
  const int nbase = n0 + 32 * w + 4 * fh;  // quad q of this lane: columns nbase + 8 q .. + 3
  if (KG == 1) {
    rows_epilogue<Fmt::QUAD_STORES, XG, GLU, ACT, RMS>(p, fr, nbase, acc, ss);
    return;
  }
  if constexpr (Fmt::FOLD) {
    if (cnt == nullptr) {
      // ---- split-K over workgroups, separate fold: fp32 partials [kg][M][N] then [kg][M] row sums of squares;
      // launch_splitk_epilogue reduces them and runs the epilogue
      float* part = ws + (long)kg * p.M * p.N;
#pragma unroll
      for (int g = 0; g < XG; ++g) {
        const int m = 32 * g + fr;
        if (m >= p.M) continue;
        if constexpr (RMS) {
          if (tile == 0 && w == 0 && fh == 0) ws[(long)KG * p.M * p.N + (long)kg * p.M + m] = ss[g];
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
  }
  // ---- split-K fixed up in this launch: slab [tile][kg] = 4 XG chunks of 256 lanes x 4 floats (chunk = one quad
  // register group: coalesced 16-B stores / loads, 4 KB per wave instruction) + MB row sums of squares, published and
  // collected in the write-through form (last_arriver above)
  constexpr int SLAB = SR_BN * MB + MB, NCH = 4 * XG;
  float v[XG][16];
#pragma unroll
  for (int g = 0; g < XG; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) v[g][r] = acc[g][r];
  const __amdgpu_buffer_rsrc_t rws = buf_rsrc(ws, 0x7fffffffL);
  const uint32_t tile_base = (uint32_t)((long)tile * KG * SLAB * 4);
  const uint32_t my_base = tile_base + (uint32_t)(kg * SLAB * 4);
  auto chunk_off = [&](int c) { return (uint32_t)((c * 256 + tid) * 16); };
  auto ss_off = [&](int g) { return (uint32_t)((SR_BN * MB + 32 * g + fr) * 4); };
#pragma unroll
  for (int c = 0; c < NCH; ++c) store4_wt(rws, my_base + chunk_off(c), &v[c >> 2][(c & 3) * 4]);
  if constexpr (RMS) {
    if (w == 0 && fh == 0) {
#pragma unroll
      for (int g = 0; g < XG; ++g) store_wt(rws, my_base + ss_off(g), ss[g]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // also: every wave is done with the ring, its first word now carries the last-arriver flag
  if (!last_arriver(cnt, tile, KG, reinterpret_cast<unsigned*>(sr_smem), tid)) return;
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
    float4_ t[2][NCH];
    float ts[2][XG];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = q0 + u < KG ? q0 + u : kg;  // past KG / own slot: re-read own slab, dropped below
      const uint32_t b = tile_base + (uint32_t)(q * SLAB * 4);
#pragma unroll
      for (int c = 0; c < NCH; ++c) t[u][c] = load4_wt(rws, b + chunk_off(c));
#pragma unroll
      for (int g = 0; g < XG; ++g) {
        ts[u][g] = 0.f;
        if constexpr (RMS) ts[u][g] = load_wt(rws, b + ss_off(g));
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
        for (int r = 0; r < 16; ++r) sum[g][r] += mine ? v[g][r] : t[u][4 * g + (r >> 2)][r & 3];
        ssum[g] += mine ? ss[g] : ts[u][g];
      }
    }
  }
  rows_epilogue<Fmt::QUAD_STORES, XG, GLU, ACT, RMS>(p, fr, nbase, sum, ssum);
}

// ---------------------------------------------------------------------------- host side
// SHAI_SKINNY_NT=0: the weight stream of the skinny kernels without the nt cache policy (default 1: weights are read
// once per decode step by one CU, and nt shortens issued -> landed; MI355X_MICROARCH nt-weights)
inline int skinny_nt() {
  static const int nt = [] {
    const char* e = getenv("SHAI_SKINNY_NT");
    return e ? atoi(e) : 1;
  }();
  return nt;
}

// largest K-group count worth trying (autotuner): groups of at least 2 K steps, at most 16
inline int max_kgroups(int ksteps) {
  int kg = 1;
  while (kg < 16 && ksteps / (kg * 2) >= 2) kg *= 2;
  return kg;
}

// kg K groups over ksteps steps: at least one group and one step per group, and no empty K groups (their partials
// would be zeros to fold, and their tickets would never arrive)
struct KSplit {
  int kg, kg_steps;
};
inline KSplit split_ksteps(int ksteps, int kg) {
  if (kg < 1) kg = 1;
  if (kg > ksteps) kg = ksteps;
  const int kg_steps = (ksteps + kg - 1) / kg;
  return {(ksteps + kg_steps - 1) / kg_steps, kg_steps};
}

// Epilogue dispatch of the launchers: calls f(glu, act, rms) with std::integral_constant arguments for the problem's
// GLU flag, activation and folded RMSNorm.  ACTS / GLU_ACTS are bit sets (act_bit) of the activations a launcher
// instantiates without / with GLU; any other activation runs as DFLT / GLU_DFLT.  RMS_FORMS = false: no folded-RMSNorm
// instantiations (rms is always false_type).
constexpr unsigned act_bit(int act) { return 1u << act; }
constexpr unsigned kActsAll = act_bit(ACT_SILU) | act_bit(ACT_GELU) | act_bit(ACT_GELU_TANH) |
                              act_bit(ACT_QUICK_GELU) | act_bit(ACT_RELU);

template <unsigned ACTS, int DFLT, class F>
inline void dispatch_act(int act, F&& f) {
#define SHAI_ACT_CASE(A)                                  \
  case A:                                                 \
    if constexpr ((ACTS & act_bit(A)) != 0) {             \
      f(std::integral_constant<int, A>{});                \
      return;                                             \
    }                                                     \
    break;
  switch (act) {
    SHAI_ACT_CASE(ACT_SILU)
    SHAI_ACT_CASE(ACT_GELU)
    SHAI_ACT_CASE(ACT_GELU_TANH)
    SHAI_ACT_CASE(ACT_QUICK_GELU)
    SHAI_ACT_CASE(ACT_RELU)
    default: break;
  }
#undef SHAI_ACT_CASE
  f(std::integral_constant<int, DFLT>{});
}

template <unsigned ACTS, unsigned GLU_ACTS = ACTS, int GLU_DFLT = ACT_NONE, bool RMS_FORMS = true, class F>
inline void dispatch_epilogue(const GemmArgs& a, F&& f) {
  auto with_rms = [&](auto glu, auto act) {
    if constexpr (RMS_FORMS) {
      if (a.rms) return f(glu, act, std::true_type{});
    }
    f(glu, act, std::false_type{});
  };
  if (a.glu) dispatch_act<GLU_ACTS, GLU_DFLT>(a.act, [&](auto act) { with_rms(std::true_type{}, act); });
  else dispatch_act<ACTS, ACT_NONE>(a.act, [&](auto act) { with_rms(std::false_type{}, act); });
}

}  // namespace shai

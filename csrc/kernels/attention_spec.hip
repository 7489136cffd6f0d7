// Speculative-decoding verify attention: T <= 8 query tokens per sequence (the last accepted token and up to 7
// drafts) against the paged bf16 KV cache, causal among themselves.
//
// One work item per (sequence, KV head, split), the decode kernel's split rule (da_splits) and persistent rotated
// walk.  The R = T * G <= 64 query rows of a KV head (G = Hq / Hkv, row r = t * G + g) are one MFMA tile set: wave w
// holds rows 32 w .. 32 w + 31 as the columns of the swapped S^T = K Q^T form of flash_v1.h (v_mfma_f32_32x32x16_bf16:
// a lane owns one query row, so the online softmax needs one cross-half shuffle and no LDS), and the item's 64-token
// K/V blocks arrive ONCE, by LDS-DMA into a two-slot ring in the XOR-swizzled layout the fragment reads expect (the
// swizzle is applied on the source side of the DMA, as in decode_common.h).  Per-block buffer descriptors range-check
// the rows at or past the context: zero-filled (P = 0 times a never-written NaN pattern would poison P.V).
//
// Determinism (one split): a row's m, l and o are functions of its q and of its visible keys in block order only.
// The MFMA computes every column independently, the mask sets a hidden key's P to exactly 0, and the running max is
// updated exactly per row and block (no deferred rescale, whose decision would look at the other rows): a block that
// is fully masked for a row multiplies its l and o by exp2(0) = 1 and adds zeros.  The engine's acceptance test rests
// on this: a token verified as draft row t gives the logits it would have given as row 0 of a later step.
//
// P enters P.V as bf16 (RNE), accumulation is fp32, the row sum adds the unrounded P (as the flash kernels).
// One split writes o; more leave {m, l, o[D]} partials per (b, t, head, split) for spec_combine_kernel.
#include "decode_common.h"
#include "flash_v1.h"

namespace shai {

// chunk XOR of K / V row `row` in the LDS tiles: k_swz / v_swz of flash_v1.h as a source-side swizzle
template <int D>
__device__ __forceinline__ int spec_ksw(int row) {
  if constexpr (D == 128) return row & 15;
  else return (row >> 1) & 7;
}
template <int D>
__device__ __forceinline__ int spec_vsw(int row) {
  if constexpr (D == 128) return (row & 3) << 2;
  else return ((row >> 1) & 1) << 2;
}

template <int D, int NQ>
__device__ __forceinline__ void spec_attn_item(const SpecAttnArgs& p, bf16_t* ring, const int b, const int hk,
                                               const int split) {
  constexpr int CPR = D / 8, RPI = 1024 / (2 * D);
  constexpr int NB = 2 * 64 * D * 2 / 1024;   // 1-KB wave DMA instructions per block (K, then V)
  constexpr int NI = NB / NQ;                 // ... per wave
  constexpr int SLOT = 2 * 64 * D;            // elements per ring slot (K then V)
  constexpr int NS = D / 16, ND = D / 32;
  static_assert(NI % 2 == 0, "a wave's instructions split evenly into K and V");
  const int G = p.Hq / p.Hkv;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 31, fh = lane >> 5;
  const int ctx = p.ctx_lens[b];
  const int qlen = min(p.q_lens[b], p.T);
  const int nblk = (ctx + 63) / 64;
  const int nsp = da_splits(nblk, p.num_splits);
  if (split >= nsp) return;
  const int per = (nblk + nsp - 1) / nsp;
  const int blk0 = split * per, blk1 = min(nblk, blk0 + per);

  // this lane's query row: r = t * G + g
  const int r = w * 32 + fr;
  const int t = r / G, g = r - t * G;
  const int hq = hk * G + g;
  const bool in_tile = t < p.T;          // a row of the [T, G] tile (stored)
  const bool valid = t < qlen;           // ... that holds a query
  // keys 0 .. vis - 1 are visible; a row without a query sees none (its output is 0)
  const int vis = valid ? max(0, min(ctx, ctx - qlen + t + 1)) : 0;
  const bool wave_active = w * 32 < qlen * G;   // (uniform) some row of this wave holds a query

  const int* bt = p.block_table + (long)b * p.max_blocks;
  int chunk0 = blk0;
  int my_phys = (blk0 + lane < blk1) ? bt[blk0 + lane] : 0;
  auto phys_of = [&](int bi) {
    if (bi - chunk0 >= 64) {
      chunk0 += 64;
      my_phys = (chunk0 + lane < blk1) ? bt[chunk0 + lane] : 0;
    }
    return __builtin_amdgcn_readfirstlane(__shfl(my_phys, bi - chunk0, 64));
  };
  // wave w issues instructions j = w + NQ * i (i < NI); j < NB / 2 is K, i.e. i < NI / 2
  auto stage = [&](int slot, int bi) {
    const int phys = phys_of(bi);
    const long base = ((long)phys * p.Hkv + hk) * 64 * D;
    const __amdgpu_buffer_rsrc_t rk =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.k_cache + base), (short)0, 64 * D * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.v_cache + base), (short)0, 64 * D * 2, 0x00020000);
    bf16_t* dst = ring + slot * SLOT;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      constexpr int kHalf = NI / 2;
      const bool isv = i >= kHalf;
      const int jj = w + NQ * (isv ? i - kHalf : i);      // instruction within the operand: 0 .. NB / 2 - 1
      const int row = jj * RPI + lane / CPR;              // this lane's row and LDS chunk position
      const int pos = lane % CPR;
      const int ch = pos ^ (isv ? spec_vsw<D>(row) : spec_ksw<D>(row));
      const uint32_t off = (bi * 64 + row < ctx) ? (uint32_t)((row * D + ch * 8) * 2) : 0x80000000u;
      SHAI_DASSERT_DMA(off, 64 * D * 2, 0x80000000u);
      SHAI_DASSERT(jj * 1024 + 1024 <= 64 * D * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isv ? rv : rk, (da_lds_void*)(dst + (isv ? 64 * D : 0) + jj * 512), 16,
                                               off, 0, 0, 0);
    }
  };

  if (blk0 < blk1) stage(0, blk0);

  // Q fragments (B operand of S^T = K Q^T): Q[row][16 s + 8 fh .. + 7]; rows without a query are zero
  bf16x8 qf[NS];
  {
    const bf16_t* qp = p.q + ((long)b * p.T + (valid ? t : 0)) * p.q_ts + (long)(valid ? hq : hk * G) * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      uint4_ v = *reinterpret_cast<const uint4_*>(qp + 16 * s + 8 * fh);
      if (!valid) v = uint4_{0u, 0u, 0u, 0u};
      qf[s] = __builtin_bit_cast(bf16x8, v);
    }
  }

  float16_ o[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[d][e] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float sl2 = p.scale * kLog2e;
  // lane roles for the transposed V reads
  const int g16 = lane >> 4, i16 = lane & 15;
  const int tq = i16 >> 2, tp = i16 & 3;

  for (int bi = blk0, slot = 0; bi < blk1; ++bi, slot ^= 1) {
    if (bi + 1 < blk1) {
      stage(slot ^ 1, bi + 1);
#if SHAI_DEBUG
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");  // block bi landed, bi + 1 in flight
#endif
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // raw barrier: __syncthreads' fence would drain the ring (vmcnt(0)) and serialise the prefetch
    __builtin_amdgcn_s_barrier();
    const bf16_t* ks = ring + slot * SLOT;
    const bf16_t* vs = ks + 64 * D;
    const int key0 = bi * 64;
    if (wave_active) {
      // ---- S^T = K Q^T for two 32-key blocks
      float16_ sacc[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[kb][e] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + k_swz<D>(kb * 32 + fr, 2 * s + fh));
          sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sacc[kb], 0, 0, 0);
        }
      }
      // ---- mask, exact per-row running max, exp2
      float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = key0 + kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
          sacc[kb][e] = key < vis ? sacc[kb][e] * sl2 : -INFINITY;
          m4[e & 3] = fmaxf(m4[e & 3], sacc[kb][e]);
        }
      float mloc = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
      const float m_new = fmaxf(m_run, mloc);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);   // 1 when the max did not move, 0 from -inf
      m_run = m_new;
      float ls4[4] = {0.f, 0.f, 0.f, 0.f};
      bf16x8 pf[2][2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float ex = __builtin_amdgcn_exp2f(sacc[kb][e] - m_use);   // hidden key: exp2(-inf) = 0
          sacc[kb][e] = ex;
          ls4[e & 3] += ex;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 v;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = (__bf16)sacc[kb][8 * s + j];
          pf[kb][s] = v;
        }
      }
      l_run = l_run * alpha + ((ls4[0] + ls4[1]) + (ls4[2] + ls4[3]));
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[d][e] *= alpha;
      // ---- O^T += V^T P^T
#pragma unroll
      for (int d = 0; d < ND; ++d) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int r0 = kb * 32 + 16 * s + 4 * fh + tq;
            const int col = d * 32 + 16 * (g16 & 1) + 4 * tp;
            const int ch = col >> 3, half = (col >> 2) & 1;
            const bf16_t* a0 = vs + v_swz<D>(r0, ch) + 4 * half;
            const bf16_t* a1 = vs + v_swz<D>(r0 + 8, ch) + 4 * half;
            const s4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a0));
            const s4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a1));
            short8 vv;
            vv[0] = t0[0]; vv[1] = t0[1]; vv[2] = t0[2]; vv[3] = t0[3];
            vv[4] = t1[0]; vv[5] = t1[1]; vv[6] = t1[2]; vv[7] = t1[3];
            o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vv), pf[kb][s], o[d], 0, 0, 0);
          }
        }
      }
    }
    __builtin_amdgcn_s_barrier();  // every wave is done with this slot before it is refilled (block bi + 2)
  }

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if (!in_tile) return;
  if (nsp == 1) {  // one split: normalise and write the output here (the combine skips these rows)
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    bf16_t* op = p.o + ((long)b * p.T + t) * p.o_ts + (long)hq * D;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int dd = d * 32 + 8 * q4 + 4 * fh;
        uint2_ wv;
        wv[0] = pack2(o[d][4 * q4] * inv, o[d][4 * q4 + 1] * inv);
        wv[1] = pack2(o[d][4 * q4 + 2] * inv, o[d][4 * q4 + 3] * inv);
        *reinterpret_cast<uint2_*>(op + dd) = wv;
      }
    }
    return;
  }
  // partial results: ws[b * T + t][hq][split] = {m, l, o[D]}
  float* dst = p.ws + ((((long)b * p.T + t) * p.Hq + hq) * p.num_splits + split) * (D + 2);
  if (fh == 0) {
    dst[0] = m_run;
    dst[1] = l_tot;
  }
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int dd = d * 32 + 8 * q4 + 4 * fh;
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[2 + dd + j] = o[d][4 * q4 + j];
    }
}

template <int D, int NQ>
__global__ void __launch_bounds__(NQ * 64) spec_attn_kernel(const SpecAttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) bf16_t spec_smem[];
  const int total = p.B * p.Hkv * p.num_splits;
  const int S = p.num_splits;
  const bool rotate = (int)gridDim.x < total;  // persistent walk only
  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    // (a sequence's splits sit at slots rotated by b, as in decode_attn_kernel)
    const int sidx = item % S, rr = item / S;
    const int b = rr / p.Hkv, hk = rr - b * p.Hkv;
    const int split = rotate ? (sidx - b % S + S) % S : sidx;
    spec_attn_item<D, NQ>(p, spec_smem, b, hk, split);
    __syncthreads();  // the next item restages ring slot 0
  }
}

// Fold of the split partials of row (b, t), head hq: decode_combine_kernel's arithmetic with (b, t) as the row.  A row
// without a query (t >= q_lens[b]) has l = 0 in every split and comes out as zeros.
__global__ void spec_combine_kernel(const SpecAttnArgs p) {
  const int row = blockIdx.x, hq = blockIdx.y;
  const int b = row / p.T;
  const int D = p.D;
  const int nsp = da_splits((p.ctx_lens[b] + 63) / 64, p.num_splits);
  if (nsp == 1) return;  // written by the attention workgroup itself
  const float* src = p.ws + ((long)row * p.Hq + hq) * p.num_splits * (D + 2);
  float m = -INFINITY;
  for (int s = 0; s < nsp; ++s) m = fmaxf(m, src[s * (D + 2)]);
  float l = 0.f;
  for (int s = 0; s < nsp; ++s) {
    const float ms = src[s * (D + 2)];
    if (ms != -INFINITY) l += src[s * (D + 2) + 1] * exp2f(ms - m);
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float acc = 0.f;
    for (int s = 0; s < nsp; ++s) {
      const float ms = src[s * (D + 2)];
      if (ms != -INFINITY) acc += src[s * (D + 2) + 2 + d] * exp2f(ms - m);
    }
    p.o[(long)row * p.o_ts + (long)hq * D + d] = f2bf(acc * inv);
  }
}

size_t spec_attn_workspace(int B, int T, int Hq, int D, int num_splits) {
  return (size_t)B * T * Hq * num_splits * (D + 2) * sizeof(float);
}

template <int D>
static void launch_spec(const SpecAttnArgs& a, dim3 grid, int nq, hipStream_t s) {
  const size_t lds = (size_t)2 * 2 * 64 * D * sizeof(bf16_t);   // two ring slots of K + V: 64 KB at D = 128
  if (nq == 1) spec_attn_kernel<D, 1><<<grid, 64, lds, s>>>(a);
  else spec_attn_kernel<D, 2><<<grid, 128, lds, s>>>(a);
}

void launch_spec_attn(const SpecAttnArgs& a, hipStream_t s) {
  const int G = a.Hq / a.Hkv;
  const int nq = (a.T * G + 31) / 32;   // waves: 32 query rows each (T * G <= 64)
  static const int width = [] {        // two workgroups per CU, as launch_decode_attn
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      cus = 256;
    return 2 * cus;
  }();
  const long items = (long)a.B * a.Hkv * a.num_splits;
  const bool persist = a.num_splits > 8;
  const dim3 grid((unsigned)(persist ? std::min<long>(items, width) : items));
  if (a.D == 128) launch_spec<128>(a, grid, nq, s);
  else launch_spec<64>(a, grid, nq, s);
  if (a.num_splits > 1) spec_combine_kernel<<<dim3(a.B * a.T, a.Hq), 128, 0, s>>>(a);
}

}  // namespace shai

// Fused temperature / top-k / top-p / multinomial sampling, one workgroup per
// sequence (the reference relies on Neuron on-device sampling with
// global_topk 64, cova/mllama-32-11b-vllm-trn1-config.yaml:19-22, and on vLLM's
// sampler with temperature 0.7 / top-k 50 / top-p 0.9, app/vllm_model_api.py:24).
//
// Replaces the topk -> softmax -> cumsum -> mask -> multinomial -> gather chain
// (six launches and a [B, V] fp32 copy) with one kernel:
//   1. exact K-th largest logit by 4-pass byte radix select over order-preserving
//      uint32 keys (wave-private LDS histograms, row re-read from L2 each pass);
//   2. gather exactly K candidates (of the keys equal to the K-th, the lowest indices) into LDS;
//   3. bitonic sort of the candidates (descending value, ascending index: deterministic);
//   4. p_i = exp((l_i - l_0) / T), inclusive block scan, nucleus cut at top_p
//      (keep i while the mass BEFORE i is <= top_p of the total -- the same rule
//      as the torch reference path), draw with a host-supplied uniform.
// Temperature <= 0 rows are greedy (K = 1).  Same distribution as
// shai_amd.engines.llm.sample(); the uniforms come from the engine's generator.
//
// The penalised instantiation (launch_sample_penalized) is the same body with three additions: the logit load
// applies the repetition / frequency / presence penalties from the row's penalty-state words (one int32 per
// vocabulary entry: bit 30 = the token occurs in the prompt, bits 0..29 = how often it was sampled), stage 4 drops
// the candidates with p_i < min_p before the nucleus cut, and the picked token's count is incremented at the end,
// so the state is current in stream order for the next (look-ahead) step.  Steps 1-3 are shared, as device
// functions, with token_logprobs_kernel (log-softmax of the raw logits at the picked token and at the top N).
//
// The constrained sampler (sample_con_kernel, launch_sample_constrained) is the penalised body once more with the
// ConLoad policy: + bias before the penalties, -inf after them where the row's automaton state does not allow the
// token (or the row bans its stop set).  Candidates at -inf are cut with min_p, so a masked token is never returned,
// and the pick advances the row's state word (one thread, a binary search of the state's edge list) in the same
// launch.  A row without a program takes exactly the penalised path.
#include "common.h"
#include "launchers.h"

namespace shai {

constexpr int SMP_T = 1024;          // threads per row
constexpr int SMP_MAXK = 1024;       // candidates kept in LDS
constexpr int SMP_WAVES = SMP_T / 64;
constexpr int PEN_PROMPT = 1 << 30;  // penalty-state word: prompt flag; the bits below it count sampled occurrences
constexpr int PEN_COUNT = PEN_PROMPT - 1;

__device__ __forceinline__ uint32_t f2key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool BF16>
__device__ __forceinline__ float smp_load(const void* row, int i) {
  if constexpr (BF16) return bf2f(reinterpret_cast<const bf16_t*>(row)[i]);
  else return reinterpret_cast<const float*>(row)[i];
}

// the raw logits of one row
template <bool BF16>
struct RawLoad {
  const char* base;
  __device__ __forceinline__ float operator()(int i) const { return smp_load<BF16>(base, i); }
};

// the penalised logits of one row (st: its state words, or null): every pass of the sampler re-reads the row
// through this one function, and contraction is off in it, so every pass sees the same value -- the value the
// fp32 oracle computes (IEEE division; no fma across the penalty steps)
template <bool BF16>
struct PenLoad {
  const char* base;
  const int* st;
  float r, f, p;
  __device__ __forceinline__ float pen(float l, int i) const {
#pragma clang fp contract(off)
    if (st) {
      const int wd = st[i];
      if (wd != 0) {
        const int c = wd & PEN_COUNT;
        l = l > 0.f ? l / r : l * r;
        const float fc = f * (float)c;
        l = l - fc;
        if (c > 0) l = l - p;
      }
    }
    return l;
  }
  __device__ __forceinline__ float operator()(int i) const { return pen(smp_load<BF16>(base, i), i); }
};

// ---- constraint programs (the layout is ops/reference.py's con_pack): CON_HDR header words, then the sections
constexpr int CON_HDR = 8;
constexpr int CON_MAX_STATES = 1024;
constexpr int CON_MAX_BIAS = 300;

// one row's program, resolved from the pool (ok = false: the row is unconstrained)
struct ConProg {
  bool ok;
  int S, W, E, NB;
  const int *masks, *stop, *plane, *dflt, *estart, *etok, *enext, *bid, *bval;
};

__device__ __forceinline__ ConProg con_resolve(const int* pool, long pool_words, long off, int V) {
  ConProg c{};
  if (!pool || off < 0 || off + CON_HDR > pool_words) return c;
  const int* h = pool + off;
  const int S = h[0], W = h[1], E = h[2], NB = h[3], total = h[4];
  const bool shape = S >= 1 && S <= CON_MAX_STATES && W == (V + 31) / 32 && E >= 0 && NB >= 0 && NB <= CON_MAX_BIAS;
  const long want = (long)CON_HDR + (long)S * W + 2L * W + S + (S + 1) + 2L * E + 2L * NB;
  SHAI_DASSERT(shape && total == want && off + want <= pool_words);
  if (!shape || total != want || off + want > pool_words) return c;
  c.S = S, c.W = W, c.E = E, c.NB = NB;
  c.masks = h + CON_HDR;
  c.stop = c.masks + (long)S * W;
  c.plane = c.stop + W;
  c.dflt = c.plane + W;
  c.estart = c.dflt + S;
  c.etok = c.estart + S + 1;
  c.enext = c.etok + E;
  c.bid = c.enext + E;
  c.bval = c.bid + NB;
  c.ok = true;
  return c;
}

// the constrained logits of one row: raw, + bias (the list, in LDS, is searched only for tokens the bias plane
// flags), the penalties, then -inf unless the state's mask (minus the stop mask when the row bans it) has the token's
// bit.  Lanes of a wave read consecutive tokens, so a wave instruction touches two mask words (one cache line).
// mask == null: the penalised logits.  Contraction is off as in PenLoad.
template <bool BF16>
struct ConLoad {
  PenLoad<BF16> pl;
  const int *mask, *stop, *plane;  // stop / plane: null = none
  const int* bid;                  // LDS
  const float* bval;               // LDS
  int nb;
  __device__ __forceinline__ float operator()(int i) const {
#pragma clang fp contract(off)
    float l = smp_load<BF16>(pl.base, i);
    if (!mask) return pl.pen(l, i);
    const int wi = i >> 5, bit = i & 31;
    if (plane && ((plane[wi] >> bit) & 1)) {
      int lo = 0, hi = nb;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bid[mid] < i) lo = mid + 1;
        else hi = mid;
      }
      if (lo < nb && bid[lo] == i) l = l + bval[lo];
    }
    l = pl.pen(l, i);
    int m = mask[wi];
    if (stop) m &= ~stop[wi];
    return ((m >> bit) & 1) ? l : -INFINITY;
  }
};

// Steps 1-3 for one row: the K largest values of load(0..V-1) into cval / cidx (SMP_MAXK entries each), sorted by
// descending value then ascending index; returns how many (K, 1 <= K <= min(V, SMP_MAXK)).  KEY16: the values are
// widened bf16 (two radix digits fix the threshold).  All SMP_T threads of the workgroup call it together.
template <bool KEY16, class Load>
__device__ __forceinline__ int smp_topk(const Load& load, int V, int K, float* cval, int* cidx) {
  // 4 histogram copies per wave (by lane & 3): logits crowd into a few exponent bins, and same-address LDS
  // atomics of one wave instruction serialise -- the copies cut the worst case from 64-way to 16-way
  __shared__ uint32_t hist[SMP_WAVES][4][256];
  __shared__ uint32_t tot[256];
  __shared__ uint32_t s_prefix, s_k, s_cnt, s_eq;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  SHAI_DASSERT(K >= 1 && K <= V && K <= SMP_MAXK);
  // ---- 1. radix select: key threshold with count(key > thr) < K <= count(key >= thr)
  if (tid == 0) {
    s_prefix = 0;
    s_k = K;
  }
  uint32_t mask = 0;
  // bf16 logits: the low 16 bits of a key are fixed by its sign, so the top two digits already fix the threshold
  for (int pass = 3; pass >= (KEY16 ? 2 : 0); --pass) {
    for (int i = tid; i < SMP_WAVES * 4 * 256; i += SMP_T) (&hist[0][0][0])[i] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    const int sh = 8 * pass;
    for (int i = tid; i < V; i += SMP_T) {
      const uint32_t key = f2key(load(i));
      if ((key & mask) == prefix) atomicAdd(&hist[w][lane & 3][(key >> sh) & 255], 1u);
    }
    __syncthreads();
    if (tid < 256) {
      uint32_t s = 0;
#pragma unroll
      for (int q = 0; q < SMP_WAVES; ++q) s += (hist[q][0][tid] + hist[q][1][tid]) + (hist[q][2][tid] + hist[q][3][tid]);
      tot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t k = s_k, above = 0;
      int b = 255;
      for (; b > 0; --b) {
        if (above + tot[b] >= k) break;
        above += tot[b];
      }
      s_k = k - above;
      s_prefix = prefix | ((uint32_t)b << sh);
      s_eq = tot[b];  // after the last pass: how many elements equal the threshold key
    }
    mask |= 255u << sh;
    __syncthreads();
  }
  uint32_t thr = s_prefix;
  // (bf16: a negative value's key has its low 16 bits all ones, a positive value's all zeros)
  if (KEY16 && !(thr & 0x80000000u)) thr |= 0xFFFFu;
  const uint32_t ties = s_k;  // how many elements equal to thr to keep
  // ---- 2. gather exactly K candidates: every key above the threshold, and of the keys equal to it the
  // `ties` with the lowest vocabulary indices (deterministic; when every equal key is kept no ordering is
  // needed, otherwise every wave counts the equal keys of its row chunk, then ranks them in index order)
  const bool all_ties = s_eq <= ties;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int i = tid; i < V; i += SMP_T) {
    const float v = load(i);
    const uint32_t key = f2key(v);
    if (key > thr || (all_ties && key == thr)) {
      const uint32_t slot = atomicAdd(&s_cnt, 1u);
      if (slot < (uint32_t)SMP_MAXK) {
        cval[slot] = v;
        cidx[slot] = i;
      }
    }
  }
  __syncthreads();
  if (!all_ties) {  // ordered selection of the `ties` lowest-index equal keys: wave w owns chunk w of the row
    __shared__ uint32_t tie_cnt[SMP_WAVES];
    const int C = ((V + SMP_WAVES - 1) / SMP_WAVES + 63) & ~63;
    const int c0 = w * C, c1 = min(V, c0 + C);
    uint32_t mine = 0;
    for (int i0 = c0; i0 < c1; i0 += 64) {
      const int i = i0 + lane;
      mine += __popcll(__ballot(i < c1 && f2key(load(i)) == thr));
    }
    if (lane == 0) tie_cnt[w] = mine;
    __syncthreads();
    uint32_t rank0 = 0;
    for (int q = 0; q < w; ++q) rank0 += tie_cnt[q];
    const uint32_t above = s_cnt;
    for (int i0 = c0; i0 < c1 && rank0 < ties; i0 += 64) {
      const int i = i0 + lane;
      const float v = i < c1 ? load(i) : 0.f;
      const bool eq = i < c1 && f2key(v) == thr;
      const unsigned long long bal = __ballot(eq);
      const uint32_t rank = rank0 + __popcll(bal & ((1ull << lane) - 1ull));
      if (eq && rank < ties && above + rank < (uint32_t)SMP_MAXK) {
        cval[above + rank] = v;
        cidx[above + rank] = i;
      }
      rank0 += __popcll(bal);
    }
    __syncthreads();
    if (tid == 0) s_cnt = above + ties;
  }
  __syncthreads();
  const int n = min((int)s_cnt, SMP_MAXK);
  SHAI_DASSERT(n == K);
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += SMP_T)
    if (i >= n) {
      cval[i] = -INFINITY;
      cidx[i] = -1;
    }
  __syncthreads();
  // ---- 3. bitonic sort, descending by value, ties by ascending index (a total order: the result does not
  // depend on the gather's slot order)
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += SMP_T) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const bool desc = (i & k2) == 0;
          const float a = cval[i], b = cval[ixj];
          const int ia = cidx[i], ib = cidx[ixj];
          // "b ranks before a": larger value, or equal value and smaller index (padding: -inf, index -1)
          const bool b_first = b > a || (b == a && (unsigned)ib < (unsigned)ia);
          const bool a_first = a > b || (a == b && (unsigned)ia < (unsigned)ib);
          if (desc ? b_first : a_first) {
            cval[i] = b;
            cval[ixj] = a;
            const int t = cidx[i];
            cidx[i] = cidx[ixj];
            cidx[ixj] = t;
          }
        }
      }
      __syncthreads();
    }
  }
  return n;
}

// per-row penalty inputs of the penalised sampler (rows: index into the state table, -1 = the row has none)
struct PenArgs {
  int* state;       // [n_rows, V] int32, or null
  int n_rows;
  const int* rows;
  const float *rep, *freq, *pres, *minp;
};

// per-row constraint inputs of the constrained sampler
struct ConArgs {
  const int* pool;   // constraint programs, back to back
  long pool_words;
  int* cstate;       // [n_slots] automaton state words
  int n_slots;
  const int* prog;   // per row: word offset of its program in the pool, -1 = unconstrained
  const int* slot;   // per row: its state word
  const int* ban;    // per row: != 0 bans the program's stop mask this step
};

// the sampler body; CON implies PEN
template <bool BF16, bool PEN, bool CON>
__device__ __forceinline__ void sample_body(const void* __restrict__ logits, long ld, int V,
                                            const float* __restrict__ temps, const int* __restrict__ topk,
                                            const float* __restrict__ topp, const float* __restrict__ uniforms,
                                            int* __restrict__ out, const PenArgs& pa, const ConArgs& ca) {
  __shared__ float cval[SMP_MAXK];
  __shared__ int cidx[SMP_MAXK];
  __shared__ float scan[SMP_MAXK];
  const int row = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const char* base = reinterpret_cast<const char*>(logits) + (long)row * ld * (BF16 ? 2 : 4);
  const float T = temps[row];
  int K = topk[row];
  if (T <= 0.f) K = 1;
  if (K <= 0 || K > V) K = V;
  K = min(K, SMP_MAXK);

  int* st = nullptr;  // this row's state words
  float minp = 0.f;
  int n;
  [[maybe_unused]] ConProg cp{};          // this row's constraint program, its automaton state and state word
  [[maybe_unused]] int cst = 0;
  [[maybe_unused]] int* cslot = nullptr;
  // the pick's bookkeeping (thread 0): count the token in the penalty state, advance the automaton
  auto picked = [&](int tok) {
    if constexpr (PEN) {
      SHAI_DASSERT(tok >= 0 && tok < V);
      if (st && tok >= 0 && tok < V) atomicAdd(&st[tok], 1);
    }
    if constexpr (CON) {
      if (cslot) {
        int lo = cp.estart[cst], hi = cp.estart[cst + 1];
        SHAI_DASSERT(lo >= 0 && lo <= hi && hi <= cp.E);
        lo = max(lo, 0), hi = min(hi, cp.E);
        const int end = hi;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (cp.etok[mid] < tok) lo = mid + 1;
          else hi = mid;
        }
        int nx = lo < end && cp.etok[lo] == tok ? cp.enext[lo] : cp.dflt[cst];
        SHAI_DASSERT(nx >= 0 && nx < cp.S);
        if (nx < 0 || nx >= cp.S) nx = cst;
        *cslot = nx;
      }
    }
  };
  if constexpr (PEN) {
    const int srow = pa.rows[row];
    SHAI_DASSERT(srow < pa.n_rows);
    if (pa.state && srow >= 0 && srow < pa.n_rows) st = pa.state + (long)srow * V;
    minp = pa.minp[row];
    const PenLoad<BF16> load{base, st, pa.rep[row], pa.freq[row], pa.pres[row]};
    if constexpr (CON) {
      __shared__ int s_bid[CON_MAX_BIAS];
      __shared__ float s_bval[CON_MAX_BIAS];
      const long off = ca.prog[row];
      const int sl = ca.slot[row];
      if (off >= 0) {
        SHAI_DASSERT(sl >= 0 && sl < ca.n_slots);
        if (ca.cstate && sl >= 0 && sl < ca.n_slots) {
          cp = con_resolve(ca.pool, ca.pool_words, off, V);
          cst = ca.cstate[sl];
          SHAI_DASSERT(!cp.ok || (cst >= 0 && cst < cp.S));
          if (cp.ok && (cst < 0 || cst >= cp.S)) cp.ok = false;
          if (cp.ok) cslot = ca.cstate + sl;
        }
      }
      if (cp.ok) {
        for (int i = tid; i < cp.NB; i += SMP_T) {
          s_bid[i] = cp.bid[i];
          s_bval[i] = __int_as_float(cp.bval[i]);
        }
        __syncthreads();
      }
      const ConLoad<BF16> cload{load, cp.ok ? cp.masks + (long)cst * cp.W : nullptr,
                                cp.ok && ca.ban[row] != 0 ? cp.stop : nullptr, cp.ok && cp.NB > 0 ? cp.plane : nullptr,
                                s_bid, s_bval, cp.NB};
      n = smp_topk<false>(cload, V, K, cval, cidx);
    } else {
      n = smp_topk<false>(load, V, K, cval, cidx);
    }
  } else {
    const RawLoad<BF16> load{base};
    n = smp_topk<BF16>(load, V, K, cval, cidx);
  }
  if (T <= 0.f || n == 1) {
    if (tid == 0) {
      const int tok = cidx[0];
      out[row] = tok;
      picked(tok);
    }
    return;
  }
  // ---- 4. probabilities, (min_p cut,) inclusive scan, nucleus cut, draw
  const float inv_t = 1.f / T, l0 = cval[0];
  float p = tid < n ? __expf((cval[tid] - l0) * inv_t) : 0.f;
  if constexpr (PEN) {
    // min_p: candidates with p_i < min_p go (p_0 = 1 stays); p falls along the sorted candidates, so they are a
    // suffix and the survivors are the first n2
    __shared__ int s_n2;
    if (tid == 0) s_n2 = 0;
    __syncthreads();
    // (constrained: candidates at -inf go too -- masked tokens, a suffix as well; candidate 0 is finite)
    bool fin = true;
    if constexpr (CON) fin = tid < n && cval[tid] > -INFINITY;
    const bool stay = tid < n && (tid == 0 || (!(p < minp) && fin));
    if (stay) atomicAdd(&s_n2, 1);
    else p = 0.f;
    __syncthreads();
    n = max(1, min(n, s_n2));
    if (tid >= n) p = 0.f;
  }
  // block inclusive scan (wave scan + wave totals)
  float x = p;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __shared__ float wsum[SMP_WAVES];
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  if (tid < 64) {
    float s = tid < SMP_WAVES ? wsum[tid] : 0.f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float y = __shfl_up(s, o, 64);
      if (lane >= o) s += y;
    }
    if (tid < SMP_WAVES) wsum[tid] = s;
  }
  __syncthreads();
  const float incl = x + (w > 0 ? wsum[w - 1] : 0.f);
  if (tid < SMP_MAXK) scan[tid] = incl;
  __syncthreads();
  const float total = scan[n - 1];
  const float cut = topp[row] * total;
  // kept prefix length L: number of i with (mass before i) <= cut  (always >= 1)
  __shared__ int s_L;
  if (tid == 0) s_L = 0;
  __syncthreads();
  if (tid < n && incl - p <= cut) atomicAdd(&s_L, 1);
  __syncthreads();
  const int L = max(1, s_L);
  const float target = uniforms[row] * scan[L - 1];
  __shared__ int s_pick;
  if (tid == 0) s_pick = 0;
  __syncthreads();
  if (tid < L - 1 && scan[tid] <= target) atomicAdd(&s_pick, 1);
  __syncthreads();
  if (tid == 0) {
    const int tok = cidx[min(s_pick, L - 1)];
    out[row] = tok;
    picked(tok);
  }
}

template <bool BF16, bool PEN>
__global__ void __launch_bounds__(SMP_T) sample_kernel(const void* __restrict__ logits, long ld, int V,
                                                       const float* __restrict__ temps, const int* __restrict__ topk,
                                                       const float* __restrict__ topp,
                                                       const float* __restrict__ uniforms, int* __restrict__ out,
                                                       PenArgs pa) {
  sample_body<BF16, PEN, false>(logits, ld, V, temps, topk, topp, uniforms, out, pa, ConArgs{});
}

template <bool BF16>
__global__ void __launch_bounds__(SMP_T) sample_con_kernel(const void* __restrict__ logits, long ld, int V,
                                                           const float* __restrict__ temps,
                                                           const int* __restrict__ topk,
                                                           const float* __restrict__ topp,
                                                           const float* __restrict__ uniforms, int* __restrict__ out,
                                                           PenArgs pa, ConArgs ca) {
  sample_body<BF16, true, true>(logits, ld, V, temps, topk, topp, uniforms, out, pa, ca);
}

void launch_sample(const void* logits, bool bf16, long ld, int B, int V, const float* temps, const int* top_k,
                   const float* top_p, const float* uniforms, int* out, hipStream_t s) {
  const PenArgs none{};
  if (bf16) sample_kernel<true, false><<<B, SMP_T, 0, s>>>(logits, ld, V, temps, top_k, top_p, uniforms, out, none);
  else sample_kernel<false, false><<<B, SMP_T, 0, s>>>(logits, ld, V, temps, top_k, top_p, uniforms, out, none);
}

void launch_sample_penalized(const void* logits, bool bf16, long ld, int B, int V, const float* temps,
                             const int* top_k, const float* top_p, const float* uniforms, int* out, int* state,
                             int n_state_rows, const int* state_rows, const float* rep, const float* freq,
                             const float* pres, const float* min_p, hipStream_t s) {
  const PenArgs pa{state, n_state_rows, state_rows, rep, freq, pres, min_p};
  if (bf16) sample_kernel<true, true><<<B, SMP_T, 0, s>>>(logits, ld, V, temps, top_k, top_p, uniforms, out, pa);
  else sample_kernel<false, true><<<B, SMP_T, 0, s>>>(logits, ld, V, temps, top_k, top_p, uniforms, out, pa);
}

void launch_sample_constrained(const void* logits, bool bf16, long ld, int B, int V, const float* temps,
                               const int* top_k, const float* top_p, const float* uniforms, int* out, int* state,
                               int n_state_rows, const int* state_rows, const float* rep, const float* freq,
                               const float* pres, const float* min_p, const int* pool, long pool_words, int* cstate,
                               int n_slots, const int* prog, const int* slot, const int* ban, hipStream_t s) {
  const PenArgs pa{state, n_state_rows, state_rows, rep, freq, pres, min_p};
  const ConArgs ca{pool, pool_words, cstate, n_slots, prog, slot, ban};
  if (bf16) sample_con_kernel<true><<<B, SMP_T, 0, s>>>(logits, ld, V, temps, top_k, top_p, uniforms, out, pa, ca);
  else sample_con_kernel<false><<<B, SMP_T, 0, s>>>(logits, ld, V, temps, top_k, top_p, uniforms, out, pa, ca);
}

// ---- constraint state: (re)initialise one sequence's automaton state word (stream-ordered: it lands after every
// launch enqueued before it, a look-ahead step of the slot's previous owner included)
__global__ void constraint_state_init_kernel(int* __restrict__ cstate, int n_slots, int slot, int value) {
  SHAI_DASSERT(slot >= 0 && slot < n_slots);
  if (threadIdx.x == 0 && blockIdx.x == 0 && slot >= 0 && slot < n_slots) cstate[slot] = value;
}

void launch_constraint_state_init(int* cstate, int n_slots, int slot, int value, hipStream_t s) {
  constraint_state_init_kernel<<<1, 64, 0, s>>>(cstate, n_slots, slot, value);
}

// ---- penalty state: (re)initialise one row.  Workgroup b owns PSI_SPAN consecutive words: it clears them, then
// walks the token list and applies the tokens that fall into its span (prompt tokens set the flag, the others
// count), so one launch needs no ordering between workgroups.  Ids outside [0, V) fall into no span.
constexpr int PSI_T = 256;
constexpr int PSI_SPAN = 4096;

__global__ void __launch_bounds__(PSI_T) penalty_state_init_kernel(int* __restrict__ st, int V,
                                                                   const int* __restrict__ tokens, int n_tokens,
                                                                   int n_prompt) {
  const int lo = blockIdx.x * PSI_SPAN, hi = min(V, lo + PSI_SPAN);
  for (int i = lo + threadIdx.x; i < hi; i += PSI_T) st[i] = 0;
  __syncthreads();
  for (int j = threadIdx.x; j < n_tokens; j += PSI_T) {
    const int t = tokens[j];
    if (t >= lo && t < hi) {
      SHAI_DASSERT(t >= 0 && t < V);
      if (j < n_prompt) atomicOr(&st[t], PEN_PROMPT);
      else atomicAdd(&st[t], 1);
    }
  }
}

void launch_penalty_state_init(int* state_row, int V, const int* tokens, int n_tokens, int n_prompt, hipStream_t s) {
  penalty_state_init_kernel<<<(V + PSI_SPAN - 1) / PSI_SPAN, PSI_T, 0, s>>>(state_row, V, tokens, n_tokens, n_prompt);
}

// ---- log-probabilities of the raw logits, one workgroup per row: vals / ids [B, 1 + N]; entry 0 is the picked
// token (toks[row]), entries 1..N the N most likely tokens (descending value, ascending index).  row_n (optional):
// how many of the N this row wants; a negative value skips the row, the entries past it read -inf / -1.
// max and sum exp(l - max) in a fixed order (per-thread partial over i = tid, tid + 1024, ...; wave butterfly; the
// 16 wave results in sequence), so the result does not vary between runs.
template <bool BF16>
__global__ void __launch_bounds__(SMP_T) token_logprobs_kernel(const void* __restrict__ logits, long ld, int V,
                                                               const int* __restrict__ toks,
                                                               const int* __restrict__ row_n, int N,
                                                               float* __restrict__ vals, int* __restrict__ ids) {
  __shared__ float cval[SMP_MAXK];
  __shared__ int cidx[SMP_MAXK];
  __shared__ float red[SMP_WAVES];
  const int row = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  int want = row_n ? min(row_n[row], N) : N;
  if (want < 0) return;
  const RawLoad<BF16> load{reinterpret_cast<const char*>(logits) + (long)row * ld * (BF16 ? 2 : 4)};
  float m = -INFINITY;
  for (int i = tid; i < V; i += SMP_T) m = fmaxf(m, load(i));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) red[w] = m;
  __syncthreads();
  float mx = red[0];
#pragma unroll
  for (int q = 1; q < SMP_WAVES; ++q) mx = fmaxf(mx, red[q]);
  __syncthreads();
  float s = 0.f;
  for (int i = tid; i < V; i += SMP_T) s += __expf(load(i) - mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) red[w] = s;
  __syncthreads();
  float sum = red[0];
#pragma unroll
  for (int q = 1; q < SMP_WAVES; ++q) sum += red[q];
  const float lse = mx + logf(sum);
  const long o0 = (long)row * (1 + N);
  if (tid == 0) {
    const int tok = toks[row];
    SHAI_DASSERT(tok >= 0 && tok < V);
    vals[o0] = tok >= 0 && tok < V ? load(tok) - lse : -INFINITY;
    ids[o0] = tok;
  }
  int n = 0;
  if (want > 0) n = smp_topk<BF16>(load, V, min(want, V), cval, cidx);
  if (tid < N) {
    SHAI_DASSERT(n <= N);
    vals[o0 + 1 + tid] = tid < n ? cval[tid] - lse : -INFINITY;
    ids[o0 + 1 + tid] = tid < n ? cidx[tid] : -1;
  }
}

void launch_token_logprobs(const void* logits, bool bf16, long ld, int B, int V, const int* toks, const int* row_n,
                           int N, float* vals, int* ids, hipStream_t s) {
  if (bf16) token_logprobs_kernel<true><<<B, SMP_T, 0, s>>>(logits, ld, V, toks, row_n, N, vals, ids);
  else token_logprobs_kernel<false><<<B, SMP_T, 0, s>>>(logits, ld, V, toks, row_n, N, vals, ids);
}

}  // namespace shai

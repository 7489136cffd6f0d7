// The host side shared by the tile GEMMs over 4-bit weights (gemm_fp4.hip: MXFP4, gemm_nf4.hip: NF4; problems of more
// than 64 activation rows): both kernels step K by 128 and have the same two tiles, so the tile set, the tile and
// split heuristics, the common part of *_supported and the launch sequence are written once here.  A kernel file keeps
// its device code, its own *_supported terms, its workspace rule and its dispatch_epilogue instantiation list.
#pragma once
#include "skinny_common.h"

namespace shai {

constexpr int Q4T_BK = 128;  // K per step of both kernels

inline int q4t_ksteps(const GemmArgs& a) { return (a.K + Q4T_BK - 1) / Q4T_BK; }

// tile 0 = 128 x 128, 1 = 256 x 128 (kQ4Tiles of them)
inline void q4t_tile_dims(int tile, int* bm, int* bn) {
  *bm = tile == 1 ? 256 : 128;
  *bn = 128;
}

// heuristic tile: the 256-row tile once it alone gives every CU a workgroup
inline int q4t_tile(const GemmArgs& a) { return (long)((a.M + 255) / 256) * ((a.N + 127) / 128) >= 256 ? 1 : 0; }

// heuristic split count: up to one workgroup per CU (one fits), each split at least 4 K steps
inline int q4t_splits(const GemmArgs& a, int tile) {
  int bm, bn;
  q4t_tile_dims(tile, &bm, &bn);
  const long tiles = (long)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn);
  const int ksteps = q4t_ksteps(a);
  int s = 1;
  while (s < 16 && tiles * s * 2 <= 256 && ksteps / (s * 2) >= 4) s *= 2;
  return s;
}

inline int q4t_max_splits(const GemmArgs& a) { return max_kgroups(q4t_ksteps(a)); }

// what a tile kernel asks beside q4_weights_supported (skinny_common.h) and its own terms
inline bool q4t_supported(const GemmArgs& a, int kmult, int sb) {
  return q4_weights_supported(a, kmult, sb) && a.M > 64 && tile_act_supported(a) && a.A2 == nullptr;
}

// splits K groups (needs ws of the kernel's workspace rule, else unsplit) folded by launch_splitk_epilogue in split
// order; launch_tile(tile, kg, kg_steps) launches the kernel of that tile
template <class F>
inline void q4t_launch(const GemmArgs& a, float* ws, int tile, int splits, hipStream_t s, F&& launch_tile) {
  const KSplit ks = split_ksteps(q4t_ksteps(a), ws != nullptr ? splits : 1);
  launch_tile(tile, ks.kg, ks.kg_steps);
  if (ks.kg > 1) launch_splitk_epilogue(a, ws, ks.kg, s);
}

}  // namespace shai

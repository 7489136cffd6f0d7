// Helpers shared by the paged decode attention kernels (attention.hip: bf16 cache, attention_kv8.hip: fp8 cache)
// and the split combine that serves both.
#pragma once
#include "common.h"

namespace shai {

// Split count of one sequence of nblk 64-token blocks when the launch has num_splits: at least kDaMinSplitBlocks
// blocks per split, so that a batch whose factor was raised for one long context (up to 64 splits at 128k) does
// not give every short sequence 64 mostly-empty workgroups and a 64-way combine.
constexpr int kDaMinSplitBlocks = 4;
__device__ __forceinline__ int da_splits(int nblk, int num_splits) {
  return max(1, min(num_splits, (nblk + kDaMinSplitBlocks - 1) / kDaMinSplitBlocks));
}

}  // namespace shai

// Host-side helpers of the entry points (no device code): the launch status, the one
// pointer-alignment predicate and the block-count rule of the strided grids.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "veon_hip.h"

namespace {

inline int launch_status() {
  return hipGetLastError() == hipSuccess ? VEON_OK : VEON_ERR_LAUNCH;
}

// p is a multiple of `bytes` (a power of two)
inline bool aligned(const void* p, uintptr_t bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// Blocks of a grid whose workgroups stride over `tiles` (> 0) units of work: the fewest
// rounds that keep the grid <= max_blocks, then even shares per round.
inline int even_share_blocks(int64_t tiles, int max_blocks) {
  const int64_t rounds = (tiles + max_blocks - 1) / max_blocks;
  return (int)((tiles + rounds - 1) / rounds);
}

}  // namespace

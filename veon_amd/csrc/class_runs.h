// Runs of classifier rows merged by their maximum (SANInVeonTemporal._merge_classes_prob,
// san_in_veon_entry_temporal.py:273-297): the group table of a detailed vocabulary and the
// running arg-max over its merged channels, one definition each, shared by the grouped
// occupancy tails (occ_tail.hip) and the 2-D label tail (sem2d.hip) -- the two arg-max the
// same way on their sums, so they can never disagree on a rule.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int MAX_ROWS = 256;     // logit rows
constexpr int MAX_MERGED = 64;    // merged channels
constexpr unsigned RUN_ENDS = 0x80u;

// entry c: the merged channel of row c, | RUN_ENDS on the last row of its run; zero past K.
// It travels in the kernel arguments (256 bytes) and is copied to LDS once per block.
struct GroupTable {
  uint8_t e[MAX_ROWS];
};

// group (HOST, K bytes) -> the kernels' table; false unless every row's channel is below
// n_merged, the rows of a channel are consecutive and every channel has exactly one run
inline bool make_table(const uint8_t* group, int K, int n_merged, GroupTable* table) {
  bool used[MAX_MERGED] = {};
  int runs = 0;
  for (int c = 0; c < MAX_ROWS; ++c) table->e[c] = 0;
  for (int c = 0; c < K; ++c) {
    if (group[c] >= n_merged) return false;
    const bool ends = c + 1 == K || group[c + 1] != group[c];
    table->e[c] = (uint8_t)(group[c] | (ends ? RUN_ENDS : 0u));
    if (ends) {
      if (used[group[c]]) return false;
      used[group[c]] = true;
      ++runs;
    }
  }
  return runs == n_merged;
}

// The running arg-max: rows arrive in order, a run of rows is merged by its maximum (NaN
// sticks), the lowest merged channel that attains the maximum wins.  `row` returns the
// maximum of the run so far: with `ends`, the merged value of channel `chan`.
struct RunArgMax {
  float vmax = -INFINITY, run = -INFINITY;
  int cls = MAX_ROWS;
  int bad = 0;   // (an int, not a bool: see PlainRows in occ_tail.hip)
  __device__ __forceinline__ float row(int chan, bool ends, float val) {
    bad |= val != val;
    run = run != run ? run : ((val != val || val > run) ? val : run);
    const float merged = run;
    if (ends) {
      if (run > vmax || (run == vmax && chan < cls)) {
        vmax = run;
        cls = chan;
      }
      run = -INFINITY;
    }
    return merged;
  }
};

}  // namespace

// Runs of equal values among the 64 lanes of a wavefront (rg_components.hip: the cell table; rg_tracking.hip: label overlap).
// A kernel with one thread per pixel sees the pixels of a cell as runs of consecutive lanes; it combines each run with a
// segmented shuffle scan -- a lane only ever takes from lanes at or after `start` -- and lets the run's last lane issue the
// atomics.  Every lane of the wavefront must call these (ballot and shuffle).
#pragma once

#include "rg_common.hpp"

namespace rg {

// heads: bit l set where lane l begins a run (bit 0 always).  start = first lane of my run, tail = I am its last lane
__device__ __forceinline__ void run_from_heads(unsigned long long heads, int lane, int* start, bool* tail) {
  *start = 63 - __builtin_clzll(heads & ((2ull << lane) - 1ull));
  *tail = lane == kWave - 1 || ((heads >> (lane + 1)) & 1ull);
}

// runs of equal `cell`
__device__ __forceinline__ void run_of(int cell, int lane, int* start, bool* tail) {
  const int prev = __shfl_up(cell, 1);
  run_from_heads(__ballot(lane == 0 || prev != cell), lane, start, tail);
}

// runs of equal pairs (a, b)
__device__ __forceinline__ void run_of_pair(int a, int b, int lane, int* start, bool* tail) {
  const int prev_a = __shfl_up(a, 1), prev_b = __shfl_up(b, 1);
  run_from_heads(__ballot(lane == 0 || prev_a != a || prev_b != b), lane, start, tail);
}

}  // namespace rg

// The row convention of the row-batched entries (l2s_*_rows, l2s_masks_to_map): row r of a call is used iff row0 + r < *count (count: a device
// int32, null = all rows).  A dead row is neither read nor written, and no grid depends on *count.
#pragma once
#include "common.h"

__device__ __forceinline__ bool row_live(int r, int row0, const int* count) { return !count || row0 + r < *count; }
// how many of a call's `rows` rows are live: they are the first ones
__device__ __forceinline__ int live_rows(int rows, int row0, const int* count) {
  if (!count) return rows;
  const int n = *count - row0;
  return n < 0 ? 0 : (n > rows ? rows : n);
}

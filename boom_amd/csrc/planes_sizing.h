// How the column service sizes its split-K planes (engine_glm.hip, column_buffers).  No HIP
// dependency: tests/cpp/planes_sizing_check.cpp compiles this header on its own.
//
// The workspace has two users.  launch_xtwx_cols writes planes(n) * R * p doubles for a launch
// of R requests; build_columns cuts the request list into launches of at most
// column_request_batch requests.  launch_rows_times_columns (X'Wz and the diagonal of every
// chain, once per sweep) writes planes(n) * chains * p doubles in ONE launch, whatever the
// batch is.  The capacity covers both.
#ifndef BOOM_AMD_PLANES_SIZING_H
#define BOOM_AMD_PLANES_SIZING_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace boom_amd {

constexpr int64_t COLS_PLANE_ROWS = 2048;   // rows per plane of xtwx_cols_kernel (its KCHUNK)

inline size_t cols_planes(int64_t n) { return (size_t)((n + COLS_PLANE_ROWS - 1) / COLS_PLANE_ROWS); }

// requests per launch_xtwx_cols launch: the planes of one launch at most 1 GiB, at least one
// request tile; never more than 32768 (the reduce kernel's grid has one row per request) nor
// than there are vectors
inline int64_t column_request_batch(size_t chains, int64_t n, size_t p) {
  const size_t per_req = cols_planes(n) * p * 8;
  const size_t batch = std::min<size_t>(std::max<size_t>(((size_t)1 << 30) / per_req, 64), 32768);
  return (int64_t)std::min<size_t>(batch, chains * p);
}

// doubles of the planes workspace: the larger of its two users.  (The 1 GiB above bounds what
// the engine can choose, the batch; the rows product needs a plane set per chain in any case,
// as the probit path's own allocation does.)
inline size_t column_planes_doubles(size_t chains, int64_t n, size_t p) {
  const size_t rows = std::max<size_t>((size_t)column_request_batch(chains, n, p), chains);
  return rows * cols_planes(n) * p;
}

}  // namespace boom_amd
#endif

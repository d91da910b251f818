// Regime geometry of the weighted aggregates (aggregate_fold.h, aggregate_qffl.hip): host arithmetic
// only, no device code -- plain C++, so a host program can include it on its own.  Every rule folds
// M rows in the same regime, sub-ranges, chunks and stage-2 tree at the same M, which is what makes
// fs_aggregate_sel bitwise fs_aggregate, the update rules' delta bitwise FedNova's mode 2, and so on.
#pragma once

#include <algorithm>
#include <cstdint>

namespace fs {

constexpr int AG_ONE_MAX_N = 512;   // clients up to which chunks <= 0 is the one-launch form
constexpr int AG_FP_SUB = 8;        // threads per float4 position of the stage-2 tree

// sub-ranges per float4 position of the one-launch form: 1 below 16 clients (then the fold is the
// reference's, bitwise), else the largest power of two <= min(32, N / 6) (~6+ clients per thread:
// one or two round trips of 8 loads)
inline int one_launch_sub(int N) {
  if (N < 16) return 1;
  int s = 1;
  while (s * 2 <= 32 && s * 2 <= N / 6) s *= 2;
  return s;
}

// the chunk rule of the two-stage form: how many consecutive client ranges (and clients per
// range) N clients are folded in (chunks <= 0: by the shape)
inline int aggregate_chunks(int N, int chunks, bool has_ws, int64_t ws_floats, int64_t len, int* per_out) {
  if (chunks <= 0) {
    // 8 chunks (>= 8 clients each): at N = 1000-1250 every count from 8 to 16 measured within
    // 5 % of the best and the earlier "~2048 workgroups" rule (74-103 chunks) 10-20 % slower
    // (profiles/r05/agg_time.txt)
    chunks = (int)std::max<int64_t>(1, std::min<int64_t>(8, N / 8));
  }
  if (chunks > N) chunks = N;
  // as many chunks as the workspace holds partials for (without one: a single chunk); an
  // automatic count above that used to fall back to ONE chunk -- 8 % of HBM at config 4
  // (1250 clients, 80 KB each, 5,120 threads walking all of them: 161 us per round)
  if (chunks > 1) chunks = has_ws ? (int)std::min<int64_t>(chunks, ws_floats / len) : 1;
  if (chunks < 1) chunks = 1;
  const int per = (N + chunks - 1) / chunks;
  *per_out = per;
  return (N + per - 1) / per;
}

}  // namespace fs

// MSE evaluation of one 16-row group -- the row body of fs_eval_mse's workgroups (eval_mse.hip)
// and of fs_eval_clients_mse's (eval_clients.hip): both run exactly this code, so a group's two
// partial sums are the same bits either way.  One wave per row at a time: 16-byte loads, a wave
// reads contiguous bytes of the row, w from L2; squared residuals and the reference's degenerate
// "correct" count (y == 0, tools.py:88-90) in fp64, folded over the waves in wave order.
#pragma once

#include "common.h"

namespace fs {

// rows [r0, min(r0 + 16, n)) of (phi, y) against the one-column model W; s: 2 * NWV doubles of
// LDS; thread 0 writes the group's (sum of squares, zero-target count) to part2[0..1]
template <int NWV>
__device__ __forceinline__ void eval_mse_group16(const float* __restrict__ phi, int64_t ld,
                                                 const float* __restrict__ y, int n, const float* __restrict__ W,
                                                 int r0, double (*s)[NWV], double* __restrict__ part2) {
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  double sq = 0.0, zc = 0.0;
  for (int r = w; r < 16; r += NWV) {
    const int row = r0 + r;
    if (row >= n) break;
    const float* xp = phi + (int64_t)row * ld;
    float a = 0.f;
    for (int64_t c = 4 * lane; c < ld; c += 256) {
      const float4 xv = ld4(xp + c);
      const float4 wv = ld4(W + c);
      a = fmaf(xv.x, wv.x, a);
      a = fmaf(xv.y, wv.y, a);
      a = fmaf(xv.z, wv.z, a);
      a = fmaf(xv.w, wv.w, a);
    }
    a = wave_sum(a);
    const float t = y[row];
    const float res = a - t;
    sq += (double)res * (double)res;
    zc += (t == 0.0f) ? 1.0 : 0.0;   // top-1 of one column is index 0 (tools.py:88-90)
  }
  if (lane == 0) {
    s[0][w] = sq;
    s[1][w] = zc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < NWV; ++i) {
      a += s[0][i];
      b += s[1][i];
    }
    part2[0] = a;
    part2[1] = b;
  }
}

}  // namespace fs

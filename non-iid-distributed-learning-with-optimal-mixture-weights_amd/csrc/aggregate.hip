// fs_aggregate -- mixture-weighted model aggregation over the clients x params buffer.
//
// Replaces the inline fold of /root/reference/functions/tools.py:345-350 (also 372-377,
// 455-460):   global = p0*W0;  global = global + p_j*W_j  for j = 1..N-1,
// every product and every sum rounded separately (no fma contraction), so with one
// chunk the result is bitwise the reference's fold of the same W_j.
//
// The plain rule of aggregate_fold.h, whose kernels, regimes and dispatch these are: the term is
// p_j * W_j, nothing is read per position, the total is stored.
#include "aggregate_fold.h"
#include "aggregate_sel.h"

namespace fs {

#pragma clang fp contract(off)

struct PlainRule {
  using Finish = StoreFinish;
  Finish f;
  const float* p;   // [N]

  // two-stage form: the range's first row, then groups of 4 loads ahead of their folds, then the
  // tail one by one; one-launch form: fold_range_cond's groups of 8
  __device__ __forceinline__ Acc<1> fold(const float* __restrict__ base, int64_t stride, const Finish::Ctx&, int j0,
                                         int j1, bool one) const {
    if (one) return {{fold_range_cond<false>(base, stride, nullptr, p, j0, j1)}};
    float4 acc = scaled4(p[j0], ld4(base + (int64_t)j0 * stride));
    int j = j0 + 1;
    for (; j + 3 < j1; j += 4) {
      const float4 a = ld4(base + (int64_t)j * stride);
      const float4 b = ld4(base + (int64_t)(j + 1) * stride);
      const float4 c = ld4(base + (int64_t)(j + 2) * stride);
      const float4 d = ld4(base + (int64_t)(j + 3) * stride);
      acc = add4(acc, scaled4(p[j], a));
      acc = add4(acc, scaled4(p[j + 1], b));
      acc = add4(acc, scaled4(p[j + 2], c));
      acc = add4(acc, scaled4(p[j + 3], d));
    }
    for (; j < j1; ++j) acc = add4(acc, scaled4(p[j], ld4(base + (int64_t)j * stride)));
    return {{acc}};
  }
};

void fold_partials_launch(const float* d_part, int K, int64_t len4, float* d_out, hipStream_t st) {
  hipLaunchKernelGGL(fold_partials_kernel<StoreFinish>, dim3((unsigned)((len4 + AG_FP_POS - 1) / AG_FP_POS)), dim3(256),
                     0, st, d_part, K, len4, StoreFinish{d_out});
}

int aggregate_launch(const float* d_W_all, int64_t stride, const float* d_p, int N, int64_t len, float* d_W_bar,
                     float* d_ws, int64_t ws_floats, int chunks, const EvalFinalize* fin, hipStream_t st) {
  FS_REQUIRE(N >= 1, "N must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_p && d_W_bar, "null pointer");
  return fold_dispatch(d_W_all, stride, PlainRule{{d_W_bar}, d_p}, N, len, d_ws, ws_floats, chunks, fin, st);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate(const float* d_W_all, int64_t stride, const float* d_p, int N, int64_t len,
                            float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks, void* stream) {
  return aggregate_launch(d_W_all, stride, d_p, N, len, d_W_bar, d_ws, ws_floats, chunks, nullptr,
                          reinterpret_cast<hipStream_t>(stream));
}

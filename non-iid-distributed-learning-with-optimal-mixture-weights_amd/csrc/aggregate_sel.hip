// fs_aggregate_sel -- the gathered fold: W_bar = q_0 * W[sel_0] + q_1 * W[sel_1] + ... over M
// sampled rows of the clients x params buffer, in k order, every product and every sum rounded
// separately (a round with partial client participation: the tools.py:345-350 left fold over
// the sampled clients in ascending client id).
//
// Contract: bitwise what fs_aggregate (aggregate.hip) returns on the compacted copy W[sel] with
// the same `chunks` -- the same two regimes chosen by M (aggregate_sel.h's rules), the same
// sub-ranges, chunks and stage-2 tree, so for M < 16 the reference's exact left fold.
//
// HBM-bound: M * len floats read plus the output written; rows outside sel are never touched
// (fs_aggregate with zero weights on them would read N * len and multiply stale rows by 0).
// Each thread owns one float4 of the len parameters and walks its range of k; consecutive threads
// read consecutive 16 B of row sel[k], so every sampled row is one coalesced sweep wherever it
// lies.  The row index sel[k] and the weight q[k] depend on k alone: in the chunked form k is
// uniform over the workgroup (scalar loads), in the one-launch form uniform over each sub-range's
// threads (a broadcast load of one address).  No atomics, no cross-workgroup wait.
#include "aggregate_sel.h"
#include "common.h"
#include "finalize.h"

namespace fs {

// No fma contraction anywhere in this file (as aggregate.hip): q * W and the sum round separately.
#pragma clang fp contract(off)

__device__ __forceinline__ float4 sel_fold_step(float4 acc, float p, float4 w) {
  return make_float4(acc.x + p * w.x, acc.y + p * w.y, acc.z + p * w.z, acc.w + p * w.w);
}

// the left fold of k = k0 .. k1-1 at one float4 position: the loads of 8 rows (and their indices
// and weights) issued before the first fold of the group, one round trip per 8 rows
__device__ __forceinline__ float4 sel_fold_range(const float* __restrict__ base, int64_t stride,
                                                 const int32_t* __restrict__ sel, const float* __restrict__ q, int k0,
                                                 int k1) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // a row's address waits for its index: the indices of the NEXT group of 8 are loaded behind
  // this group's row loads, so only the range's first group pays the extra round trip
  int idx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = (k0 + u < k1) ? sel[k0 + u] : 0;
  for (int k = k0; k < k1; k += 8) {
    const int n = min(8, k1 - k);
    float4 v[8];
    float pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (u < n) {
        v[u] = ld4(base + (int64_t)idx[u] * stride);
        pv[u] = q[k + u];
      }
#pragma unroll
    for (int u = 0; u < 8; ++u) idx[u] = (k + 8 + u < k1) ? sel[k + 8 + u] : 0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (u < n) {
        if (u == 0 && k == k0)
          acc = make_float4(pv[0] * v[0].x, pv[0] * v[0].y, pv[0] * v[0].z, pv[0] * v[0].w);
        else
          acc = sel_fold_step(acc, pv[u], v[u]);
      }
  }
  return acc;
}

// two-stage form, stage 1 (aggregate_kernel's geometry): chunk blockIdx.y folds k in
// [y * per, min(M, y * per + per)) into partial y (one chunk: straight into the output)
__global__ __launch_bounds__(256) void aggregate_sel_kernel(const float* __restrict__ W, int64_t stride,
                                                           const int32_t* __restrict__ sel,
                                                           const float* __restrict__ q, int M, int64_t len4,
                                                           int per_chunk, float* __restrict__ out,
                                                           int64_t out_stride) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len4) return;
  const int c = blockIdx.y;
  const int k0 = c * per_chunk;
  const int k1 = min(M, k0 + per_chunk);
  st4(out + (int64_t)c * out_stride + 4 * i, sel_fold_range(W + 4 * i, stride, sel, q, k0, k1));
}

// one-launch form (aggregate_one_kernel's geometry): SUB consecutive ranges of k per float4
// position folded by SUB threads of one workgroup, their partials folded in order in LDS; the
// deferred evaluation's finaliser rides as the last workgroup
template <int SUB>
__global__ __launch_bounds__(256) void aggregate_sel_one_kernel(const float* __restrict__ W, int64_t stride,
                                                               const int32_t* __restrict__ sel,
                                                               const float* __restrict__ q, int M, int64_t len4,
                                                               int per, float* __restrict__ out, EvalFinalize fin) {
  constexpr int POS = 256 / SUB;
  __shared__ float4 sums[SUB][POS];
  if (fin.part && blockIdx.x == gridDim.x - 1) {
    eval_finalize_block(fin.part, fin.nb, fin.n, fin.out, reinterpret_cast<double(*)[256]>(&sums[0][0]));
    return;
  }
  static_assert(sizeof(sums) >= 2 * 256 * sizeof(double), "the finaliser reuses the partials' LDS");
  const int sub = threadIdx.x / POS, pl = threadIdx.x % POS;
  const int64_t i = (int64_t)blockIdx.x * POS + pl;
  const int k0 = sub * per, k1 = min(M, k0 + per);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < len4 && k0 < k1) acc = sel_fold_range(W + 4 * i, stride, sel, q, k0, k1);
  sums[sub][pl] = acc;
  __syncthreads();
  if (sub == 0 && i < len4) {
    float4 t = sums[0][pl];
    for (int s2 = 1; s2 < SUB && s2 * per < M; ++s2) {
      const float4 v = sums[s2][pl];
      t = make_float4(t.x + v.x, t.y + v.y, t.z + v.z, t.w + v.w);
    }
    st4(out + 4 * i, t);
  }
}

template <int SUB>
static void launch_sel_one(const float* W, int64_t stride, const int32_t* sel, const float* q, int M, int64_t len4,
                           float* out, const EvalFinalize& fin, hipStream_t st) {
  constexpr int POS = 256 / SUB;
  const int per = (M + SUB - 1) / SUB;
  const int64_t blocks = (len4 + POS - 1) / POS + (fin.part ? 1 : 0);
  hipLaunchKernelGGL((aggregate_sel_one_kernel<SUB>), dim3((unsigned)blocks), dim3(256), 0, st, W, stride, sel, q, M,
                     len4, per, out, fin);
}

int aggregate_sel_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                         int64_t len, float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks,
                         const EvalFinalize* fin, hipStream_t st) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_sel && d_q && d_W_bar, "null pointer");
  const int64_t len4 = len / 4;
  const EvalFinalize none{nullptr, 0, 0, nullptr};
  if (chunks <= 0 && M <= AG_ONE_MAX_N) {
    const EvalFinalize& f = fin ? *fin : none;
    switch (one_launch_sub(M)) {
      case 1: launch_sel_one<1>(d_W_all, stride, d_sel, d_q, M, len4, d_W_bar, f, st); break;
      case 2: launch_sel_one<2>(d_W_all, stride, d_sel, d_q, M, len4, d_W_bar, f, st); break;
      case 4: launch_sel_one<4>(d_W_all, stride, d_sel, d_q, M, len4, d_W_bar, f, st); break;
      case 8: launch_sel_one<8>(d_W_all, stride, d_sel, d_q, M, len4, d_W_bar, f, st); break;
      case 16: launch_sel_one<16>(d_W_all, stride, d_sel, d_q, M, len4, d_W_bar, f, st); break;
      default: launch_sel_one<32>(d_W_all, stride, d_sel, d_q, M, len4, d_W_bar, f, st); break;
    }
    FS_LAUNCH_CHECK();
    return FS_OK;
  }
  if (fin) {
    const int rc = eval_finalize_launch(fin->part, fin->nb, fin->n, fin->out, st);
    if (rc != FS_OK) return rc;
  }
  const int64_t bx = (len4 + 255) / 256;
  int per = 0;
  chunks = aggregate_chunks(M, chunks, d_ws != nullptr, ws_floats, len, &per);
  if (chunks == 1) {
    hipLaunchKernelGGL(aggregate_sel_kernel, dim3((unsigned)bx, 1), dim3(256), 0, st, d_W_all, stride, d_sel, d_q, M,
                       len4, per, d_W_bar, (int64_t)0);
  } else {
    hipLaunchKernelGGL(aggregate_sel_kernel, dim3((unsigned)bx, chunks), dim3(256), 0, st, d_W_all, stride, d_sel, d_q,
                       M, len4, per, d_ws, len);
    fold_partials_launch(d_ws, chunks, len4, d_W_bar, st);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_sel(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                                int64_t len, float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks,
                                void* stream) {
  return aggregate_sel_launch(d_W_all, stride, d_sel, d_q, M, len, d_W_bar, d_ws, ws_floats, chunks, nullptr,
                              reinterpret_cast<hipStream_t>(stream));
}

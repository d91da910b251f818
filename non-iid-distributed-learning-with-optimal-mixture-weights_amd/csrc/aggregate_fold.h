// The fold skeleton of the weighted aggregates: fs_aggregate, _sel, _nova, _scaffold and _opt are
// one kernel family -- a sum over M rows of the clients x params buffer in k order, every operation
// rounded separately, the first term of any range of k the term itself (not 0 + term) -- and differ
// only in the term they form from a row, in what they read per position and in what they do with the
// folded total.  A rule R (by value: a kernel argument) is that difference:
//
//   R::fold(W + 4 i, stride, cx, k0, k1, one)   the left fold of the terms k0 .. k1-1 (k0 < k1) at one
//                                               float4 position, in the rule's own load schedule
//                                               (one: called from the one-launch form)
//   R::Finish f                                 what stage 2 needs as well:
//     SETS                accumulators, and partial sets, per position (Acc<SETS>)
//     RIDES               whether the deferred evaluation's finaliser may ride on the one-launch form
//     Ctx load(i, fin)    the position's context (the base / state the terms subtract); fin: this
//                         thread also finishes, so it loads what only the finish needs
//     finish(i, cx, t)    the stores, from the folded total
//
// Everything else stands here once: the three kernels, the regimes and their geometry
// (aggregate_geom.h), the finaliser handling, the launches.  So the rules' contracts -- sel bitwise
// plain, opt's and scaffold's delta bitwise FedNova's mode 2 -- hold by construction.
//
// Aliasing (rules that update in place): a position's context is read by the workgroup that writes
// that position, before it writes.  One-launch form: every sub-range's thread loads before the
// barrier, sub-range 0's thread finishes after it.  Two-stage form: stage 1 writes partials only,
// stage 2 loads and finishes in one thread; one chunk: one thread per position loads, folds, finishes.
#pragma once
#include "aggregate_geom.h"
#include "common.h"
#include "finalize.h"

namespace fs {

// No fma contraction in any fold (the pragma applies to the text below it, so a rule's file repeats
// it above its own arithmetic): every product, difference, quotient and sum rounds separately.  Plain
// operators under this pragma; HIP's __fmul_rn/__fadd_rn are header functions whose instructions
// keep the default contract flag and still fuse after inlining.
#pragma clang fp contract(off)

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}
__device__ __forceinline__ float4 scaled4(float s, float4 v) { return make_float4(s * v.x, s * v.y, s * v.z, s * v.w); }

// a position's accumulators
template <int SETS>
struct Acc {
  float4 a[SETS];
};

template <int SETS>
__device__ __forceinline__ Acc<SETS> zero_acc() {
  Acc<SETS> z;
#pragma unroll
  for (int s = 0; s < SETS; ++s) z.a[s] = zero4();
  return z;
}

// row of term k (SEL is a template parameter, not a test of the pointer: a run-time "load or not"
// select around each index makes hipcc branch around the loads and wait for them one by one)
template <bool SEL>
__device__ __forceinline__ int fold_row(const int32_t* __restrict__ sel, int k) { return SEL ? sel[k] : k; }

// ---- load schedule: conditional groups of 8 (fs_aggregate's one-launch form, fs_aggregate_sel) ----
// The left fold of q_k * W[row_k], k = k0 .. k1-1: every load of a group of 8 rows (the range's first
// included, and their weights) issued before the first fold of the group -- one round trip per 8 rows
// (the first row's load, then groups of 8 / 4, then the tail one by one took 4 dependent round trips
// at 7 rows per range).  SEL: a row's address waits for its index, so the indices of the NEXT group
// are loaded behind this group's row loads and only the range's first group pays the extra round trip.
template <bool SEL>
__device__ __forceinline__ float4 fold_range_cond(const float* __restrict__ base, int64_t stride,
                                                  const int32_t* __restrict__ sel, const float* __restrict__ q, int k0,
                                                  int k1) {
  float4 acc = zero4();
  int idx[8];
  if (SEL) {
#pragma unroll
    for (int u = 0; u < 8; ++u) idx[u] = (k0 + u < k1) ? sel[k0 + u] : 0;
  }
  for (int k = k0; k < k1; k += 8) {
    const int n = min(8, k1 - k);
    float4 v[8];
    float pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (u < n) {
        v[u] = ld4(base + (int64_t)(SEL ? idx[u] : k + u) * stride);
        pv[u] = q[k + u];
      }
    if (SEL) {
#pragma unroll
      for (int u = 0; u < 8; ++u) idx[u] = (k + 8 + u < k1) ? sel[k + 8 + u] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (u < n) {
        const float4 t = scaled4(pv[u], v[u]);
        if (u == 0 && k == k0)
          acc = t;
        else
          acc = add4(acc, t);
      }
  }
  return acc;
}

// ---- load schedule: clamped groups of 8 (fs_aggregate_nova, _opt, _scaffold) -------------------------
// Over a term T: T::NC per-k coefficient arrays coef[0..NC-1], T::SETS accumulators, and
// term(first_of_fold, cf, w) from the NC coefficients of a row and the row's float4.
//
// One group of up to 8 terms k .. k+7 (< k1) folded onto acc, fold_range_cond's schedule: the 8 row
// loads issued before the first fold, the indices of the next group behind them.  No load sits
// under a condition: with the loads under `if (u < n)` hipcc branched around each one and waited
// vmcnt(0) before the next -- eight dependent round trips per group, 2 - 2.5 x the time at
// N = 1000 - 1250.  FULL: all 8 terms exist, nothing is conditional.  Else (a range's short last
// group): the loads re-read the range's last row (k clamped to k1 - 1: a sampled row, a cache
// hit), only the folds are skipped, and the coefficients are pinned where they are loaded (the
// empty asm) so that they are not sunk into the skipped folds one scalar round trip each.
template <class T, bool SEL, bool FULL>
__device__ __forceinline__ Acc<T::SETS> fold_group(const float* __restrict__ W, int64_t stride, const int32_t* sel,
                                                   const T& t, Acc<T::SETS> acc, int (&idx)[8], int k, int k0, int k1) {
  const int last = k1 - 1;
  float4 v[8];
  float cf[8][T::NC];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int ku = FULL ? k + u : min(k + u, last);
    v[u] = ld4(W + (int64_t)idx[u] * stride);
#pragma unroll
    for (int c = 0; c < T::NC; ++c) cf[u][c] = t.coef[c][ku];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = fold_row<SEL>(sel, min(k + 8 + u, last));
  if (!FULL) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      static_assert(T::NC == 1 || T::NC == 2, "one asm statement pins all coefficients of a row");
      if constexpr (T::NC == 2)
        asm volatile("" : "+v"(cf[u][0]), "+v"(cf[u][1]));
      else
        asm volatile("" : "+v"(cf[u][0]));
    }
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (FULL || k + u < k1) {
      const Acc<T::SETS> x = t.term(u == 0 && k == 0, cf[u], v[u]);
      if (u == 0 && k == k0) {
#pragma unroll
        for (int s = 0; s < T::SETS; ++s) acc.a[s] = x.a[s];
      } else {
#pragma unroll
        for (int s = 0; s < T::SETS; ++s) acc.a[s] = add4(acc.a[s], x.a[s]);
      }
    }
  return acc;
}

// the left fold of the terms k = k0 .. k1-1 (k0 < k1) at one float4 position
template <bool SEL, class T>
__device__ __forceinline__ Acc<T::SETS> fold_range_clamped(const float* __restrict__ W, int64_t stride,
                                                           const int32_t* sel, const T& t, int k0, int k1) {
  Acc<T::SETS> acc = zero_acc<T::SETS>();
  int idx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = fold_row<SEL>(sel, min(k0 + u, k1 - 1));
  int k = k0;
  for (; k + 8 <= k1; k += 8) acc = fold_group<T, SEL, true>(W, stride, sel, t, acc, idx, k, k0, k1);
  if (k < k1) acc = fold_group<T, SEL, false>(W, stride, sel, t, acc, idx, k, k0, k1);
  return acc;
}

// the term of the rules that fold the clients' updates about the position's x (FedNova's update
// form and fs_aggregate_opt; SCAFFOLD's ScafTerm forms the same one for W_g): fl(q_k * fl(W[row_k] - x))
struct UpdateTerm {
  static constexpr int NC = 1, SETS = 1;
  const float* coef[1];   // q [M]
  float4 x;
  __device__ __forceinline__ Acc<1> term(bool, const float (&cf)[1], float4 w) const {
    return {{scaled4(cf[0], sub4(w, x))}};
  }
};

// ---- the finish of a plain sum (fs_aggregate, _sel, FedNova's reference form): store it ---------------
struct StoreFinish {
  static constexpr int SETS = 1;
  static constexpr bool RIDES = true;
  float* out;
  struct Ctx {};
  __device__ __forceinline__ Ctx load(int64_t, bool) const { return {}; }
  __device__ __forceinline__ void finish(int64_t i, const Ctx&, const Acc<1>& t) const { st4(out + 4 * i, t.a[0]); }
};

// ---- the kernels ------------------------------------------------------------------------------------------
// HBM-bound streaming reductions: each thread owns one float4 of the len parameters and walks its
// range of k; consecutive threads read consecutive 16 B, so every row is one coalesced sweep
// wherever it lies.  What depends on k alone (row index, coefficients) is uniform over the workgroup
// in the chunked form (scalar loads) and over each sub-range's threads in the one-launch form (a
// broadcast load of one address).  No atomics, no cross-workgroup wait.

// two-stage form, stage 1: chunk blockIdx.y folds k in [y * per, min(M, y * per + per)) into its
// SETS partials (set s of chunk y at part + (s * gridDim.y + y) * 4 len4).  When len4 / 256 workgroups
// cannot fill the chip the range of k is cut into such chunks, folded in parallel.  FINAL (one
// chunk): fold and finish in the one thread of the position.
template <class R, bool FINAL>
__global__ __launch_bounds__(256) void fold_chunk_kernel(const float* __restrict__ W, int64_t stride, R r, int M,
                                                        int64_t len4, int per_chunk, float* part) {
  using F = typename R::Finish;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len4) return;
  const int ch = blockIdx.y;
  const int k0 = ch * per_chunk;
  const int k1 = min(M, k0 + per_chunk);
  const typename F::Ctx cx = r.f.load(i, FINAL);
  const Acc<F::SETS> acc = r.fold(W + 4 * i, stride, cx, k0, k1, false);
  if (FINAL) {
    r.f.finish(i, cx, acc);
  } else {
#pragma unroll
    for (int s = 0; s < F::SETS; ++s) st4(part + ((int64_t)s * gridDim.y + ch) * 4 * len4 + 4 * i, acc.a[s]);
  }
}

// stage 2: AG_FP_SUB threads per float4 position, thread s folding the partials k = s, s + AG_FP_SUB,
// ... in order, then thread 0 of the position folding the AG_FP_SUB sums in order (a fixed tree:
// the same bits every run) and finishing.  One thread per position walking all K partials put only
// len4 / 256 workgroups on the chip (20 CUs, 20 us for 5 MB of partials).
constexpr int AG_FP_POS = 256 / AG_FP_SUB;

template <class F>
__global__ __launch_bounds__(256) void fold_partials_kernel(const float* __restrict__ part, int K, int64_t len4, F f) {
  constexpr int S = F::SETS;
  __shared__ float4 sums[S][AG_FP_SUB][AG_FP_POS];
  const int sub = threadIdx.x / AG_FP_POS, pl = threadIdx.x % AG_FP_POS;
  const int64_t i = (int64_t)blockIdx.x * AG_FP_POS + pl;
  Acc<S> acc = zero_acc<S>();
  typename F::Ctx cx{};
  if (i < len4 && sub < K) {
    if (sub == 0) cx = f.load(i, true);
#pragma unroll
    for (int s = 0; s < S; ++s) acc.a[s] = ld4(part + ((int64_t)s * K + sub) * 4 * len4 + 4 * i);
    for (int k = sub + AG_FP_SUB; k < K; k += AG_FP_SUB) {
#pragma unroll
      for (int s = 0; s < S; ++s) acc.a[s] = add4(acc.a[s], ld4(part + ((int64_t)s * K + k) * 4 * len4 + 4 * i));
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) sums[s][sub][pl] = acc.a[s];
  __syncthreads();
  if (sub == 0 && i < len4) {
    Acc<S> t;
#pragma unroll
    for (int s = 0; s < S; ++s) t.a[s] = sums[s][0][pl];
    for (int s2 = 1; s2 < AG_FP_SUB && s2 < K; ++s2) {
#pragma unroll
      for (int s = 0; s < S; ++s) t.a[s] = add4(t.a[s], sums[s][s2][pl]);
    }
    f.finish(i, cx, t);
  }
}

// One-launch form (chunks <= 0 with M <= AG_ONE_MAX_N): SUB consecutive ranges of k per float4
// position folded by SUB threads of one workgroup (stage 1, as fold_chunk_kernel's chunks), their
// partials folded in order in LDS (stage 2) and finished by the position's thread 0 -- one launch
// instead of two, no workspace.  The round plan also hands it the deferred evaluation's finaliser
// (one extra workgroup, eval.hip's eval_finalize arithmetic): the plain round went from four launches
// after the training (finalise, aggregate, fold, next training) to two.
// (AG_ONE_MAX_N = 512; above: 64 sub-ranges of 4 positions read 64-byte pieces of each client row --
// N = 1000-1250: 34-38 vs 18-19 us)
template <class R, int SUB>
__global__ __launch_bounds__(256) void fold_one_kernel(const float* __restrict__ W, int64_t stride, R r, int M,
                                                      int64_t len4, int per, EvalFinalize fin) {
  using F = typename R::Finish;
  constexpr int POS = 256 / SUB, S = F::SETS;
  __shared__ float4 sums[S][SUB][POS];
  if (F::RIDES) {
    if (fin.part && blockIdx.x == gridDim.x - 1) {
      eval_finalize_block(fin.part, fin.nb, fin.n, fin.out, reinterpret_cast<double(*)[256]>(&sums[0][0][0]));
      return;
    }
    static_assert(!F::RIDES || sizeof(sums) >= 2 * 256 * sizeof(double), "the finaliser reuses the partials' LDS");
  }
  const int sub = threadIdx.x / POS, pl = threadIdx.x % POS;
  const int64_t i = (int64_t)blockIdx.x * POS + pl;
  const int k0 = sub * per, k1 = min(M, k0 + per);
  Acc<S> acc = zero_acc<S>();
  typename F::Ctx cx{};
  if (i < len4 && k0 < k1) {
    cx = r.f.load(i, sub == 0);                       // (sub 0 always has a range: M >= 1)
    acc = r.fold(W + 4 * i, stride, cx, k0, k1, true);
  }
#pragma unroll
  for (int s = 0; s < S; ++s) sums[s][sub][pl] = acc.a[s];
  __syncthreads();
  if (sub == 0 && i < len4) {
    Acc<S> t;
#pragma unroll
    for (int s = 0; s < S; ++s) t.a[s] = sums[s][0][pl];
    for (int s2 = 1; s2 < SUB && s2 * per < M; ++s2) {
#pragma unroll
      for (int s = 0; s < S; ++s) t.a[s] = add4(t.a[s], sums[s][s2][pl]);
    }
    r.f.finish(i, cx, t);
  }
}

// ---- the dispatch -------------------------------------------------------------------------------------------
template <class R, int SUB>
void launch_fold_one(const float* W, int64_t stride, const R& r, int M, int64_t len4, const EvalFinalize& fin,
                     hipStream_t st) {
  constexpr int POS = 256 / SUB;
  const int per = (M + SUB - 1) / SUB;
  const int64_t blocks = (len4 + POS - 1) / POS + (fin.part ? 1 : 0);
  hipLaunchKernelGGL((fold_one_kernel<R, SUB>), dim3((unsigned)blocks), dim3(256), 0, st, W, stride, r, M, len4, per,
                     fin);
}

// The fold of M rows under rule r: one launch where chunks <= 0 and M <= AG_ONE_MAX_N (the finaliser
// as its last workgroup), else the two-stage form (the finaliser as a launch of its own before it),
// its chunks clamped to the partials d_ws holds (SETS per chunk).  fin: nullptr for none, and always
// for a rule whose Finish does not let it ride.
template <class R>
int fold_dispatch(const float* W, int64_t stride, const R& r, int M, int64_t len, float* d_ws, int64_t ws_floats,
                  int chunks, const EvalFinalize* fin, hipStream_t st) {
  using F = typename R::Finish;
  const int64_t len4 = len / 4;
  const EvalFinalize none{nullptr, 0, 0, nullptr};
  if (chunks <= 0 && M <= AG_ONE_MAX_N) {
    const EvalFinalize& f = fin && F::RIDES ? *fin : none;
    switch (one_launch_sub(M)) {
      case 1: launch_fold_one<R, 1>(W, stride, r, M, len4, f, st); break;
      case 2: launch_fold_one<R, 2>(W, stride, r, M, len4, f, st); break;
      case 4: launch_fold_one<R, 4>(W, stride, r, M, len4, f, st); break;
      case 8: launch_fold_one<R, 8>(W, stride, r, M, len4, f, st); break;
      case 16: launch_fold_one<R, 16>(W, stride, r, M, len4, f, st); break;
      default: launch_fold_one<R, 32>(W, stride, r, M, len4, f, st); break;
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
  chunks = aggregate_chunks(M, chunks, d_ws != nullptr, ws_floats / F::SETS, len, &per);
  if (chunks == 1) {
    hipLaunchKernelGGL((fold_chunk_kernel<R, true>), dim3((unsigned)bx, 1), dim3(256), 0, st, W, stride, r, M, len4, per,
                       (float*)nullptr);
  } else {
    hipLaunchKernelGGL((fold_chunk_kernel<R, false>), dim3((unsigned)bx, chunks), dim3(256), 0, st, W, stride, r, M, len4,
                       per, d_ws);
    hipLaunchKernelGGL(fold_partials_kernel<F>, dim3((unsigned)((len4 + AG_FP_POS - 1) / AG_FP_POS)), dim3(256), 0, st,
                       d_ws, chunks, len4, r.f);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace fs

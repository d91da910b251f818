// fs_aggregate_nova -- FedNova's scaled fold over M rows of the clients x params buffer, in k
// order, every operation rounded separately.  The one aggregation rule of the reference that is
// not a plain sum_k q_k W_k (tools.py:383-410), in two forms:
//
//   mode 1 (FS_NOVA_REFERENCE)  the reference's own lines (tools.py:401-405), which scale the
//       clients' WEIGHTS:  W_bar = fl(W[sel_0] * s0) + sum_{k>=1} fl(fl(fl(q_k * W[sel_k]) * te) / b_k)
//       -- s0 belongs to the fold's global first row only; the division is the correctly rounded
//       IEEE quotient (hipcc's default float `/`; a multiplication by 1/b differs in the last bit).
//   mode 2 (FS_NOVA_UPDATES)    Wang et al.'s normalised averaging of the clients' UPDATES:
//       W_bar = fl(base + sum_k fl(q_k * fl(W[sel_k] - base))).
//
// The first term of any range of k is the term itself, not 0 + term.  Regimes, sub-ranges, chunks
// and the stage-2 tree are fs_aggregate's, chosen by M (aggregate_sel.h): for M < 16 or
// chunks == 1 the exact left fold.
//
// HBM-bound as fs_aggregate_sel, whose design point this keeps: one float4 of the len parameters
// per thread, the loads of 8 rows in flight before the first fold of a group, the row indices of
// the next group loaded behind this group's rows, q_k / b_k uniform per k (scalar loads in the
// chunked form, one broadcast address per sub-range in the one-launch form).  M * len floats read
// (+ len of base in mode 2, per chunk or sub-range) and len written; rows outside sel never
// touched.  No atomics, no cross-workgroup wait, no allocation.
//
// Aliasing (mode 2, base == W_bar: the round plan's d_W_g): a position's base is read by the
// workgroup that writes that position, before it writes.  One-launch form: every sub-range's
// thread reads it before the barrier, the position's thread 0 writes after.  Two-stage form:
// stage 1 writes partials only, stage 2 reads base and writes; one chunk: one thread per position
// reads, folds and writes.
#include "aggregate_sel.h"
#include "common.h"
#include "finalize.h"

namespace fs {

// No fma contraction anywhere in this file (as aggregate.hip): every product, difference, quotient
// and sum rounds separately.
#pragma clang fp contract(off)

// the per-k coefficients of both modes (by value: kernel arguments)
struct NovaCoef {
  const int32_t* sel;   // [M] row ids, or nullptr: rows 0..M-1
  const float* q;       // [M]
  const float* b;       // [M], mode 1
  float te, s0;         // mode 1
};

// (SEL is a template parameter, not a test of the pointer: a run-time "load or not" select around
// each index makes hipcc branch around the loads and wait for them one by one)
template <bool SEL>
__device__ __forceinline__ int nova_row(const int32_t* __restrict__ sel, int k) { return SEL ? sel[k] : k; }

template <int MODE>
__device__ __forceinline__ float4 nova_term(bool first, float q, float b, float te, float s0, float4 w, float4 base) {
  if (MODE == 1) {
    if (first) return make_float4(w.x * s0, w.y * s0, w.z * s0, w.w * s0);
    return make_float4(((q * w.x) * te) / b, ((q * w.y) * te) / b, ((q * w.z) * te) / b, ((q * w.w) * te) / b);
  }
  return make_float4(q * (w.x - base.x), q * (w.y - base.y), q * (w.z - base.z), q * (w.w - base.w));
}

// One group of up to 8 terms k .. k+7 (< k1) folded onto acc, sel_fold_range's schedule: the 8 row
// loads issued before the first fold, the indices of the next group behind them.  No load sits
// under a condition: with the loads under `if (u < n)` hipcc branched around each one and waited
// vmcnt(0) before the next -- eight dependent round trips per group, 2 - 2.5 x the time at
// N = 1000 - 1250.  FULL: all 8 terms exist, nothing is conditional.  Else (a range's short last
// group): the loads re-read the range's last row (k clamped to k1 - 1: a sampled row, a cache
// hit), only the folds are skipped, and the coefficients are pinned where they are loaded (the
// empty asm) so that they are not sunk into the skipped folds one scalar round trip each.
template <int MODE, bool SEL, bool FULL>
__device__ __forceinline__ float4 nova_fold_group(const float* __restrict__ W, int64_t stride, const NovaCoef& c,
                                                  float4 base, float4 acc, int (&idx)[8], int k, int k0, int k1) {
  const int last = k1 - 1;
  float4 v[8];
  float qv[8], bv[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int ku = FULL ? k + u : min(k + u, last);
    v[u] = ld4(W + (int64_t)idx[u] * stride);
    qv[u] = c.q[ku];
    bv[u] = MODE == 1 ? c.b[ku] : 1.f;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = nova_row<SEL>(c.sel, min(k + 8 + u, last));
  if (!FULL) {
#pragma unroll
    for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(qv[u]), "+v"(bv[u]));
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (FULL || k + u < k1) {
      const float4 t = nova_term<MODE>(u == 0 && k == 0, qv[u], bv[u], c.te, c.s0, v[u], base);
      if (u == 0 && k == k0)
        acc = t;
      else
        acc = make_float4(acc.x + t.x, acc.y + t.y, acc.z + t.z, acc.w + t.w);
    }
  return acc;
}

// the left fold of the terms k = k0 .. k1-1 (k0 < k1) at one float4 position
template <int MODE, bool SEL>
__device__ __forceinline__ float4 nova_fold_range(const float* __restrict__ W, int64_t stride, const NovaCoef& c,
                                                  float4 base, int k0, int k1) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int idx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = nova_row<SEL>(c.sel, min(k0 + u, k1 - 1));
  int k = k0;
  for (; k + 8 <= k1; k += 8) acc = nova_fold_group<MODE, SEL, true>(W, stride, c, base, acc, idx, k, k0, k1);
  if (k < k1) acc = nova_fold_group<MODE, SEL, false>(W, stride, c, base, acc, idx, k, k0, k1);
  return acc;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// two-stage form, stage 1 (aggregate_kernel's geometry): chunk blockIdx.y folds k in
// [y * per, min(M, y * per + per)) into partial y.  FINAL (one chunk): straight into the output,
// mode 2 adding the base this thread read before it folds.
template <int MODE, bool SEL, bool FINAL>
__global__ __launch_bounds__(256) void aggregate_nova_kernel(const float* __restrict__ W, int64_t stride, NovaCoef c,
                                                            const float* base, int M, int64_t len4, int per_chunk,
                                                            float* out, int64_t out_stride) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len4) return;
  const int ch = blockIdx.y;
  const int k0 = ch * per_chunk;
  const int k1 = min(M, k0 + per_chunk);
  const float4 bs = MODE == 2 ? ld4(base + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc = nova_fold_range<MODE, SEL>(W + 4 * i, stride, c, bs, k0, k1);
  if (MODE == 2 && FINAL) acc = add4(bs, acc);
  st4(out + (int64_t)ch * out_stride + 4 * i, acc);
}

// mode 2's stage 2: fold_partials_kernel's tree (AG_FP_SUB threads per position, thread s folding
// the partials s, s + AG_FP_SUB, ... in order, thread 0 those sums in order), then base + delta
constexpr int NV_FP_POS = 256 / AG_FP_SUB;

__global__ __launch_bounds__(256) void nova_fold_partials_kernel(const float* __restrict__ part, int K, int64_t len4,
                                                                const float* base, float* out) {
  __shared__ float4 sums[AG_FP_SUB][NV_FP_POS];
  const int sub = threadIdx.x / NV_FP_POS, pl = threadIdx.x % NV_FP_POS;
  const int64_t i = (int64_t)blockIdx.x * NV_FP_POS + pl;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 bs = acc;
  if (i < len4 && sub < K) {
    if (sub == 0) bs = ld4(base + 4 * i);
    acc = ld4(part + (int64_t)sub * 4 * len4 + 4 * i);
    for (int k = sub + AG_FP_SUB; k < K; k += AG_FP_SUB) acc = add4(acc, ld4(part + (int64_t)k * 4 * len4 + 4 * i));
  }
  sums[sub][pl] = acc;
  __syncthreads();
  if (sub == 0 && i < len4) {
    float4 t = sums[0][pl];
    for (int s2 = 1; s2 < AG_FP_SUB && s2 < K; ++s2) t = add4(t, sums[s2][pl]);
    st4(out + 4 * i, add4(bs, t));
  }
}

// one-launch form (aggregate_one_kernel's geometry): SUB consecutive ranges of k per float4
// position folded by SUB threads of one workgroup, their partials folded in order in LDS; the
// deferred evaluation's finaliser rides as the last workgroup
template <int MODE, bool SEL, int SUB>
__global__ __launch_bounds__(256) void aggregate_nova_one_kernel(const float* __restrict__ W, int64_t stride,
                                                                NovaCoef c, const float* base, int M, int64_t len4,
                                                                int per, float* out, EvalFinalize fin) {
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
  float4 bs = acc;
  if (i < len4 && k0 < k1) {
    if (MODE == 2) bs = ld4(base + 4 * i);          // (sub 0 always has a range: M >= 1)
    acc = nova_fold_range<MODE, SEL>(W + 4 * i, stride, c, bs, k0, k1);
  }
  sums[sub][pl] = acc;
  __syncthreads();
  if (sub == 0 && i < len4) {
    float4 t = sums[0][pl];
    for (int s2 = 1; s2 < SUB && s2 * per < M; ++s2) t = add4(t, sums[s2][pl]);
    if (MODE == 2) t = add4(bs, t);
    st4(out + 4 * i, t);
  }
}

template <int MODE, bool SEL, int SUB>
static void launch_nova_one(const float* W, int64_t stride, const NovaCoef& c, const float* base, int M, int64_t len4,
                            float* out, const EvalFinalize& fin, hipStream_t st) {
  constexpr int POS = 256 / SUB;
  const int per = (M + SUB - 1) / SUB;
  const int64_t blocks = (len4 + POS - 1) / POS + (fin.part ? 1 : 0);
  hipLaunchKernelGGL((aggregate_nova_one_kernel<MODE, SEL, SUB>), dim3((unsigned)blocks), dim3(256), 0, st, W, stride, c,
                     base, M, len4, per, out, fin);
}

template <int MODE, bool SEL>
static int nova_launch_mode(const float* W, int64_t stride, const NovaCoef& c, const float* base, int M, int64_t len,
                            float* out, float* d_ws, int64_t ws_floats, int chunks, const EvalFinalize* fin,
                            hipStream_t st) {
  const int64_t len4 = len / 4;
  const EvalFinalize none{nullptr, 0, 0, nullptr};
  if (chunks <= 0 && M <= AG_ONE_MAX_N) {
    const EvalFinalize& f = fin ? *fin : none;
    switch (one_launch_sub(M)) {
      case 1: launch_nova_one<MODE, SEL, 1>(W, stride, c, base, M, len4, out, f, st); break;
      case 2: launch_nova_one<MODE, SEL, 2>(W, stride, c, base, M, len4, out, f, st); break;
      case 4: launch_nova_one<MODE, SEL, 4>(W, stride, c, base, M, len4, out, f, st); break;
      case 8: launch_nova_one<MODE, SEL, 8>(W, stride, c, base, M, len4, out, f, st); break;
      case 16: launch_nova_one<MODE, SEL, 16>(W, stride, c, base, M, len4, out, f, st); break;
      default: launch_nova_one<MODE, SEL, 32>(W, stride, c, base, M, len4, out, f, st); break;
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
    hipLaunchKernelGGL((aggregate_nova_kernel<MODE, SEL, true>), dim3((unsigned)bx, 1), dim3(256), 0, st, W, stride, c, base,
                       M, len4, per, out, (int64_t)0);
  } else {
    hipLaunchKernelGGL((aggregate_nova_kernel<MODE, SEL, false>), dim3((unsigned)bx, chunks), dim3(256), 0, st, W, stride, c,
                       base, M, len4, per, d_ws, len);
    if (MODE == 1)
      fold_partials_launch(d_ws, chunks, len4, out, st);
    else
      hipLaunchKernelGGL(nova_fold_partials_kernel, dim3((unsigned)((len4 + NV_FP_POS - 1) / NV_FP_POS)), dim3(256), 0,
                         st, d_ws, chunks, len4, base, out);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int aggregate_nova_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                          const float* d_b, float te, float s0, int mode, const float* d_W_base, int M, int64_t len,
                          float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks, const EvalFinalize* fin,
                          hipStream_t st) {
  FS_REQUIRE(mode == FS_NOVA_REFERENCE || mode == FS_NOVA_UPDATES, "mode must be FS_NOVA_REFERENCE or FS_NOVA_UPDATES");
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_q && d_W_bar, "null pointer");
  FS_REQUIRE(mode != FS_NOVA_REFERENCE || d_b, "mode 1 needs d_b");
  FS_REQUIRE(mode != FS_NOVA_UPDATES || d_W_base, "mode 2 needs d_W_base");
  const NovaCoef c{d_sel, d_q, d_b, te, s0};
#define FS_NOVA_GO(MODE, SEL, base) \
  return nova_launch_mode<MODE, SEL>(d_W_all, stride, c, base, M, len, d_W_bar, d_ws, ws_floats, chunks, fin, st)
  if (mode == FS_NOVA_REFERENCE) {
    if (d_sel) FS_NOVA_GO(1, true, nullptr);
    FS_NOVA_GO(1, false, nullptr);
  }
  if (d_sel) FS_NOVA_GO(2, true, d_W_base);
  FS_NOVA_GO(2, false, d_W_base);
#undef FS_NOVA_GO
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_nova(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                                 const float* d_b, float te, float s0, int mode, const float* d_W_base, int M,
                                 int64_t len, float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks,
                                 void* stream) {
  return aggregate_nova_launch(d_W_all, stride, d_sel, d_q, d_b, te, s0, mode, d_W_base, M, len, d_W_bar, d_ws,
                               ws_floats, chunks, nullptr, reinterpret_cast<hipStream_t>(stream));
}

// fs_aggregate_scaffold -- SCAFFOLD's server step: two folds over the M sampled rows of the
// clients x params buffer from ONE pass over those rows, both in place:
//
//   W_g <- fl(x + sum_k fl(q_k * fl(W[sel_k] - x)))                x = W_g before the call
//   c   <- fl(fl(cs * c) + sum_k fl(r_k * fl(x - W[sel_k])))
//
// in k order, every operation rounded separately.  The W_g fold is fs_aggregate_nova's mode 2
// (aggregate_nova.hip) term for term and regime for regime -- the same sub-ranges, chunks and
// stage-2 tree (aggregate_sel.h), the chunk clamp taken on half the workspace since every chunk
// keeps two partials -- so W_g is bitwise what mode 2 returns; the c fold has the same structure
// over its own terms: the first term of a range is the term itself, fl(cs * c) is added last.
//
// The identity behind the second fold: option II's c_i+ - c_i = -c + (x - W_i) / (K_i lr) needs no
// c_i, so with r_k = p_k / (K_k lr) and cs = 1 - sum_S p_k the server variate stays
// c = sum_j p_j c_j over ALL clients without reading the N x len variate buffer.
//
// HBM-bound; aggregate_nova.hip's load schedule: one float4 of the len parameters per thread, the
// loads of 8 rows in flight before the first fold of a group, the next group's row indices loaded
// behind them, no load under a condition; each row load feeds both accumulators.  (M + 2) * len
// floats read (+ len of x per further chunk or sub-range, cache hits) and 2 * len written, where
// two mode-2 launches read 2 (M + 1) * len.  No atomics, no cross-workgroup wait, no allocation.
//
// Aliasing (both outputs are updated in place): a position's x and c are read by the workgroup
// that writes that position, before it writes.  One-launch form: every sub-range's thread reads x
// (sub-range 0 also c) before the barrier, thread 0 of the position writes after.  Two-stage
// form: stage 1 reads x and writes partials only, stage 2 reads x and c and writes; one chunk:
// one thread per position reads, folds and writes.
#include "aggregate_sel.h"
#include "common.h"
#include "scaffold.h"

namespace fs {

// No fma contraction anywhere in this file (as aggregate_nova.hip)
#pragma clang fp contract(off)

struct ScafCoef {
  const int32_t* sel;   // [M] row ids, or nullptr: rows 0..M-1
  const float* q;       // [M]
  const float* r;       // [M]
};

struct Acc2 {
  float4 w, c;
};

// (a template parameter, not a test of the pointer: see aggregate_nova.hip)
template <bool SEL>
__device__ __forceinline__ int scaf_row(const int32_t* __restrict__ sel, int k) { return SEL ? sel[k] : k; }

__device__ __forceinline__ float4 sadd4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// One group of up to 8 terms k .. k+7 (< k1) folded onto both accumulators: nova_fold_group's
// schedule (FULL: all 8 exist; else the loads re-read the range's last row and only the folds are
// skipped, the coefficients pinned where they are loaded).
template <bool SEL, bool FULL>
__device__ __forceinline__ Acc2 scaf_fold_group(const float* __restrict__ W, int64_t stride, const ScafCoef& c,
                                                float4 x, Acc2 acc, int (&idx)[8], int k, int k0, int k1) {
  const int last = k1 - 1;
  float4 v[8];
  float qv[8], rv[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int ku = FULL ? k + u : min(k + u, last);
    v[u] = ld4(W + (int64_t)idx[u] * stride);
    qv[u] = c.q[ku];
    rv[u] = c.r[ku];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = scaf_row<SEL>(c.sel, min(k + 8 + u, last));
  if (!FULL) {
#pragma unroll
    for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(qv[u]), "+v"(rv[u]));
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (FULL || k + u < k1) {
      const float4 w = v[u];
      const float4 tw = make_float4(qv[u] * (w.x - x.x), qv[u] * (w.y - x.y), qv[u] * (w.z - x.z), qv[u] * (w.w - x.w));
      const float4 tc = make_float4(rv[u] * (x.x - w.x), rv[u] * (x.y - w.y), rv[u] * (x.z - w.z), rv[u] * (x.w - w.w));
      if (u == 0 && k == k0) {
        acc.w = tw;
        acc.c = tc;
      } else {
        acc.w = sadd4(acc.w, tw);
        acc.c = sadd4(acc.c, tc);
      }
    }
  return acc;
}

// the two left folds of the terms k = k0 .. k1-1 (k0 < k1) at one float4 position
template <bool SEL>
__device__ __forceinline__ Acc2 scaf_fold_range(const float* __restrict__ W, int64_t stride, const ScafCoef& c, float4 x,
                                                int k0, int k1) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  Acc2 acc{z, z};
  int idx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = scaf_row<SEL>(c.sel, min(k0 + u, k1 - 1));
  int k = k0;
  for (; k + 8 <= k1; k += 8) acc = scaf_fold_group<SEL, true>(W, stride, c, x, acc, idx, k, k0, k1);
  if (k < k1) acc = scaf_fold_group<SEL, false>(W, stride, c, x, acc, idx, k, k0, k1);
  return acc;
}

__device__ __forceinline__ float4 scaled4(float s, float4 v) { return make_float4(s * v.x, s * v.y, s * v.z, s * v.w); }

// two-stage form, stage 1: chunk blockIdx.y folds k in [y * per, min(M, y * per + per)) into its
// two partials (out_w / out_c + y * part_stride).  FINAL (one chunk): straight into W_g and c.
template <bool SEL, bool FINAL>
__global__ __launch_bounds__(256) void aggregate_scaffold_kernel(const float* __restrict__ W, int64_t stride, ScafCoef c,
                                                                float cs, int M, int64_t len4, int per_chunk,
                                                                const float* xin, const float* cin, float* out_w,
                                                                float* out_c, int64_t part_stride) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len4) return;
  const int ch = blockIdx.y;
  const int k0 = ch * per_chunk;
  const int k1 = min(M, k0 + per_chunk);
  const float4 x = ld4(xin + 4 * i);
  float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (FINAL) cv = ld4(cin + 4 * i);
  Acc2 acc = scaf_fold_range<SEL>(W + 4 * i, stride, c, x, k0, k1);
  if (FINAL) {
    acc.w = sadd4(x, acc.w);
    acc.c = sadd4(scaled4(cs, cv), acc.c);
  }
  st4(out_w + (int64_t)ch * part_stride + 4 * i, acc.w);
  st4(out_c + (int64_t)ch * part_stride + 4 * i, acc.c);
}

// stage 2: nova_fold_partials_kernel's tree for both sets of partials (AG_FP_SUB threads per
// position, thread s folding the partials s, s + AG_FP_SUB, ... in order, thread 0 those sums in
// order), then x + delta and fl(cs * c) + delta
constexpr int SC_FP_POS = 256 / AG_FP_SUB;

__global__ __launch_bounds__(256) void scaffold_fold_partials_kernel(const float* __restrict__ part_w,
                                                                    const float* __restrict__ part_c, int K,
                                                                    int64_t len4, float cs, float* W_g, float* c_g) {
  __shared__ float4 sums[2][AG_FP_SUB][SC_FP_POS];
  const int sub = threadIdx.x / SC_FP_POS, pl = threadIdx.x % SC_FP_POS;
  const int64_t i = (int64_t)blockIdx.x * SC_FP_POS + pl;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 aw = z, ac = z, x = z, cv = z;
  if (i < len4 && sub < K) {
    if (sub == 0) {
      x = ld4(W_g + 4 * i);
      cv = ld4(c_g + 4 * i);
    }
    aw = ld4(part_w + (int64_t)sub * 4 * len4 + 4 * i);
    ac = ld4(part_c + (int64_t)sub * 4 * len4 + 4 * i);
    for (int k = sub + AG_FP_SUB; k < K; k += AG_FP_SUB) {
      aw = sadd4(aw, ld4(part_w + (int64_t)k * 4 * len4 + 4 * i));
      ac = sadd4(ac, ld4(part_c + (int64_t)k * 4 * len4 + 4 * i));
    }
  }
  sums[0][sub][pl] = aw;
  sums[1][sub][pl] = ac;
  __syncthreads();
  if (sub == 0 && i < len4) {
    float4 tw = sums[0][0][pl], tc = sums[1][0][pl];
    for (int s2 = 1; s2 < AG_FP_SUB && s2 < K; ++s2) {
      tw = sadd4(tw, sums[0][s2][pl]);
      tc = sadd4(tc, sums[1][s2][pl]);
    }
    st4(W_g + 4 * i, sadd4(x, tw));
    st4(c_g + 4 * i, sadd4(scaled4(cs, cv), tc));
  }
}

// one-launch form (aggregate_nova_one_kernel's geometry): SUB consecutive ranges of k per float4
// position folded by SUB threads of one workgroup, their partials folded in order in LDS
template <bool SEL, int SUB>
__global__ __launch_bounds__(256) void aggregate_scaffold_one_kernel(const float* __restrict__ W, int64_t stride,
                                                                    ScafCoef c, float cs, int M, int64_t len4, int per,
                                                                    float* W_g, float* c_g) {
  constexpr int POS = 256 / SUB;
  __shared__ float4 sums[2][SUB][POS];
  const int sub = threadIdx.x / POS, pl = threadIdx.x % POS;
  const int64_t i = (int64_t)blockIdx.x * POS + pl;
  const int k0 = sub * per, k1 = min(M, k0 + per);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  Acc2 acc{z, z};
  float4 x = z, cv = z;
  if (i < len4 && k0 < k1) {
    x = ld4(W_g + 4 * i);                           // (sub 0 always has a range: M >= 1)
    if (sub == 0) cv = ld4(c_g + 4 * i);
    acc = scaf_fold_range<SEL>(W + 4 * i, stride, c, x, k0, k1);
  }
  sums[0][sub][pl] = acc.w;
  sums[1][sub][pl] = acc.c;
  __syncthreads();
  if (sub == 0 && i < len4) {
    float4 tw = sums[0][0][pl], tc = sums[1][0][pl];
    for (int s2 = 1; s2 < SUB && s2 * per < M; ++s2) {
      tw = sadd4(tw, sums[0][s2][pl]);
      tc = sadd4(tc, sums[1][s2][pl]);
    }
    st4(W_g + 4 * i, sadd4(x, tw));
    st4(c_g + 4 * i, sadd4(scaled4(cs, cv), tc));
  }
}

template <bool SEL, int SUB>
static void launch_scaffold_one(const float* W, int64_t stride, const ScafCoef& c, float cs, int M, int64_t len4,
                                float* W_g, float* c_g, hipStream_t st) {
  constexpr int POS = 256 / SUB;
  const int per = (M + SUB - 1) / SUB;
  const int64_t blocks = (len4 + POS - 1) / POS;
  hipLaunchKernelGGL((aggregate_scaffold_one_kernel<SEL, SUB>), dim3((unsigned)blocks), dim3(256), 0, st, W, stride, c, cs,
                     M, len4, per, W_g, c_g);
}

template <bool SEL>
static int scaffold_launch_sel(const float* W, int64_t stride, const ScafCoef& c, float cs, int M, int64_t len, float* W_g,
                               float* c_g, float* d_ws, int64_t ws_floats, int chunks, hipStream_t st) {
  const int64_t len4 = len / 4;
  if (chunks <= 0 && M <= AG_ONE_MAX_N) {
    switch (one_launch_sub(M)) {
      case 1: launch_scaffold_one<SEL, 1>(W, stride, c, cs, M, len4, W_g, c_g, st); break;
      case 2: launch_scaffold_one<SEL, 2>(W, stride, c, cs, M, len4, W_g, c_g, st); break;
      case 4: launch_scaffold_one<SEL, 4>(W, stride, c, cs, M, len4, W_g, c_g, st); break;
      case 8: launch_scaffold_one<SEL, 8>(W, stride, c, cs, M, len4, W_g, c_g, st); break;
      case 16: launch_scaffold_one<SEL, 16>(W, stride, c, cs, M, len4, W_g, c_g, st); break;
      default: launch_scaffold_one<SEL, 32>(W, stride, c, cs, M, len4, W_g, c_g, st); break;
    }
    FS_LAUNCH_CHECK();
    return FS_OK;
  }
  const int64_t bx = (len4 + 255) / 256;
  int per = 0;
  // two partials per chunk: the clamp sees half the workspace (what mode 2 is held against)
  chunks = aggregate_chunks(M, chunks, d_ws != nullptr, ws_floats / 2, len, &per);
  if (chunks == 1) {
    hipLaunchKernelGGL((aggregate_scaffold_kernel<SEL, true>), dim3((unsigned)bx, 1), dim3(256), 0, st, W, stride, c, cs, M,
                       len4, per, W_g, c_g, W_g, c_g, (int64_t)0);
  } else {
    float* part_w = d_ws;
    float* part_c = d_ws + (int64_t)chunks * len;
    hipLaunchKernelGGL((aggregate_scaffold_kernel<SEL, false>), dim3((unsigned)bx, chunks), dim3(256), 0, st, W, stride, c,
                       cs, M, len4, per, W_g, c_g, part_w, part_c, len);
    hipLaunchKernelGGL(scaffold_fold_partials_kernel, dim3((unsigned)((len4 + SC_FP_POS - 1) / SC_FP_POS)), dim3(256), 0,
                       st, part_w, part_c, chunks, len4, cs, W_g, c_g);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int aggregate_scaffold_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                              const float* d_r, float cs, int M, int64_t len, float* d_W_g, float* d_c, float* d_ws,
                              int64_t ws_floats, int chunks, hipStream_t st) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_q && d_r && d_W_g && d_c, "null pointer");
  FS_REQUIRE(d_W_g != d_c, "d_W_g and d_c must be different buffers");
  const ScafCoef c{d_sel, d_q, d_r};
  if (d_sel) return scaffold_launch_sel<true>(d_W_all, stride, c, cs, M, len, d_W_g, d_c, d_ws, ws_floats, chunks, st);
  return scaffold_launch_sel<false>(d_W_all, stride, c, cs, M, len, d_W_g, d_c, d_ws, ws_floats, chunks, st);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_scaffold(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                                     const float* d_r, float cs, int M, int64_t len, float* d_W_g, float* d_c,
                                     float* d_ws, int64_t ws_floats, int chunks, void* stream) {
  return aggregate_scaffold_launch(d_W_all, stride, d_sel, d_q, d_r, cs, M, len, d_W_g, d_c, d_ws, ws_floats, chunks,
                                   reinterpret_cast<hipStream_t>(stream));
}

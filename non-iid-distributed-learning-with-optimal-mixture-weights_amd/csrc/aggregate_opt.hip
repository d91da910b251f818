// fs_aggregate_opt -- the FedOpt server step (Reddi et al., ICLR 2021, Algorithm 2; FedAvgM, Hsu et
// al. 2019): the fold of the M sampled clients' updates with an element-wise optimizer step fused
// onto its end, all three state buffers in place.  With x = W_g, m, v on entry:
//
//   delta = sum_k fl(q_k * fl(W[sel_k] - x))                     (k ascending)
//   AVGM     m' = fl(fl(beta1*m) + delta)                         x' = fl(x + fl(eta*m'))
//   others   m' = fl(fl(beta1*m) + fl(omb1*delta)),  d2 = fl(delta*delta)
//     ADAGRAD  v' = fl(v + d2)
//     ADAM     v' = fl(fl(beta2*v) + fl(omb2*d2))
//     YOGI     v' = fl(v - fl(fl(omb2*d2) * s)),  s = sgn(fl(v - d2))
//            x' = fl(x + fl(fl(eta*m') / fl(sqrtf(v') + tau)))
//
// every operation rounded separately, the quotient and the square root the correctly rounded IEEE
// ones, no bias correction (as the paper).  The fold is fs_aggregate_nova's mode 2
// (aggregate_nova.hip) before it adds its base, term for term and regime for regime: the same
// sub-ranges, chunks (one partial per chunk: the clamp sees the whole workspace) and stage-2 tree
// (aggregate_sel.h), the first term of a range the term itself.  AVGM with beta1 = 0, eta = 1 is
// therefore bitwise mode 2.
//
// HBM-bound; aggregate_nova.hip's load schedule: one float4 of the len parameters per thread, the
// loads of 8 rows in flight before the first fold of a group, the next group's row indices loaded
// behind them, no load under a condition.  The finish runs once per element, in the thread that
// writes the position -- some 30 VALU operations per element against M row loads, off the
// stream's critical path.  (M + 3) * len floats read and 3 * len written (AVGM: M + 2 and 2; + len
// of x per further chunk or sub-range, cache hits).  No atomics, no cross-workgroup wait, no
// allocation.
//
// Aliasing (all three buffers are updated in place): a position's x, m and v are read by the
// workgroup that writes that position, before it writes.  One-launch form: every sub-range's
// thread reads x (sub-range 0 also m and v) before the barrier, thread 0 of the position finishes
// and writes after.  Two-stage form: stage 1 reads x and writes delta partials only, stage 2 folds
// them by the fixed tree, reads x / m / v and writes; one chunk: one thread per position reads,
// folds, finishes and writes.
#include "aggregate_sel.h"
#include "common.h"
#include "finalize.h"

namespace fs {

// No fma contraction anywhere in this file (as aggregate_nova.hip)
#pragma clang fp contract(off)

struct OptCoef {
  const int32_t* sel;   // [M] row ids, or nullptr: rows 0..M-1
  const float* q;       // [M]
};

// the server step's scalars (by value: kernel arguments); the rule is uniform over the launch
struct OptStep {
  int rule;
  float eta, beta1, omb1, beta2, omb2, tau;
};

// a position's state: x, m, v before the step, x', m', v' after
struct OptState {
  float4 x, m, v;
};

// (a template parameter, not a test of the pointer: see aggregate_nova.hip)
template <bool SEL>
__device__ __forceinline__ int opt_row(const int32_t* __restrict__ sel, int k) { return SEL ? sel[k] : k; }

__device__ __forceinline__ float4 oadd4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// One group of up to 8 terms k .. k+7 (< k1) folded onto acc: nova_fold_group's schedule in mode 2
// (FULL: all 8 exist; else the loads re-read the range's last row and only the folds are skipped,
// the coefficients pinned where they are loaded).
template <bool SEL, bool FULL>
__device__ __forceinline__ float4 opt_fold_group(const float* __restrict__ W, int64_t stride, const OptCoef& c, float4 x,
                                                 float4 acc, int (&idx)[8], int k, int k0, int k1) {
  const int last = k1 - 1;
  float4 v[8];
  float qv[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int ku = FULL ? k + u : min(k + u, last);
    v[u] = ld4(W + (int64_t)idx[u] * stride);
    qv[u] = c.q[ku];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = opt_row<SEL>(c.sel, min(k + 8 + u, last));
  if (!FULL) {
#pragma unroll
    for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(qv[u]));
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (FULL || k + u < k1) {
      const float4 w = v[u];
      const float4 t = make_float4(qv[u] * (w.x - x.x), qv[u] * (w.y - x.y), qv[u] * (w.z - x.z), qv[u] * (w.w - x.w));
      if (u == 0 && k == k0)
        acc = t;
      else
        acc = oadd4(acc, t);
    }
  return acc;
}

// the left fold of the terms k = k0 .. k1-1 (k0 < k1) at one float4 position
template <bool SEL>
__device__ __forceinline__ float4 opt_fold_range(const float* __restrict__ W, int64_t stride, const OptCoef& c, float4 x,
                                                 int k0, int k1) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int idx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = opt_row<SEL>(c.sel, min(k0 + u, k1 - 1));
  int k = k0;
  for (; k + 8 <= k1; k += 8) acc = opt_fold_group<SEL, true>(W, stride, c, x, acc, idx, k, k0, k1);
  if (k < k1) acc = opt_fold_group<SEL, false>(W, stride, c, x, acc, idx, k, k0, k1);
  return acc;
}

// the server step at one element.  YOGI's sign is a select (a NaN difference selects 0).
__device__ __forceinline__ void opt_step1(const OptStep& p, float d, float& x, float& m, float& v) {
  if (p.rule == FS_OPT_AVGM) {
    m = p.beta1 * m + d;
    x = x + p.eta * m;
    return;
  }
  const float d2 = d * d;
  m = p.beta1 * m + p.omb1 * d;
  if (p.rule == FS_OPT_ADAGRAD) {
    v = v + d2;
  } else if (p.rule == FS_OPT_ADAM) {
    v = p.beta2 * v + p.omb2 * d2;
  } else {
    const float t = v - d2;
    const float s = t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f);
    v = v - (p.omb2 * d2) * s;
  }
  x = x + (p.eta * m) / (sqrtf(v) + p.tau);
}

__device__ __forceinline__ void opt_step4(const OptStep& p, float4 d, OptState& s) {
  opt_step1(p, d.x, s.x.x, s.m.x, s.v.x);
  opt_step1(p, d.y, s.x.y, s.m.y, s.v.y);
  opt_step1(p, d.z, s.x.z, s.m.z, s.v.z);
  opt_step1(p, d.w, s.x.w, s.m.w, s.v.w);
}

// a position's m and v (v only where the rule has one: AVGM's d_v may be NULL)
__device__ __forceinline__ void opt_load_mv(const OptStep& p, const float* m, const float* v, int64_t i, OptState& s) {
  s.m = ld4(m + 4 * i);
  if (p.rule != FS_OPT_AVGM) s.v = ld4(v + 4 * i);
}

__device__ __forceinline__ void opt_store(const OptStep& p, float* x, float* m, float* v, int64_t i, const OptState& s) {
  st4(x + 4 * i, s.x);
  st4(m + 4 * i, s.m);
  if (p.rule != FS_OPT_AVGM) st4(v + 4 * i, s.v);
}

// two-stage form, stage 1 (aggregate_nova_kernel's geometry): chunk blockIdx.y folds k in
// [y * per, min(M, y * per + per)) into delta partial y.  FINAL (one chunk): fold, step and write
// in the one thread of the position.
template <bool SEL, bool FINAL>
__global__ __launch_bounds__(256) void aggregate_opt_kernel(const float* __restrict__ W, int64_t stride, OptCoef c,
                                                           OptStep p, int M, int64_t len4, int per_chunk, float* W_g,
                                                           float* m_g, float* v_g, float* part) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len4) return;
  const int ch = blockIdx.y;
  const int k0 = ch * per_chunk;
  const int k1 = min(M, k0 + per_chunk);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  OptState s{ld4(W_g + 4 * i), z, z};
  if (FINAL) opt_load_mv(p, m_g, v_g, i, s);
  const float4 acc = opt_fold_range<SEL>(W + 4 * i, stride, c, s.x, k0, k1);
  if (FINAL) {
    opt_step4(p, acc, s);
    opt_store(p, W_g, m_g, v_g, i, s);
  } else {
    st4(part + (int64_t)ch * 4 * len4 + 4 * i, acc);
  }
}

// stage 2: nova_fold_partials_kernel's tree (AG_FP_SUB threads per position, thread s folding the
// partials s, s + AG_FP_SUB, ... in order, thread 0 those sums in order), then the step
constexpr int OP_FP_POS = 256 / AG_FP_SUB;

__global__ __launch_bounds__(256) void opt_fold_partials_kernel(const float* __restrict__ part, int K, int64_t len4,
                                                               OptStep p, float* W_g, float* m_g, float* v_g) {
  __shared__ float4 sums[AG_FP_SUB][OP_FP_POS];
  const int sub = threadIdx.x / OP_FP_POS, pl = threadIdx.x % OP_FP_POS;
  const int64_t i = (int64_t)blockIdx.x * OP_FP_POS + pl;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc = z;
  OptState s{z, z, z};
  if (i < len4 && sub < K) {
    if (sub == 0) {
      s.x = ld4(W_g + 4 * i);
      opt_load_mv(p, m_g, v_g, i, s);
    }
    acc = ld4(part + (int64_t)sub * 4 * len4 + 4 * i);
    for (int k = sub + AG_FP_SUB; k < K; k += AG_FP_SUB) acc = oadd4(acc, ld4(part + (int64_t)k * 4 * len4 + 4 * i));
  }
  sums[sub][pl] = acc;
  __syncthreads();
  if (sub == 0 && i < len4) {
    float4 t = sums[0][pl];
    for (int s2 = 1; s2 < AG_FP_SUB && s2 < K; ++s2) t = oadd4(t, sums[s2][pl]);
    opt_step4(p, t, s);
    opt_store(p, W_g, m_g, v_g, i, s);
  }
}

// one-launch form (aggregate_nova_one_kernel's geometry): SUB consecutive ranges of k per float4
// position folded by SUB threads of one workgroup, their partials folded in order in LDS, the
// step in thread 0 of the position; the deferred evaluation's finaliser rides as the last workgroup
template <bool SEL, int SUB>
__global__ __launch_bounds__(256) void aggregate_opt_one_kernel(const float* __restrict__ W, int64_t stride, OptCoef c,
                                                               OptStep p, int M, int64_t len4, int per, float* W_g,
                                                               float* m_g, float* v_g, EvalFinalize fin) {
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
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc = z;
  OptState s{z, z, z};
  if (i < len4 && k0 < k1) {
    s.x = ld4(W_g + 4 * i);                         // (sub 0 always has a range: M >= 1)
    if (sub == 0) opt_load_mv(p, m_g, v_g, i, s);
    acc = opt_fold_range<SEL>(W + 4 * i, stride, c, s.x, k0, k1);
  }
  sums[sub][pl] = acc;
  __syncthreads();
  if (sub == 0 && i < len4) {
    float4 t = sums[0][pl];
    for (int s2 = 1; s2 < SUB && s2 * per < M; ++s2) t = oadd4(t, sums[s2][pl]);
    opt_step4(p, t, s);
    opt_store(p, W_g, m_g, v_g, i, s);
  }
}

template <bool SEL, int SUB>
static void launch_opt_one(const float* W, int64_t stride, const OptCoef& c, const OptStep& p, int M, int64_t len4,
                           float* W_g, float* m_g, float* v_g, const EvalFinalize& fin, hipStream_t st) {
  constexpr int POS = 256 / SUB;
  const int per = (M + SUB - 1) / SUB;
  const int64_t blocks = (len4 + POS - 1) / POS + (fin.part ? 1 : 0);
  hipLaunchKernelGGL((aggregate_opt_one_kernel<SEL, SUB>), dim3((unsigned)blocks), dim3(256), 0, st, W, stride, c, p, M,
                     len4, per, W_g, m_g, v_g, fin);
}

template <bool SEL>
static int opt_launch_sel(const float* W, int64_t stride, const OptCoef& c, const OptStep& p, int M, int64_t len,
                          float* W_g, float* m_g, float* v_g, float* d_ws, int64_t ws_floats, int chunks,
                          const EvalFinalize* fin, hipStream_t st) {
  const int64_t len4 = len / 4;
  const EvalFinalize none{nullptr, 0, 0, nullptr};
  if (chunks <= 0 && M <= AG_ONE_MAX_N) {
    const EvalFinalize& f = fin ? *fin : none;
    switch (one_launch_sub(M)) {
      case 1: launch_opt_one<SEL, 1>(W, stride, c, p, M, len4, W_g, m_g, v_g, f, st); break;
      case 2: launch_opt_one<SEL, 2>(W, stride, c, p, M, len4, W_g, m_g, v_g, f, st); break;
      case 4: launch_opt_one<SEL, 4>(W, stride, c, p, M, len4, W_g, m_g, v_g, f, st); break;
      case 8: launch_opt_one<SEL, 8>(W, stride, c, p, M, len4, W_g, m_g, v_g, f, st); break;
      case 16: launch_opt_one<SEL, 16>(W, stride, c, p, M, len4, W_g, m_g, v_g, f, st); break;
      default: launch_opt_one<SEL, 32>(W, stride, c, p, M, len4, W_g, m_g, v_g, f, st); break;
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
    hipLaunchKernelGGL((aggregate_opt_kernel<SEL, true>), dim3((unsigned)bx, 1), dim3(256), 0, st, W, stride, c, p, M, len4,
                       per, W_g, m_g, v_g, (float*)nullptr);
  } else {
    hipLaunchKernelGGL((aggregate_opt_kernel<SEL, false>), dim3((unsigned)bx, chunks), dim3(256), 0, st, W, stride, c, p, M,
                       len4, per, W_g, m_g, v_g, d_ws);
    hipLaunchKernelGGL(opt_fold_partials_kernel, dim3((unsigned)((len4 + OP_FP_POS - 1) / OP_FP_POS)), dim3(256), 0, st,
                       d_ws, chunks, len4, p, W_g, m_g, v_g);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int aggregate_opt_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int rule,
                         float eta, float beta1, float omb1, float beta2, float omb2, float tau, int M, int64_t len,
                         float* d_W_g, float* d_m, float* d_v, float* d_ws, int64_t ws_floats, int chunks,
                         const EvalFinalize* fin, hipStream_t st) {
  FS_REQUIRE(rule >= FS_OPT_AVGM && rule <= FS_OPT_YOGI, "rule must be FS_OPT_AVGM, _ADAGRAD, _ADAM or _YOGI");
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_q && d_W_g && d_m, "null pointer");
  FS_REQUIRE(rule == FS_OPT_AVGM || d_v, "the rule needs d_v");
  FS_REQUIRE(rule == FS_OPT_AVGM || tau > 0.f, "tau must be > 0");
  FS_REQUIRE(d_W_g != d_m && (!d_v || (d_v != d_W_g && d_v != d_m)), "d_W_g, d_m and d_v must be different buffers");
  const OptCoef c{d_sel, d_q};
  const OptStep p{rule, eta, beta1, omb1, beta2, omb2, tau};
  if (d_sel)
    return opt_launch_sel<true>(d_W_all, stride, c, p, M, len, d_W_g, d_m, d_v, d_ws, ws_floats, chunks, fin, st);
  return opt_launch_sel<false>(d_W_all, stride, c, p, M, len, d_W_g, d_m, d_v, d_ws, ws_floats, chunks, fin, st);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_opt(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int rule,
                                float eta, float beta1, float omb1, float beta2, float omb2, float tau, int M,
                                int64_t len, float* d_W_g, float* d_m, float* d_v, float* d_ws, int64_t ws_floats,
                                int chunks, void* stream) {
  return aggregate_opt_launch(d_W_all, stride, d_sel, d_q, rule, eta, beta1, omb1, beta2, omb2, tau, M, len, d_W_g, d_m,
                              d_v, d_ws, ws_floats, chunks, nullptr, reinterpret_cast<hipStream_t>(stream));
}

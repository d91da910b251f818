// fs_aggregate_qffl -- the q-FedAvg server step (q-FFL; Li, Sanjabi, Beirami, Smith, ICLR 2020) from
// one pass over the M sampled clients' rows: the weighted fold of their updates AND every update's
// squared norm, from the same loads.  With x = W_g on entry, k ascending:
//
//   d_k   = fl(W[sel_k] - x)                         (element-wise; the one difference both sums use)
//   S     = sum_k fl(u_k * d_k)                      fs_aggregate_nova's mode 2 before it adds its base
//   n_k   = sum_i d_k[i]^2                           float inside a wave's share, double above it
//   U = sum_k (double)u_k,  G = sum_k (double)g_k * n_k,  H = Lc*U + G     (double, k ascending)
//   coef  = (float)(Lc / H)   (0 when H is not finite or <= 0: the model is then left as it is)
//   x'    = fl(x + fl(coef * S))
//
// The fold is aggregate_opt.hip's, term for term and regime for regime (one_launch_sub,
// aggregate_chunks, AG_FP_SUB of aggregate_geom.h, the stage-2 tree of aggregate_fold.h; the first
// term of a range is the term itself), so S is bitwise fs_aggregate_opt's delta.  The kernels stay
// this file's own: the range fold runs the wave in lockstep and writes the norm table.  Its load schedule too: one float4 of
// the len parameters per thread, 8 row loads in flight, the next group's row indices loaded behind
// them, no load under a condition (a short last group loads clamped and skips its folds and its
// norm terms).
//
// Norms.  A thread's term of row k is e = ((dx^2 + dy^2) + dz^2) + dw^2 (4 squares, 3 sums, each
// rounded).  The 8 terms of a group of rows are summed over the LANES = min(64, positions per
// sub-range) lanes that hold the same rows by a reduce-scatter over DPP / permlane exchanges
// (lanes.h): log2(LANES) <= 6 further roundings per row, a fixed tree, every row's share in
// LANES / 8 lanes.  That float -- one wave's share of one row, at most 10 roundings -- is stored to
// the partial table nt[column][M] (column: the wave's place along the positions; every (column, k)
// is written exactly once, zeros from lanes past len4), the shares of LANES / 8 groups in one store
// of LANES rows.  qffl_norms_kernel then sums a row's columns in double in a fixed order, one
// workgroup per row; nothing depends on timing.  The cross-lane exchanges
// run in wave-uniform control flow: every sub-range walks ceil(per / 8) groups, and a lane past
// len4 or past its range's end computes on clamped loads and contributes zero.
//
// Finish: qffl_step_kernel; every workgroup sums U and G itself (k ascending, double: M dependent
// adds from LDS per sum, the two chains in two waves side by side) and applies the step to its
// positions; workgroup 0 writes d_hc.  The chains are what the contract's order costs: some 8 ns
// per client on the launch's critical path.
//
// (M + 1) * len floats read by the pass; the table is M * len / 256 floats where a sub-range has 64
// or more positions (up to M * len / 32 at M >= 192), the later launches touch len- and M-sized
// data only.  No atomics, no cross-workgroup wait, no allocation, no host synchronisation.
//
// Aliasing: the pass reads x and writes S, the table and (two-stage form) the partials; only the
// step writes W_g, each position by the thread that read it.  d_S must not be d_W_g.
//
// fs_qffl_coef: the round's coefficients u_k = p_k Ft^q, g_k = p_k q Ft^(q-1) L^2 from the losses
// fs_eval_clients left on the device, in double, rounded once.
#include "aggregate_fold.h"
#include "aggregate_sel.h"
#include "lanes.h"

namespace fs {

// No fma contraction anywhere in this file (as aggregate_nova.hip)
#pragma clang fp contract(off)

struct QfCoef {
  const int32_t* sel;   // [M] row ids, or nullptr: rows 0..M-1
  const float* u;       // [M]
};

// One group of up to 8 terms k .. k+7 (< k1) folded onto acc, aggregate_fold.h's fold_group schedule; e[u] is
// the thread's norm term of row k + u (left as it is where the row does not exist).
template <bool SEL, bool FULL>
__device__ __forceinline__ float4 qf_fold_group(const float* __restrict__ W, int64_t stride, const QfCoef& c, float4 x,
                                                float4 acc, int (&idx)[8], int k, int k0, int k1, float (&e)[8]) {
  const int last = k1 - 1;
  float4 v[8];
  float uv[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int ku = FULL ? k + u : min(k + u, last);
    v[u] = ld4(W + (int64_t)idx[u] * stride);
    uv[u] = c.u[ku];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = fold_row<SEL>(c.sel, min(k + 8 + u, last));
  if (!FULL) {
#pragma unroll
    for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(uv[u]));
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (FULL || k + u < k1) {
      const float4 w = v[u];
      const float4 d = make_float4(w.x - x.x, w.y - x.y, w.z - x.z, w.w - x.w);
      const float4 t = make_float4(uv[u] * d.x, uv[u] * d.y, uv[u] * d.z, uv[u] * d.w);
      e[u] = ((d.x * d.x + d.y * d.y) + d.z * d.z) + d.w * d.w;
      if (u == 0 && k == k0)
        acc = t;
      else
        acc = add4(acc, t);
    }
  return acc;
}

// The 8 per-lane terms v[0..7] summed over each aligned segment of LANES lanes (8, 16, 32 or 64):
// three reduce-scatter levels, then the butterfly on what is left.  Lane l of a segment returns
// the total of v[(l / (LANES / 8)) & 7]; log2(LANES) roundings per total, a fixed tree.  Every lane
// of the wave must be active.
template <int LANES>
__device__ __forceinline__ float qf_reduce8(float (&v)[8], int lane) {
  int off = LANES / 2;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = rs_pair(v[i], v[i + 4], off, lane);
  off /= 2;
#pragma unroll
  for (int i = 0; i < 2; ++i) v[i] = rs_pair(v[i], v[i + 2], off, lane);
  off /= 2;
  float o = rs_pair(v[0], v[1], off, lane);
#pragma unroll
  for (off /= 2; off >= 1; off /= 2) o += xor_get(o, off, lane);
  return o;
}

// The left fold of the terms k = k0 .. k1-1 at one float4 position, and the rows' norm shares into
// this segment's column of the table (col [M], indexed by k).  groups = ceil(per / 8) is the same
// for every lane of the wave (k1 - k0 <= per; an empty or shorter range idles through the rest);
// live: the position exists (else the loads were clamped and the terms count as zero).
template <bool SEL, int LANES>
__device__ __forceinline__ float4 qf_fold_range(const float* __restrict__ W, int64_t stride, const QfCoef& c, float4 x,
                                                int k0, int k1, int groups, bool live, float* __restrict__ col) {
  // Lane l of a segment ends a group with row r's total, r = (l / GW) & 7, in all GW = LANES / 8
  // lanes of that r: lane j of them keeps group g's total where g % GW == j, and the totals of GW
  // groups (LANES rows) go out in one store, every lane one row, instead of GW stores of 8 rows
  // between the loads of consecutive groups.
  constexpr int GW = LANES / 8;
  const int lane = threadIdx.x & 63;
  const int r = (lane / GW) & 7, j = lane % GW;
  float keep = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int idx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) idx[u] = k0 < k1 ? fold_row<SEL>(c.sel, min(k0 + u, k1 - 1)) : 0;
  for (int g = 0; g < groups; ++g) {
    const int k = k0 + 8 * g;
    float e[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) e[u] = 0.f;
    if (k + 8 <= k1)
      acc = qf_fold_group<SEL, true>(W, stride, c, x, acc, idx, k, k0, k1, e);
    else if (k < k1)
      acc = qf_fold_group<SEL, false>(W, stride, c, x, acc, idx, k, k0, k1, e);
#pragma unroll
    for (int u = 0; u < 8; ++u) e[u] = live ? e[u] : 0.f;
    const float tot = qf_reduce8<LANES>(e, lane);
    const int gj = g % GW;
    keep = j == gj ? tot : keep;
    if (gj == GW - 1 || g == groups - 1) {     // (the same for every lane of the wave)
      const int row = k0 + 8 * (g - gj + j) + r;
      if (j <= gj && row < k1) col[row] = keep;
    }
  }
  return acc;
}

// two-stage form, stage 1 (fold_chunk_kernel's geometry): chunk blockIdx.y folds k in
// [y * per, min(M, y * per + per)) into partial y; FINAL (one chunk): straight into S.  Column of
// the table: 4 * blockIdx.x + wave.
template <bool SEL, bool FINAL>
__global__ __launch_bounds__(256) void aggregate_qffl_kernel(const float* __restrict__ W, int64_t stride, QfCoef c,
                                                            int M, int64_t len4, int per_chunk, int groups,
                                                            const float* __restrict__ W_g, float* __restrict__ out,
                                                            float* __restrict__ nt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < len4;
  const int64_t ic = live ? i : len4 - 1;
  const int ch = blockIdx.y;
  const int k0 = ch * per_chunk;
  const int k1 = min(M, k0 + per_chunk);
  const float4 x = ld4(W_g + 4 * ic);
  float* col = nt + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * M;
  const float4 acc = qf_fold_range<SEL, 64>(W + 4 * ic, stride, c, x, k0, k1, groups, live, col);
  if (live) st4(out + (FINAL ? 0 : (int64_t)ch * 4 * len4) + 4 * i, acc);
}

// one-launch form (fold_one_kernel's geometry): SUB consecutive ranges of k per float4
// position folded by SUB threads of one workgroup, their partials folded in order in LDS; the
// deferred evaluation's finaliser rides as the last workgroup.  Column of the table:
// blockIdx.x * (POS / LANES) + the segment's place among the sub-range's positions.
template <bool SEL, int SUB>
__global__ __launch_bounds__(256) void aggregate_qffl_one_kernel(const float* __restrict__ W, int64_t stride, QfCoef c,
                                                                int M, int64_t len4, int per, int groups,
                                                                const float* __restrict__ W_g, float* __restrict__ S,
                                                                float* __restrict__ nt, EvalFinalize fin) {
  constexpr int POS = 256 / SUB;
  constexpr int LANES = POS < 64 ? POS : 64;
  __shared__ float4 sums[SUB][POS];
  if (fin.part && blockIdx.x == gridDim.x - 1) {
    eval_finalize_block(fin.part, fin.nb, fin.n, fin.out, reinterpret_cast<double(*)[256]>(&sums[0][0]));
    return;
  }
  static_assert(sizeof(sums) >= 2 * 256 * sizeof(double), "the finaliser reuses the partials' LDS");
  const int sub = threadIdx.x / POS, pl = threadIdx.x % POS;
  const int64_t i = (int64_t)blockIdx.x * POS + pl;
  const bool live = i < len4;
  const int64_t ic = live ? i : len4 - 1;
  const int k0 = sub * per, k1 = min(M, k0 + per);
  const float4 x = ld4(W_g + 4 * ic);
  float* col = nt + ((int64_t)blockIdx.x * (POS / LANES) + pl / LANES) * M;
  const float4 acc = qf_fold_range<SEL, LANES>(W + 4 * ic, stride, c, x, k0, k1, groups, live, col);
  sums[sub][pl] = acc;
  __syncthreads();
  if (sub == 0 && live) {
    float4 t = sums[0][pl];
    for (int s2 = 1; s2 < SUB && s2 * per < M; ++s2) t = add4(t, sums[s2][pl]);
    st4(S + 4 * i, t);
  }
}

// n[k] = the sum of row k's `cols` wave shares, in double: one workgroup per row (the table is a
// few loads per thread then, whatever M), thread t the columns t, t + 256, ... in order, then the
// 256 sums by the halving tree -- a fixed order
__global__ __launch_bounds__(256) void qffl_norms_kernel(const float* __restrict__ nt, int64_t cols, int M,
                                                        double* __restrict__ n) {
  __shared__ double sums[256];
  const int k = blockIdx.x;
  double acc = 0.0;
  for (int64_t cidx = threadIdx.x; cidx < cols; cidx += 256) acc += (double)nt[cidx * M + k];
  sums[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sums[threadIdx.x] += sums[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) n[k] = sums[0];
}

// The finish.  Every workgroup: U = sum_k (double)u_k and G = sum_k (double)g_k * n_k, k ascending
// (the terms staged in LDS 256 at a time, one thread adding them in order), H = Lc * U + G,
// coef = (float)(Lc / H) or 0; then x' = fl(x + fl(coef * S)) at its positions (coef = 0: nothing
// is written).  Workgroup 0 writes hc = {H, coef}.
__global__ __launch_bounds__(256) void qffl_step_kernel(const float* __restrict__ u, const float* __restrict__ g,
                                                       const double* __restrict__ n, double Lc, int M, int64_t len4,
                                                       const float* __restrict__ S, float* W_g,
                                                       double* __restrict__ hc) {
  __shared__ double st[2][256];     // the terms of U and of G, 256 at a time
  __shared__ double sG;
  __shared__ float scoef;
  // the two chains of dependent double adds run side by side, U's in wave 0 and G's in wave 1,
  // each one thread, the operands of 8 steps read ahead of them
  // (the next 256 terms are loaded while the chains run: the barriers wait for LDS only)
  const int chain = threadIdx.x >> 6;
  double acc = 0.0;
  double tu = (int)threadIdx.x < M ? (double)u[threadIdx.x] : 0.0;
  double tg = (int)threadIdx.x < M ? (double)g[threadIdx.x] * n[threadIdx.x] : 0.0;
  for (int base = 0; base < M; base += 256) {
    st[0][threadIdx.x] = tu;
    st[1][threadIdx.x] = tg;
    const int k = base + 256 + threadIdx.x;
    tu = k < M ? (double)u[k] : 0.0;
    tg = k < M ? (double)g[k] * n[k] : 0.0;
    lds_barrier();
    if ((threadIdx.x & 63) == 0 && chain < 2) {
      // 32 terms per LDS round trip.  The tile's tail past M holds +0.0, and acc + 0.0 is acc bit for
      // bit (acc starts at +0.0 and a sum that started there is never -0.0), so whole batches run.
      const double* t = st[chain];
      const int cnt = min(256, M - base);
      for (int j = 0; j < cnt; j += 32) {
        double a[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) a[i] = t[j + i];
#pragma unroll
        for (int i = 0; i < 32; ++i) acc += a[i];
      }
    }
    lds_barrier();
  }
  if (threadIdx.x == 64) sG = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double U = acc, G = sG;
    const double H = Lc * U + G;
    const bool ok = H > 0.0 && H <= 1.7976931348623157e308;   // finite and positive (a NaN fails both)
    const float coef = ok ? (float)(Lc / H) : 0.f;
    scoef = coef;
    if (blockIdx.x == 0) {
      hc[0] = H;
      hc[1] = (double)coef;
    }
  }
  __syncthreads();
  const float coef = scoef;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (coef == 0.f || i >= len4) return;
  const float4 s = ld4(S + 4 * i);
  const float4 x = ld4(W_g + 4 * i);
  st4(W_g + 4 * i, make_float4(x.x + coef * s.x, x.y + coef * s.y, x.z + coef * s.z, x.w + coef * s.w));
}

// columns of the partial table in the one-launch form at SUB sub-ranges / in the two-stage form
static int64_t qf_cols_one(int sub, int64_t len4) {
  const int pos = 256 / sub;
  return (len4 + pos - 1) / pos * std::max(1, pos / 64);
}
static int64_t qf_cols_chunked(int64_t len4) { return (len4 + 255) / 256 * 4; }

// doubles of d_nws (it holds floats: the table [columns][M]), the larger of the two forms'
int64_t aggregate_qffl_ws_doubles(int M, int64_t len) {
  if (M < 1 || len < 4) return 0;
  const int64_t len4 = len / 4;
  int64_t cols = qf_cols_chunked(len4);
  if (M <= AG_ONE_MAX_N) cols = std::max(cols, qf_cols_one(one_launch_sub(M), len4));
  return (cols * M + 1) / 2;
}

// the largest of them over 1 <= M <= N (a plan's subset rounds may fold any M): within a regime
// the table grows with M, so the regimes' last M and N itself
int64_t aggregate_qffl_ws_doubles_upto(int N, int64_t len) {
  int64_t need = aggregate_qffl_ws_doubles(N, len);
  for (int m : {15, 23, 47, 95, 191, AG_ONE_MAX_N})
    if (m < N) need = std::max(need, aggregate_qffl_ws_doubles(m, len));
  return need;
}

template <bool SEL, int SUB>
static void launch_qffl_one(const float* W, int64_t stride, const QfCoef& c, int M, int64_t len4, const float* W_g,
                            float* S, float* nt, const EvalFinalize& fin, hipStream_t st) {
  constexpr int POS = 256 / SUB;
  const int per = (M + SUB - 1) / SUB;
  const int64_t blocks = (len4 + POS - 1) / POS + (fin.part ? 1 : 0);
  hipLaunchKernelGGL((aggregate_qffl_one_kernel<SEL, SUB>), dim3((unsigned)blocks), dim3(256), 0, st, W, stride, c, M,
                     len4, per, (per + 7) / 8, W_g, S, nt, fin);
}

// the pass: S, and the table (its column count in *cols)
template <bool SEL>
static int qffl_pass_sel(const float* W, int64_t stride, const QfCoef& c, int M, int64_t len, const float* W_g, float* S,
                         float* nt, int64_t* cols, float* d_ws, int64_t ws_floats, int chunks, const EvalFinalize* fin,
                         hipStream_t st) {
  const int64_t len4 = len / 4;
  const EvalFinalize none{nullptr, 0, 0, nullptr};
  if (chunks <= 0 && M <= AG_ONE_MAX_N) {
    const EvalFinalize& f = fin ? *fin : none;
    const int sub = one_launch_sub(M);
    *cols = qf_cols_one(sub, len4);
    switch (sub) {
      case 1: launch_qffl_one<SEL, 1>(W, stride, c, M, len4, W_g, S, nt, f, st); break;
      case 2: launch_qffl_one<SEL, 2>(W, stride, c, M, len4, W_g, S, nt, f, st); break;
      case 4: launch_qffl_one<SEL, 4>(W, stride, c, M, len4, W_g, S, nt, f, st); break;
      case 8: launch_qffl_one<SEL, 8>(W, stride, c, M, len4, W_g, S, nt, f, st); break;
      case 16: launch_qffl_one<SEL, 16>(W, stride, c, M, len4, W_g, S, nt, f, st); break;
      default: launch_qffl_one<SEL, 32>(W, stride, c, M, len4, W_g, S, nt, f, st); break;
    }
    FS_LAUNCH_CHECK();
    return FS_OK;
  }
  if (fin) {
    const int rc = eval_finalize_launch(fin->part, fin->nb, fin->n, fin->out, st);
    if (rc != FS_OK) return rc;
  }
  const int64_t bx = (len4 + 255) / 256;
  *cols = qf_cols_chunked(len4);
  int per = 0;
  chunks = aggregate_chunks(M, chunks, d_ws != nullptr, ws_floats, len, &per);
  const int groups = (per + 7) / 8;
  if (chunks == 1) {
    hipLaunchKernelGGL((aggregate_qffl_kernel<SEL, true>), dim3((unsigned)bx, 1), dim3(256), 0, st, W, stride, c, M, len4,
                       per, groups, W_g, S, nt);
  } else {
    hipLaunchKernelGGL((aggregate_qffl_kernel<SEL, false>), dim3((unsigned)bx, chunks), dim3(256), 0, st, W, stride, c, M,
                       len4, per, groups, W_g, d_ws, nt);
    fold_partials_launch(d_ws, chunks, len4, S, st);
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int aggregate_qffl_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_u,
                          const float* d_g, double Lc, int M, int64_t len, float* d_W_g, float* d_S, double* d_n,
                          double* d_hc, float* d_ws, int64_t ws_floats, int chunks, double* d_nws, int64_t nws_doubles,
                          const EvalFinalize* fin, hipStream_t st) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_u && d_g && d_W_g && d_S && d_n && d_hc && d_nws, "null pointer");
  FS_REQUIRE(Lc > 0.0 && Lc <= 1.7976931348623157e308, "Lc must be finite and > 0");
  FS_REQUIRE(nws_doubles >= aggregate_qffl_ws_doubles(M, len), "d_nws is too small (fs_aggregate_qffl_ws_doubles)");
  FS_REQUIRE(d_S != d_W_g, "d_S and d_W_g must be different buffers");
  const QfCoef c{d_sel, d_u};
  float* nt = reinterpret_cast<float*>(d_nws);
  int64_t cols = 0;
  const int rc = d_sel ? qffl_pass_sel<true>(d_W_all, stride, c, M, len, d_W_g, d_S, nt, &cols, d_ws, ws_floats, chunks,
                                             fin, st)
                       : qffl_pass_sel<false>(d_W_all, stride, c, M, len, d_W_g, d_S, nt, &cols, d_ws, ws_floats, chunks,
                                              fin, st);
  if (rc != FS_OK) return rc;
  const int64_t len4 = len / 4;
  hipLaunchKernelGGL(qffl_norms_kernel, dim3((unsigned)M), dim3(256), 0, st, nt, cols, M, d_n);
  hipLaunchKernelGGL(qffl_step_kernel, dim3((unsigned)((len4 + 255) / 256)), dim3(256), 0, st, d_u, d_g, d_n, Lc, M, len4,
                     d_S, d_W_g, d_hc);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// u_k = p_k Ft^q, g_k = p_k q Ft^(q-1) L^2 with Ft = F[row_k] + 1e-10, in double, rounded once
// (q = 0: u = p and g = 0 exactly, whatever the loss)
__global__ __launch_bounds__(256) void qffl_coef_kernel(const double* __restrict__ F2, const int32_t* __restrict__ sel,
                                                       const float* __restrict__ p, double q, double L, int M,
                                                       float* __restrict__ u, float* __restrict__ g) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= M) return;
  const float pk = p[k];
  if (q == 0.0) {
    u[k] = pk;
    g[k] = 0.f;
    return;
  }
  const int row = sel ? sel[k] : k;
  const double Ft = F2[2 * (int64_t)row] + 1e-10;
  u[k] = (float)((double)pk * pow(Ft, q));
  g[k] = (float)((double)pk * q * pow(Ft, q - 1.0) * (L * L));
}

}  // namespace fs

using namespace fs;

extern "C" int64_t fs_aggregate_qffl_ws_doubles(int M, int64_t len) { return aggregate_qffl_ws_doubles(M, len); }

extern "C" int fs_aggregate_qffl(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_u,
                                 const float* d_g, double Lc, int M, int64_t len, float* d_W_g, float* d_S, double* d_n,
                                 double* d_hc, float* d_ws, int64_t ws_floats, int chunks, double* d_nws,
                                 int64_t nws_doubles, void* stream) {
  return aggregate_qffl_launch(d_W_all, stride, d_sel, d_u, d_g, Lc, M, len, d_W_g, d_S, d_n, d_hc, d_ws, ws_floats,
                               chunks, d_nws, nws_doubles, nullptr, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_qffl_coef(const double* d_F2, const int32_t* d_sel, const float* d_p, double q, double L, int M,
                            float* d_u, float* d_g, void* stream) {
  FS_REQUIRE(d_F2 && d_p && d_u && d_g, "null pointer");
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(q >= 0.0 && q <= 1.7976931348623157e308, "q must be finite and >= 0");
  FS_REQUIRE(L > 0.0 && L <= 1.7976931348623157e308, "L must be finite and > 0");
  hipLaunchKernelGGL(qffl_coef_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     d_F2, d_sel, d_p, q, L, M, d_u, d_g);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

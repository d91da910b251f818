// fs_aggregate_rfa: RFA, the smoothed-Weiszfeld approximation of the geometric median (Pillutla,
// Kakade, Harchaoui, IEEE TSP 2022) of the M rows d_sel (NULL: rows 0..M-1) of d_W_all under the
// weights alpha.  An iteration is a distance pass and a weighted fold over the same M x len rows;
// fs_rfa_step does both from one HBM read.  The rule and every summation order: include/fedsim.h.
//
// Geometry of fs_rfa_step (aggregate_robust.hip's).  A workgroup of 256 threads owns a stripe of W
// consecutive columns (W = 32: 128 B of every row; 16 and 8 for the M that no longer fit 32
// columns into the CU's 160 KiB).  It
//   1. stages the stripe of all M rows into LDS as floats, column-major with the odd pitch M | 1:
//      one float4 load per row element, 8 row loads in flight per thread, the sel ids of the next
//      group of 8 loaded before this group's rows are waited for, no load under a condition (row
//      and column are clamped; the LDS write and the stores are what the conditions guard);
//   2. folds v' on its stripe from LDS: the T = 256 / W threads of a column each sum their
//      k-strided slice of (double)b_k * (double)W_k[c] in ascending k (b read from global memory,
//      16 weights one group ahead, the first group before the rows are staged: every thread of a
//      slice reads the same word; a row with b_k == 0 is never multiplied), the slices joined by the fixed pairwise tree, rounded once to float, kept in
//      LDS and stored.  Pass 0 (FOLD = false) and a step after "no finite row" load the stripe of
//      v instead;
//   3. walks the staged rows a second time, from LDS: thread tid takes the rows k = tid, tid + 256,
//      ..., sums (double)fl(W_k[c] - v'[c])^2 over the stripe's columns in ascending c (consecutive
//      lanes read consecutive LDS words, v'[c] is a broadcast) and writes part[stripe][k].
// fs_rfa_weights: rfa_reduce_kernel sums a row's column of the partial table (8 rows x 32 slices
// to a workgroup, ceil(M / 8) workgroups), rfa_weights_kernel (one workgroup) takes the distances,
// beta, B, b and the objective.  The launch boundary is the only global reduction: no global
// atomics, no cross-workgroup wait.  The deferred evaluation's finaliser rides as an extra last
// workgroup of the chain's last step, as on the folds.
#include <cmath>

#include "aggregate_sel.h"
#include "common.h"
#include "finalize.h"

namespace fs {

#pragma clang fp contract(off)

constexpr int RF_NT = 256;                                   // threads of a workgroup
constexpr int RF_LDS = 160 * 1024;                           // the CU's LDS
constexpr int RF_AUX = 2304;                                 // bytes: the fold's slices [T][W] doubles (2048), then v' [32] floats
constexpr int RF_VOFF = 2048;                                // byte offset of v' in the aux region
constexpr int RF_VALS = (RF_LDS - RF_AUX) / 4;               // floats a workgroup can stage
constexpr int RF_GRP = 8;                                    // loads in flight per thread
constexpr int RF_BG = 16;                                    // weights a fold thread loads one group ahead
constexpr int RF_RR = 8;                                     // rfa_reduce_kernel: rows of a workgroup
constexpr int RF_RS = RF_NT / RF_RR;                         // ... and slices of a row's column

static_assert(RF_AUX >= RF_VOFF + 32 * 4 && RF_AUX % 16 == 0, "the aux region holds the slices and v'");

__host__ __device__ constexpr int rf_pitch(int M) { return M | 1; }
// the largest M at W columns: W * (M | 1) <= RF_VALS
constexpr int rf_max_m(int W) { return ((RF_VALS / W) & 1) ? RF_VALS / W : RF_VALS / W - 1; }
constexpr int RF_MAX_M32 = rf_max_m(32), RF_MAX_M16 = rf_max_m(16), RF_MAX_M8 = rf_max_m(8);
static_assert(RF_MAX_M32 >= 1250 && RF_MAX_M8 >= 5047, "the widths' ranges");

static int rf_width(int M) { return M <= RF_MAX_M32 ? 32 : M <= RF_MAX_M16 ? 16 : 8; }

template <int W, bool SEL, bool FOLD>
__global__ __launch_bounds__(RF_NT) void rfa_step_kernel(const float* __restrict__ Wall, int64_t stride,
                                                         const int32_t* __restrict__ sel, int M, int64_t len4,
                                                         const float* vin, const float* __restrict__ b,
                                                         const int32_t* __restrict__ flag, float* vout,
                                                         double* __restrict__ part, EvalFinalize fin) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rf_lds[];
  if (fin.part && blockIdx.x == gridDim.x - 1) {
    eval_finalize_block(fin.part, fin.nb, fin.n, fin.out, reinterpret_cast<double(*)[256]>(rf_lds));
    return;
  }
  constexpr int T = RF_NT / W;          // threads (slices) per column
  constexpr int Q4 = W / 4;             // float4 per row of the stripe
  constexpr int RP = RF_NT / Q4;        // rows a workgroup loads at once
  double* slice = reinterpret_cast<double*>(rf_lds);                 // [T][W]
  float* vs = reinterpret_cast<float*>(rf_lds + RF_VOFF / 4);       // [W]: the stripe of v'
  float* vals = reinterpret_cast<float*>(rf_lds + RF_AUX / 4);      // [W][pitch]
  const int pitch = rf_pitch(M);
  const int tid = threadIdx.x;

  // the fold's first group of weights, issued before the rows: every later group is loaded while
  // the one before it is consumed, so the fold never waits a global latency per 8 rows
  float bn[RF_BG];
  if (FOLD) {
#pragma unroll
    for (int u = 0; u < RF_BG; ++u) bn[u] = b[min(tid / W + u * T, M - 1)];
  }

  // ---- 1. stage ----
  {
    const int q = tid % Q4, r = tid / Q4;
    int64_t c4 = (int64_t)blockIdx.x * Q4 + q;
    if (c4 >= len4) c4 = len4 - 1;      // a ragged last stripe: a valid column, never used
    const float* base = Wall + 4 * c4;
    float* kq = vals + (4 * q) * pitch;
    int row[RF_GRP];
#pragma unroll
    for (int u = 0; u < RF_GRP; ++u) {
      const int k = min(u * RP + r, M - 1);
      row[u] = SEL ? sel[k] : k;
    }
    for (int k0 = 0; k0 < M; k0 += RF_GRP * RP) {
      float4 v[RF_GRP];
#pragma unroll
      for (int u = 0; u < RF_GRP; ++u) v[u] = ld4(base + (int64_t)row[u] * stride);
#pragma unroll
      for (int u = 0; u < RF_GRP; ++u) {
        const int k = min(k0 + RF_GRP * RP + u * RP + r, M - 1);
        row[u] = SEL ? sel[k] : k;
      }
#pragma unroll
      for (int u = 0; u < RF_GRP; ++u) {
        const int k = k0 + u * RP + r;
        if (k < M) {
          kq[k] = v[u].x;
          kq[pitch + k] = v[u].y;
          kq[2 * pitch + k] = v[u].z;
          kq[3 * pitch + k] = v[u].w;
        }
      }
    }
  }
  const int64_t col0 = (int64_t)blockIdx.x * W;
  const int64_t left = 4 * len4 - col0;
  const int wv = left < W ? (int)left : W;          // the stripe's columns that exist
  __syncthreads();                                  // the staged rows

  // ---- 2. v' on the stripe ----
  const bool keep = FOLD ? flag[0] != 0 : true;     // no finite row was left: v' = v bit for bit
  if (keep) {
    if (tid < W) vs[tid] = vin[col0 + min(tid, wv - 1)];
  } else {
    const int c = tid % W, s = tid / W;
    const float* vc = vals + c * pitch;
    double acc = 0.0;
    for (int k0 = s; k0 < M; k0 += RF_BG * T) {
      float bb[RF_BG];
#pragma unroll
      for (int u = 0; u < RF_BG; ++u) bb[u] = bn[u];
#pragma unroll
      for (int u = 0; u < RF_BG; ++u) bn[u] = b[min(k0 + (RF_BG + u) * T, M - 1)];
#pragma unroll
      for (int u0 = 0; u0 < RF_BG; u0 += RF_GRP) {
        float w[RF_GRP];
#pragma unroll
        for (int u = 0; u < RF_GRP; ++u) w[u] = vc[min(k0 + (u0 + u) * T, M - 1)];
#pragma unroll
        for (int u = 0; u < RF_GRP; ++u) {
          const double t = bb[u0 + u] != 0.0f ? (double)bb[u0 + u] * (double)w[u] : 0.0;
          if (k0 + (u0 + u) * T < M) acc += t;
        }
      }
    }
    slice[s * W + c] = acc;
    __syncthreads();
    if (s == 0) {
      double p[T];
#pragma unroll
      for (int j = 0; j < T; ++j) p[j] = slice[j * W + c];
#pragma unroll
      for (int h = 1; h < T; h *= 2)
#pragma unroll
        for (int j = 0; j < T; j += 2 * h) p[j] += p[j + h];
      vs[c] = (float)p[0];
    }
  }
  __syncthreads();                                  // v' in LDS
  if (tid < wv) vout[col0 + tid] = vs[tid];

  // ---- 3. every row's squared distance to v' over the stripe ----
  float vr[W];
#pragma unroll
  for (int c = 0; c < W; ++c) vr[c] = vs[c];
  double* prow = part + (int64_t)blockIdx.x * M;
  for (int k = tid; k < M; k += RF_NT) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const float e = vals[c * pitch + k] - vr[c];
      const double e2 = (double)e * (double)e;
      if (c < wv) acc += e2;
    }
    prow[k] = acc;
  }
}

// d2[k] = the sum of row k's column of the partial table [S][M]: slice s takes the stripes s,
// s + 32, ... in ascending order, the 32 slices joined by the pairwise tree
__global__ __launch_bounds__(RF_NT) void rfa_reduce_kernel(const double* __restrict__ part, int M, int S,
                                                           double* __restrict__ d2) {
  __shared__ double p[RF_RS][RF_RR + 1];
  const int kk = threadIdx.x % RF_RR, s = threadIdx.x / RF_RR;
  const int k = blockIdx.x * RF_RR + kk;
  const double* col = part + min(k, M - 1);
  double acc = 0.0;
  for (int j0 = s; j0 < S; j0 += RF_GRP * RF_RS) {
    double v[RF_GRP];
#pragma unroll
    for (int u = 0; u < RF_GRP; ++u) v[u] = col[(int64_t)min(j0 + u * RF_RS, S - 1) * M];
#pragma unroll
    for (int u = 0; u < RF_GRP; ++u)
      if (j0 + u * RF_RS < S) acc += v[u];
  }
  p[s][kk] = acc;
  __syncthreads();
  for (int h = 1; h < RF_RS; h *= 2) {
    if (s % (2 * h) == 0) p[s][kk] += p[s + h][kk];
    __syncthreads();
  }
  if (s == 0 && k < M) d2[k] = p[0][kk];
}

// the pairwise tree over a workgroup's 256 slices (every thread returns the total)
__device__ __forceinline__ double rf_tree(double v, double* p) {
  const int tid = threadIdx.x;
  __syncthreads();                                  // p is free again
  p[tid] = v;
  __syncthreads();
  for (int h = 1; h < RF_NT; h *= 2) {
    if (tid % (2 * h) == 0) p[tid] += p[tid + h];
    __syncthreads();
  }
  return p[0];
}

__device__ __forceinline__ double rf_beta(double d, float a, double nu, int mean) {
  if (!(fabs(d) < INFINITY)) return 0.0;            // NaN or Inf: the row is left out
  return mean ? (double)a : (double)a / fmax(nu, d);
}

// one workgroup: d_k, beta_k, B, b_k, the objective and the "no finite row" flag from d2 [M]
__global__ __launch_bounds__(RF_NT) void rfa_weights_kernel(const double* __restrict__ d2, int M,
                                                            const float* __restrict__ alpha, float ualpha, double nu,
                                                            int mean, double* __restrict__ dist, float* __restrict__ b,
                                                            double* __restrict__ obj, int obj_clear,
                                                            int32_t* __restrict__ flag) {
  __shared__ double p[RF_NT];
  const int tid = threadIdx.x;
  double sb = 0.0, sg = 0.0, nf = 0.0;
  for (int k = tid; k < M; k += RF_NT) {
    const double d = sqrt(d2[k]);
    const float a = alpha ? alpha[k] : ualpha;
    const bool ok = fabs(d) < INFINITY;
    sb += rf_beta(d, a, nu, mean);
    const double h = d > nu ? d : d * d / (2.0 * nu) + nu / 2.0;
    const double g = (double)a * h;
    sg += ok ? g : 0.0;
    nf += ok ? 1.0 : 0.0;
    if (dist) dist[k] = d;
  }
  const double B = rf_tree(sb, p);
  const double G = rf_tree(sg, p);
  const double NF = rf_tree(nf, p);
  const bool good = B > 0.0 && B < INFINITY;
  if (b)
    for (int k = tid; k < M; k += RF_NT) {
      const float a = alpha ? alpha[k] : ualpha;
      b[k] = good ? (float)(rf_beta(sqrt(d2[k]), a, nu, mean) / B) : 0.0f;
    }
  if (tid == 0) {
    obj[0] = NF > 0.0 ? G : (double)NAN;
    if (flag) flag[0] = good ? 0 : 1;
  }
  for (int i = 1 + tid; i <= obj_clear; i += RF_NT) obj[i] = (double)NAN;
}

// dynamic LDS beyond the 64 KB a kernel gets unasked (set once per kernel, to the whole CU's)
template <int W, bool SEL, bool FOLD>
static int rf_launch(const float* Wall, int64_t stride, const int32_t* sel, int M, int64_t len, const float* vin,
                     const float* b, const int32_t* flag, float* vout, double* part, const EvalFinalize& fin,
                     hipStream_t st) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&rfa_step_kernel<W, SEL, FOLD>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, RF_LDS);
  if (attr != hipSuccess) return fail(FS_EHIP, std::string("fs_rfa_step: ") + hipGetErrorString(attr));
  size_t lds = (size_t)RF_AUX + (size_t)W * rf_pitch(M) * 4;
  if (fin.part) lds = std::max(lds, (size_t)(2 * 256 * sizeof(double)));
  const int64_t blocks = (len + W - 1) / W + (fin.part ? 1 : 0);
  hipLaunchKernelGGL((rfa_step_kernel<W, SEL, FOLD>), dim3((unsigned)blocks), dim3(RF_NT), lds, st, Wall, stride, sel,
                     M, len / 4, vin, b, flag, vout, part, fin);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

template <int W>
static int rf_launch_w(const float* Wall, int64_t stride, const int32_t* sel, int M, int64_t len, const float* vin,
                       const float* b, const int32_t* flag, float* vout, double* part, const EvalFinalize& fin,
                       hipStream_t st) {
  if (sel) {
    if (b) return rf_launch<W, true, true>(Wall, stride, sel, M, len, vin, b, flag, vout, part, fin, st);
    return rf_launch<W, true, false>(Wall, stride, sel, M, len, vin, b, flag, vout, part, fin, st);
  }
  if (b) return rf_launch<W, false, true>(Wall, stride, sel, M, len, vin, b, flag, vout, part, fin, st);
  return rf_launch<W, false, false>(Wall, stride, sel, M, len, vin, b, flag, vout, part, fin, st);
}

static int rfa_check_rows(int M, int64_t len, int64_t stride) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(M <= RF_MAX_M8, "M is larger than fs_aggregate_rfa_max_m()");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  return FS_OK;
}

// one step (b == nullptr: pass 0, the distances to vin and a copy of it; no flag is read)
static int rfa_step_launch(const float* Wall, int64_t stride, const int32_t* sel, int M, int64_t len, const float* vin,
                           const float* b, const int32_t* flag, float* vout, double* part, const EvalFinalize& fin,
                           hipStream_t st) {
  const int W = rf_width(M);
  if (W == 32) return rf_launch_w<32>(Wall, stride, sel, M, len, vin, b, flag, vout, part, fin, st);
  if (W == 16) return rf_launch_w<16>(Wall, stride, sel, M, len, vin, b, flag, vout, part, fin, st);
  return rf_launch_w<8>(Wall, stride, sel, M, len, vin, b, flag, vout, part, fin, st);
}

static int64_t rf_stripes(int M, int64_t len) {
  const int W = rf_width(M);
  return (len + W - 1) / W;
}

static int rfa_weights_launch(const double* part, int M, int64_t len, const float* alpha, float ualpha, double nu,
                              int mean, double* d2, double* dist, float* b, double* obj, int obj_clear, int32_t* flag,
                              hipStream_t st) {
  if (part) {
    hipLaunchKernelGGL(rfa_reduce_kernel, dim3((unsigned)((M + RF_RR - 1) / RF_RR)), dim3(RF_NT), 0, st, part, M,
                       (int)rf_stripes(M, len), d2);
    FS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rfa_weights_kernel, dim3(1), dim3(RF_NT), 0, st, d2, M, alpha, ualpha, nu, mean, dist, b, obj,
                     obj_clear, flag);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

static int64_t rf_up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// the workspace: the partial table [stripes][M] doubles, d2 [M] doubles, two v buffers [len]
// floats, the flag -- every term grows with M (a wider M has no fewer stripes)
int64_t aggregate_rfa_ws_bytes(int M, int64_t len) {
  if (M < 1 || M > RF_MAX_M8 || len < 4) return 0;
  return rf_up16(rf_stripes(M, len) * M * 8) + rf_up16((int64_t)M * 8) + 2 * rf_up16(len * 4) + 16;
}

int aggregate_rfa_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                         const float* d_x, const float* d_alpha, float ualpha, int T, double nu, int init, float* d_out,
                         double* d_dist, float* d_b, double* d_obj, void* d_ws, int64_t ws_bytes,
                         const EvalFinalize* fin, hipStream_t st) {
  if (const int rc = rfa_check_rows(M, len, stride)) return rc;
  FS_REQUIRE(T >= 0 && T <= FS_RFA_MAX_ITERS, "T must be in [0, 32]");
  FS_REQUIRE(nu > 0.0 && std::isfinite(nu), "nu must be positive and finite");
  FS_REQUIRE(init == FS_RFA_INIT_START || init == FS_RFA_INIT_MEAN, "init must be FS_RFA_INIT_START or FS_RFA_INIT_MEAN");
  FS_REQUIRE(d_W_all && d_x && d_out && d_dist && d_b && d_obj && d_ws, "null pointer");
  FS_REQUIRE(ws_bytes >= aggregate_rfa_ws_bytes(M, len), "d_ws is too small (fs_aggregate_rfa_ws_bytes(M, len))");
  char* w = static_cast<char*>(d_ws);
  double* part = reinterpret_cast<double*>(w);
  w += rf_up16(rf_stripes(M, len) * M * 8);
  double* d2 = reinterpret_cast<double*>(w);
  w += rf_up16((int64_t)M * 8);
  float* V[2];
  V[0] = reinterpret_cast<float*>(w);
  w += rf_up16(len * 4);
  V[1] = reinterpret_cast<float*>(w);
  w += rf_up16(len * 4);
  int32_t* flag = reinterpret_cast<int32_t*>(w);
  const EvalFinalize none{nullptr, 0, 0, nullptr};
  const int mean = init == FS_RFA_INIT_MEAN ? 1 : 0;
  const int nfold = T + mean;
  // stage 0 is pass 0 (the distances to x), stage i >= 1 the i-th fused step; every stage's
  // distances give the next one's weights, the last stage's are the recorded ones
  for (int i = 0; i <= nfold; ++i) {
    const float* vin = i == 0 ? d_x : V[(i - 1) & 1];
    float* vout = i == nfold ? d_out : V[i & 1];
    const EvalFinalize& f = (i == nfold && fin) ? *fin : none;
    int rc = rfa_step_launch(d_W_all, stride, d_sel, M, len, vin, i == 0 ? nullptr : d_b, flag, vout, part, f, st);
    if (rc != FS_OK) return rc;
    // d_b keeps the last weights used: the last stage writes it only when no fold ran at all
    float* bout = (i < nfold || nfold == 0) ? d_b : nullptr;
    rc = rfa_weights_launch(part, M, len, d_alpha, ualpha, nu, (mean && i == 0) ? 1 : 0, d2, d_dist, bout, d_obj + i,
                            i == 0 ? T + 1 : 0, bout ? flag : nullptr, st);
    if (rc != FS_OK) return rc;
  }
  return FS_OK;
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_rfa_max_m(void) { return RF_MAX_M8; }

extern "C" int fs_rfa_width(int M) { return (M < 1 || M > RF_MAX_M8) ? 0 : rf_width(M); }

extern "C" int64_t fs_aggregate_rfa_ws_bytes(int M, int64_t len) { return aggregate_rfa_ws_bytes(M, len); }

extern "C" int fs_rfa_step(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                           const float* d_v, const float* d_b, const int32_t* d_flag, float* d_v_out, double* d_part,
                           void* stream) {
  if (const int rc = rfa_check_rows(M, len, stride)) return rc;
  FS_REQUIRE(d_W_all && d_v && d_v_out && d_part, "null pointer");
  FS_REQUIRE(!d_b == !d_flag, "d_b and d_flag come together (both NULL: pass 0)");
  const EvalFinalize none{nullptr, 0, 0, nullptr};
  return rfa_step_launch(d_W_all, stride, d_sel, M, len, d_v, d_b, d_flag, d_v_out, d_part, none,
                         reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_rfa_weights(const double* d_part, int M, int64_t len, const float* d_alpha, double nu, int mean,
                              double* d_d2, double* d_dist, float* d_b, double* d_obj, int32_t* d_flag, void* stream) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(M <= RF_MAX_M8, "M is larger than fs_aggregate_rfa_max_m()");
  FS_REQUIRE(len >= 4 && len % 4 == 0, "len must be a multiple of 4");
  FS_REQUIRE(nu > 0.0 && std::isfinite(nu), "nu must be positive and finite");
  FS_REQUIRE(mean == 0 || mean == 1, "mean must be 0 or 1");
  FS_REQUIRE(d_alpha && d_d2 && d_dist && d_b && d_obj && d_flag, "null pointer");
  return rfa_weights_launch(d_part, M, len, d_alpha, 0.0f, nu, mean, d_d2, d_dist, d_b, d_obj, 0, d_flag,
                            reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_aggregate_rfa(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                                const float* d_x, const float* d_alpha, int T, double nu, int init, float* d_out,
                                double* d_dist, float* d_b, double* d_obj, void* d_ws, int64_t ws_bytes, void* stream) {
  FS_REQUIRE(d_alpha, "null pointer");
  return aggregate_rfa_launch(d_W_all, stride, d_sel, M, len, d_x, d_alpha, 0.0f, T, nu, init, d_out, d_dist, d_b, d_obj,
                              d_ws, ws_bytes, nullptr, reinterpret_cast<hipStream_t>(stream));
}

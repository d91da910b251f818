// fs_eval_clients -- local evaluation: the test_loop metrics (tools.py:218-237) of a model on
// EVERY client's own training rows, one pass over the resident features (phi, CSR by client).
// The reference never computes them: its train_loop keeps a running train_acc.avg
// (tools.py:213-215) that every caller drops.  w_stride = 0 scores one model (the global one) on
// every client -- the per-client distribution and, n_j-weighted, the true objective F(W_g);
// w_stride = C * ld scores W_out[j] on client j (the local model on local data).
//
// Three launches on the caller's stream, no atomics, no cross-workgroup wait:
//   1. eval_clients_prefix  one workgroup: pre[j] = sum_{i<j} ceil(n_i / 16) from d_row_off, into
//                           the head of the workspace (int32 [N + 1])
//   2. eval_clients_kernel  one workgroup per 16-row group COUNTED FROM THE CLIENT'S FIRST ROW
//                           (client j owns groups pre[j] .. pre[j+1]-1; a workgroup finds its
//                           client by binary search in pre); the group body is eval_rows.h's
//                           eval_group16 -- fs_eval's -- on (phi + row_off[j] ld, labels +
//                           row_off[j], n_j, W + j w_stride); its fp64 pair to part[2 g]
//      (MSE: eval_mse_rows.h's eval_mse_group16, fs_eval_mse's body, 4 waves)
//   3. eval_clients_finalize  one 256-thread workgroup per client: finalize.h's
//                           eval_finalize_block over the client's partials, division by n_j
// So d_out[2j..2j+1] is bit for bit what fs_eval returns on client j's slice (contract A,
// include/fedsim.h), and depends on client j's rows and model alone.  HBM-bound like fs_eval: one
// read of the features; W (C ld floats) is re-read per group from L2.
#include "common.h"
#include "finalize.h"
#include "eval_rows.h"
#include "eval_mse_rows.h"

namespace fs {

constexpr int EC_WAVES = 8;        // = eval.hip's EV_WAVES: the same LDS fold order per row
constexpr int EC_MSE_WAVES = 4;    // = eval_mse.hip's EM_WAVES
constexpr int EC_ROWS = 16;
constexpr int EC_PRE_THREADS = 1024;

__device__ __forceinline__ int ec_groups(int64_t n) { return n > 0 ? (int)((n + EC_ROWS - 1) / EC_ROWS) : 0; }

// pre[j] = groups of the clients before j, pre[N] = all groups.  Thread t owns the K = ceil(N /
// 1024) consecutive clients from t K; their counts are scanned over the threads through LDS.
__global__ __launch_bounds__(EC_PRE_THREADS) void eval_clients_prefix(const int64_t* __restrict__ row_off, int N,
                                                                      int32_t* __restrict__ pre) {
  __shared__ int32_t s[EC_PRE_THREADS];
  const int t = threadIdx.x;
  const int K = (N + EC_PRE_THREADS - 1) / EC_PRE_THREADS;
  const int j0 = min(t * K, N), j1 = min(j0 + K, N);
  int32_t own = 0;
  for (int j = j0; j < j1; ++j) own += ec_groups(row_off[j + 1] - row_off[j]);
  s[t] = own;
  __syncthreads();
  for (int h = 1; h < EC_PRE_THREADS; h <<= 1) {      // inclusive scan (Hillis-Steele)
    const int32_t v = t >= h ? s[t - h] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  int32_t run = s[t] - own;
  for (int j = j0; j < j1; ++j) {
    pre[j] = run;
    run += ec_groups(row_off[j + 1] - row_off[j]);
  }
  if (t == EC_PRE_THREADS - 1) pre[N] = s[t];
}

// the client that owns group g: the largest j with pre[j] <= g (clients have >= 1 group each)
__device__ __forceinline__ int ec_find_client(const int32_t* __restrict__ pre, int N, int g) {
  int lo = 0, hi = N;                                  // pre[lo] <= g < pre[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

template <int CT>
__global__ __launch_bounds__(EC_WAVES * 64) void eval_clients_kernel(const float* __restrict__ phi, int64_t ld,
                                                                     const int64_t* __restrict__ row_off,
                                                                     const int32_t* __restrict__ y, int N,
                                                                     const float* __restrict__ W, int64_t w_stride,
                                                                     int C, const int32_t* __restrict__ pre,
                                                                     double* __restrict__ part) {
  __shared__ float zt[EC_WAVES * 16 * (CT * 16 + 1)];
  const int g = (int)blockIdx.x;
  if (g >= pre[N]) return;                             // (the host count and d_row_off disagree: no work)
  const int j = ec_find_client(pre, N, g);
  const int64_t r0 = row_off[j];
  const int n = (int)(row_off[j + 1] - r0);
  double ce = 0.0, cor = 0.0;
  eval_group16<EC_WAVES, CT>(phi + r0 * ld, ld, y + r0, n, W + (int64_t)j * w_stride, C, (g - pre[j]) * EC_ROWS, zt,
                             ce, cor);
  if ((threadIdx.x >> 6) == 0) {
    ce = wave_sum(ce);
    cor = wave_sum(cor);
    if ((threadIdx.x & 63) == 0) {
      part[2 * (int64_t)g] = ce;
      part[2 * (int64_t)g + 1] = cor;
    }
  }
}

__global__ __launch_bounds__(EC_MSE_WAVES * 64) void eval_clients_mse_kernel(const float* __restrict__ phi,
                                                                             int64_t ld,
                                                                             const int64_t* __restrict__ row_off,
                                                                             const float* __restrict__ y, int N,
                                                                             const float* __restrict__ W,
                                                                             int64_t w_stride,
                                                                             const int32_t* __restrict__ pre,
                                                                             double* __restrict__ part) {
  __shared__ double s[2][EC_MSE_WAVES];
  const int g = (int)blockIdx.x;
  if (g >= pre[N]) return;
  const int j = ec_find_client(pre, N, g);
  const int64_t r0 = row_off[j];
  const int n = (int)(row_off[j + 1] - r0);
  eval_mse_group16<EC_MSE_WAVES>(phi + r0 * ld, ld, y + r0, n, W + (int64_t)j * w_stride, (g - pre[j]) * EC_ROWS, s,
                                 part + 2 * (int64_t)g);
}

// client blockIdx.x: fs_eval's fold (finalize.h) of its partials, clamped to the G groups launched
__global__ __launch_bounds__(256) void eval_clients_finalize(const double* __restrict__ part,
                                                            const int32_t* __restrict__ pre,
                                                            const int64_t* __restrict__ row_off, int G,
                                                            double* __restrict__ out) {
  __shared__ double s[2][256];
  const int j = (int)blockIdx.x;
  const int lo = min(pre[j], G), hi = min(pre[j + 1], G);
  eval_finalize_block(part + 2 * (int64_t)lo, hi - lo, (int)(row_off[j + 1] - row_off[j]), out + 2 * (int64_t)j, s);
}

static int64_t eval_clients_ws_doubles(int64_t total_rows, int N) {
  return ((int64_t)N + 2) / 2 + 2 * (total_rows / EC_ROWS + N);
}

static int eval_clients(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int64_t* h_n,
                        const void* d_tgt, int N, const float* d_W, int64_t w_stride, int C, bool mse, double* d_out,
                        double* d_ws, int64_t ws_doubles, hipStream_t st) {
  FS_REQUIRE(N >= 1, "N must be >= 1");
  FS_REQUIRE(C >= 1 && C <= 32, "num_classes must be in [1, 32]");
  FS_REQUIRE(ld >= 64 && ld % 64 == 0, "ld must be a positive multiple of 64");
  FS_REQUIRE(d_phi && d_row_off && h_n && d_tgt && d_W && d_out && d_ws, "null pointer");
  FS_REQUIRE(w_stride >= 0 && w_stride % 4 == 0, "w_stride must be a non-negative multiple of 4 floats");
  int64_t rows = 0, groups = 0;
  for (int j = 0; j < N; ++j) {
    FS_REQUIRE(h_n[j] >= 1, "every client needs n_j >= 1");
    FS_REQUIRE(h_n[j] <= INT32_MAX, "a client has more than 2^31 - 1 rows");
    rows += h_n[j];
    groups += (h_n[j] + EC_ROWS - 1) / EC_ROWS;
  }
  if (groups > INT32_MAX) return fail(FS_EUNSUPPORTED, std::string(__func__) + ": more than 2^31 - 1 row groups");
  FS_REQUIRE(ws_doubles >= eval_clients_ws_doubles(rows, N), "workspace too small (fs_eval_clients_ws_doubles)");
  int32_t* pre = reinterpret_cast<int32_t*>(d_ws);
  double* part = d_ws + ((int64_t)N + 2) / 2;
  const int G = (int)groups;
  hipLaunchKernelGGL(eval_clients_prefix, dim3(1), dim3(EC_PRE_THREADS), 0, st, d_row_off, N, pre);
  if (mse)
    hipLaunchKernelGGL(eval_clients_mse_kernel, dim3(G), dim3(EC_MSE_WAVES * 64), 0, st, d_phi, ld, d_row_off,
                       static_cast<const float*>(d_tgt), N, d_W, w_stride, pre, part);
  else if (C <= 16)
    hipLaunchKernelGGL((eval_clients_kernel<1>), dim3(G), dim3(EC_WAVES * 64), 0, st, d_phi, ld, d_row_off,
                       static_cast<const int32_t*>(d_tgt), N, d_W, w_stride, C, pre, part);
  else
    hipLaunchKernelGGL((eval_clients_kernel<2>), dim3(G), dim3(EC_WAVES * 64), 0, st, d_phi, ld, d_row_off,
                       static_cast<const int32_t*>(d_tgt), N, d_W, w_stride, C, pre, part);
  hipLaunchKernelGGL(eval_clients_finalize, dim3(N), dim3(256), 0, st, part, pre, d_row_off, G, d_out);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace fs

extern "C" int64_t fs_eval_clients_ws_doubles(int64_t total_rows, int N) {
  return (total_rows < 1 || N < 1) ? 0 : fs::eval_clients_ws_doubles(total_rows, N);
}

extern "C" int fs_eval_clients(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int64_t* h_n,
                               const int32_t* d_labels, int N, const float* d_W, int64_t w_stride, int C,
                               double* d_out, double* d_ws, int64_t ws_doubles, void* stream) {
  return fs::eval_clients(d_phi, ld, d_row_off, h_n, d_labels, N, d_W, w_stride, C, false, d_out, d_ws, ws_doubles,
                          reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_eval_clients_mse(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int64_t* h_n,
                                   const float* d_y, int N, const float* d_W, int64_t w_stride, double* d_out,
                                   double* d_ws, int64_t ws_doubles, void* stream) {
  return fs::eval_clients(d_phi, ld, d_row_off, h_n, d_y, N, d_W, w_stride, 1, true, d_out, d_ws, ws_doubles,
                          reinterpret_cast<hipStream_t>(stream));
}

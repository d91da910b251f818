// fs_eval_mse -- test-set mean squared error of the one-column global model, and the
// reference's degenerate "accuracy" at one output.
//
// Replaces test_loop + comp_accuracy + Meter (the reference's functions/tools.py:218-237,
// 82-96, 99-148) under nn.MSELoss (tools.py:223-224).  The reference averages per-batch means
// weighted by batch size, which equals the plain mean over all rows up to fp32 rounding; the
// shuffle only matters for the RNG stream, which the host replays.  comp_accuracy takes the
// top-1 index of a one-column output -- always 0 -- and compares it with the float target, so
// the "accuracy" is 100 * #{y == 0} / n whatever the model says; reproduced as is.
//
// One 4-wave workgroup per 16 rows (the partial layout and the workspace size of fs_eval:
// fs_eval_ws_doubles(n)), one wave per row at a time: 16-byte loads, a wave reads contiguous
// bytes of the row, w from L2.  Per-block fp64 partials, folded by fs_eval's one-block
// finaliser in a fixed order (bitwise reproducible).  HBM-bound: one read of the test features.
#include "common.h"
#include "finalize.h"
#include "mse_rows.h"

namespace fs {

constexpr int EM_WAVES = 4;
constexpr int EM_ROWS = 16;   // rows per workgroup (= eval.hip's EV_ROWS: fs_eval_ws_doubles covers it)

__global__ __launch_bounds__(EM_WAVES * 64) void eval_mse_kernel(const float* __restrict__ phi, int64_t ld,
                                                                 const float* __restrict__ y, int n,
                                                                 const float* __restrict__ W,
                                                                 double* __restrict__ part) {
  __shared__ double s[2][EM_WAVES];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  double sq = 0.0, zc = 0.0;
  for (int r = w; r < EM_ROWS; r += EM_WAVES) {
    const int row = (int)blockIdx.x * EM_ROWS + r;
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
    for (int i = 0; i < EM_WAVES; ++i) {
      a += s[0][i];
      b += s[1][i];
    }
    part[2 * blockIdx.x] = a;
    part[2 * blockIdx.x + 1] = b;
  }
}

int eval_mse(const float* d_phi, int64_t ld, const float* d_y, int n, const float* d_W, double* d_out,
             double* d_ws, hipStream_t st) {
  FS_REQUIRE(n >= 1, "n must be >= 1");
  FS_REQUIRE(ld >= 64 && ld % 64 == 0, "ld must be a positive multiple of 64");
  FS_REQUIRE(d_phi && d_y && d_W && d_out && d_ws, "null pointer");
  const int nb = (n + EM_ROWS - 1) / EM_ROWS;
  hipLaunchKernelGGL(eval_mse_kernel, dim3(nb), dim3(EM_WAVES * 64), 0, st, d_phi, ld, d_y, n, d_W, d_ws);
  FS_LAUNCH_CHECK();
  return eval_finalize_launch(d_ws, nb, n, d_out, st);
}

}  // namespace fs

extern "C" int fs_eval_mse(const float* d_phi, int64_t ld, const float* d_y, int n, const float* d_W,
                           double* d_out, double* d_ws, void* stream) {
  return fs::eval_mse(d_phi, ld, d_y, n, d_W, d_out, d_ws, reinterpret_cast<hipStream_t>(stream));
}

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
// One 4-wave workgroup per 16 rows (eval_mse_rows.h's body, which fs_eval_clients_mse shares; the
// partial layout and the workspace size of fs_eval: fs_eval_ws_doubles(n)), one wave per row at a time: 16-byte loads, a wave reads contiguous
// bytes of the row, w from L2.  Per-block fp64 partials, folded by fs_eval's one-block
// finaliser in a fixed order (bitwise reproducible).  HBM-bound: one read of the test features.
#include "common.h"
#include "finalize.h"
#include "eval_mse_rows.h"
#include "mse_rows.h"

namespace fs {

constexpr int EM_WAVES = 4;
constexpr int EM_ROWS = 16;   // rows per workgroup (= eval.hip's EV_ROWS: fs_eval_ws_doubles covers it)

__global__ __launch_bounds__(EM_WAVES * 64) void eval_mse_kernel(const float* __restrict__ phi, int64_t ld,
                                                                 const float* __restrict__ y, int n,
                                                                 const float* __restrict__ W,
                                                                 double* __restrict__ part) {
  __shared__ double s[2][EM_WAVES];
  eval_mse_group16<EM_WAVES>(phi, ld, y, n, W, (int)blockIdx.x * EM_ROWS, s, part + 2 * blockIdx.x);
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

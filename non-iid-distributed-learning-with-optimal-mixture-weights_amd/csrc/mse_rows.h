// Shared by the one-output-column (MSE) kernels: the host-side launchers round.hip calls, and
// the row helpers of local_train_mse.hip and mixture_mse.hip, which both compute |b| dots of
// gathered rows with a lane-owned vector.
#pragma once
#include "common.h"

namespace fs {

// the one-output-column (MSE) forms of fs_local_train / fs_eval with a HIP stream (round.hip calls them)
int local_train_mse(const float* d_phi, int64_t ld, const int64_t* d_row_off, const float* d_y,
                    const int32_t* d_perms, const int32_t* d_order, int N, int B, int E, float lr, float mu,
                    int prox, float lam, int reg, int chained, const float* d_W_start, float* d_W_out,
                    double* d_loss, hipStream_t st);
int eval_mse(const float* d_phi, int64_t ld, const float* d_y, int n, const float* d_W, double* d_out,
             double* d_ws, hipStream_t st);

// v[0..R) per lane -> the wave total of row (lane * R) >> 6, in a fixed order.  Stage k sends
// half of the rows to the lane 32 >> k away and keeps the other half: R + log2(64 / R) - 1
// shuffles for R rows instead of 6 R.
template <int R>
__device__ __forceinline__ float reduce_rows(float (&v)[R], int lane) {
  int off = 32;
#pragma unroll
  for (int n = R; n > 1; n >>= 1) {
    const int h = n >> 1;
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const float send = up ? v[i] : v[i + h];
      const float keep = up ? v[i + h] : v[i];
      v[i] = keep + __shfl_xor(send, off, 64);
    }
    off >>= 1;
  }
  float r = v[0];
#pragma unroll
  for (; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
  return r;
}

__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}

__device__ __forceinline__ float4 fma4(float s, float4 a, float4 acc) {
  return make_float4(fmaf(s, a.x, acc.x), fmaf(s, a.y, acc.y), fmaf(s, a.z, acc.z), fmaf(s, a.w, acc.w));
}

// lane `idx` (wave-uniform) of v
__device__ __forceinline__ float lane_value(float v, int idx) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), idx));
}

}  // namespace fs

// What the SCAFFOLD kernels (local_train_scaffold.hip, aggregate_scaffold.hip) share with their
// host side (local_train_host.cpp) and with the round plan (round.hip).  No device code here, and
// no existing kernel includes it.
#pragma once

#include "common.h"

namespace fs {

// fs_local_train_scaffold's parameters: LTParams without the prox term, the chained mode and the
// fused evaluation, with the two variates
struct LTSParams {
  const float* phi;
  int64_t ld;
  const int64_t* row_off;
  const int32_t* labels;
  const int32_t* perms;
  const int32_t* order;
  int N, C, B, E;
  float lr, lam;
  int reg;
  const float* W_start;
  const float* c;       // [C][ld] server variate (read only)
  float* ci;            // [clients][C][ld] client variates, by client id, updated in place
  float* W_out;
  double* loss;
};

// local_train_scaffold.hip: the instance for (B, C) on P.N workgroups
int launch_local_train_scaffold(const LTSParams& P, hipStream_t st);

// fs_local_train_scaffold behind its validation (local_train_host.cpp)
int local_train_scaffold(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int32_t* d_labels,
                         const int32_t* d_perms, const int32_t* d_order, int N, int C, int B, int E, float lr,
                         float lam, int reg, const float* d_W_start, const float* d_c, float* d_ci, float* d_W_out,
                         double* d_loss, hipStream_t st);

// fs_aggregate_scaffold (aggregate_scaffold.hip)
int aggregate_scaffold_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                              const float* d_r, float cs, int M, int64_t len, float* d_W_g, float* d_c, float* d_ws,
                              int64_t ws_floats, int chunks, hipStream_t st);

}  // namespace fs

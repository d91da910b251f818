// What the p-solver kernels (mixture.hip) share with their host side, mixture_host.cpp: the
// constants both the kernels and the planner read, the plan, and one launch entry point per
// solver.  No device code here.
// Which solver a shape gets, the exchange workspace, the helpers and every measured tuning
// policy live in mixture_host.cpp, which no kernel revision (_lib.source_revision) covers.
#pragma once

#include "common.h"

namespace fs {

// client stride of a Z row segment: N rounded up to 4 (16-byte aligned class segments)
__host__ __device__ __forceinline__ int mix_ldn(int N) { return (N + 3) & ~3; }

// global / staged: one workgroup of 1024 threads
constexpr int MS_THREADS = 1024;
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int MS_MAXB = 64;
constexpr int MS2_PER_THREAD = 4;     // float4 of staged rows per thread (one batch <= 64 KB)
constexpr int MS2_NK = 4;             // clients per lane (N <= 256 on this path)
// reg / reg2: waves, one / two batch rows each
constexpr int MR_WAVES = 16;
constexpr int M2_WAVES = 8;
// quad, quadl and qmc: waves of 4 batch rows
constexpr int MQ_WAVES = 4;
// mc and qmc: the exchange
constexpr int MC_THREADS = 256;
constexpr int MC_XCDS = 8;
constexpr int MC_KMAX = 32;
constexpr int MC_SLOT = 256;                     // granules per workgroup per parity
constexpr int MC_TOT = 256;                      // hop-2 granules (logit totals) per parity
constexpr unsigned MC_SPIN_LIMIT = 1u << 20;
constexpr int QMC_KMAX = 16;
// caller-owned workspace of the multi-CU solvers: [2][K][MC_SLOT] exchange granules (zeroed
// before every launch) followed by a 256-byte error block (sticky: only the caller clears it;
// the helpers' progress word is its byte 128)
constexpr int64_t MC_ERR_BYTES = 256;

// the thirteen values every solver takes, and where fs_mix_solve placed the caller's workspace
struct MixArgs {
  const float* Z;
  const int32_t* y;
  const int32_t* perms;
  int N, C, nv, epochs, Bv;
  float lr, mom;
  float* p;
  float* buf;
  int* first;
  unsigned long long* xbuf = nullptr;   // exchange granules (mc, qmc)
  unsigned* err = nullptr;              // error block (mc, qmc)
  unsigned* prog = nullptr;             // helpers' progress word (null: no helpers)
};

// bytes of Z (32-bit buffer offsets: mix_plan admits the solvers that use them only below 2^31)
inline int mix_z_bytes(const MixArgs& a) { return (int)((int64_t)a.nv * a.C * mix_ldn(a.N) * 4); }

// mix_plan's answer (mixture_host.cpp): the solver that launches and all its launch needs
// beyond MixArgs.  Fields a solver does not read are 0.
struct MixPlan {
  int solver = 0;            // FS_SOLVER_* (0: no solver fits the shape)
  int K = 0;                 // mc, qmc: workgroups
  int nk = 0;                // qmc: clients per lane (4 or 8)
  int S = 0, hops = 0;       // mc: clients per workgroup, exchange hops
  int zR = 1;                // qmc: rank blocks of Z (fs_mix_solve_blocked), else 1
  bool fast_softmax = false; // quad, bin: v_exp_f32 / v_rcp_f32 softmax
  bool loaders = false;      // quad: the loader-wave kernel
  int helpers = 0;           // L2 prefetch helper workgroups after the solver's own clamp
  int lead = 0;              // steps the helpers run ahead (0 without helpers)
  int poll_delay = 0;        // qmc: s_sleep(1) units before a step's first poll
  unsigned spin_limit = 0;   // mc, qmc: the exchange's spin bound
  size_t lds = 0;            // staged, global: dynamic LDS bytes
  int64_t ws_bytes = 0;      // workspace bytes the launch uses (exchange + error block)
};

// the solver fs_mix_solve launches for this shape under this tuning (pure; fs_mix_solve_plan
// reports it); blocks > 1: fs_mix_solve_blocked's rank-blocked Z
MixPlan mix_plan(int N, int C, int n_val, int epochs, int Bv, int blocks, const fs_tuning& t);

// One entry point per solver: choose the template instance from what the plan fixed and launch
// it.  FS_OK, or a status from fail().
int launch_mix_global(const MixArgs& a, const MixPlan& plan, hipStream_t st);
int launch_mix_staged(const MixArgs& a, const MixPlan& plan, hipStream_t st);
int launch_mix_reg(const MixArgs& a, const MixPlan& plan, hipStream_t st);
int launch_mix_reg2(const MixArgs& a, const MixPlan& plan, hipStream_t st);
int launch_mix_quad(const MixArgs& a, const MixPlan& plan, hipStream_t st);
int launch_mix_wave(const MixArgs& a, const MixPlan& plan, hipStream_t st);
int launch_mix_bin(const MixArgs& a, const MixPlan& plan, hipStream_t st);
int launch_mix_mc(const MixArgs& a, const MixPlan& plan, hipStream_t st);
int launch_mix_qmc(const MixArgs& a, const MixPlan& plan, hipStream_t st);

}  // namespace fs

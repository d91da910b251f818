// What the exchanging local-training forms (split with its team and double-buffered instances,
// pair, pipe) share with their host side, local_train_host.cpp: the constants both the kernels
// and the host geometry read, and each kernel file's one entry point.  No device code here.
// The planner, the workspace layout, the hand-off tags and the launch setup live in
// local_train_host.cpp, which no kernel revision (_lib.source_revision) covers.
#pragma once

#include "common.h"

namespace fs {

struct SplitWS;

// the split form (local_train_split.hip, local_train_dbuf.hip)
constexpr int SP_WAVES = 8;
constexpr int SP_TPW = 2;                 // max 64-column tiles per wave (register budget)
constexpr unsigned SP_SPIN_LIMIT = 1u << 22;
constexpr int SP_ERR_BYTES = 256;         // error block at the END of the workspace (never memset)

// the pair form (local_train_pair.hip)
constexpr int PR_WAVES = 8;
constexpr int PR_THREADS = PR_WAVES * 64;
constexpr int PR_TILES = PR_WAVES;            // 64-column tiles per workgroup and client (one per wave)
constexpr unsigned PR_SPIN_LIMIT = 1u << 22;
constexpr int PR_ERR_BYTES = 256;

// the pipe form (local_train_pipe.hip)
constexpr int PP_WAVES = 8;
constexpr int PP_THREADS = PP_WAVES * 64;
constexpr int PP_TPW = 2;                 // 64-column tiles per wave (the slice is 16 tiles)
constexpr int PP_NTS = PP_WAVES * PP_TPW;
constexpr int PP_RS = PP_NTS * 64 + 8;    // LDS image row stride (floats)
constexpr int PP_NR = 32;                 // batch rows (two 16-row tiles)
constexpr int PP_SZ = 520;                // granules per (group, parity, slice): [rt][kk][lane] + 2 norms
constexpr int PP_ERR_BYTES = 256;

// 16-row batch tiles of a step (every exchanging form: B <= 32)
constexpr int lt_rt(int B) { return B <= 16 ? 1 : 2; }

// One entry point per kernel file: choose the instance for (P, G) and launch it on `grid`
// workgroups with `lds` bytes of dynamic LDS.  FS_OK, or a status from fail().
int launch_local_train_single(const LTParams& P, hipStream_t st);
int launch_split_instance(const LTParams& P, int G, const SplitWS& X, int grid, size_t lds, hipStream_t st);
int launch_teams_instance(const LTParams& P, int G, const SplitWS& X, int grid, size_t lds, hipStream_t st);
int launch_pair_instance(const LTParams& P, int G, const SplitWS& X, int grid, size_t lds, hipStream_t st);
int launch_pipe_instance(const LTParams& P, int G, const SplitWS& X, int grid, size_t lds, hipStream_t st);

}  // namespace fs

// What the wide local-training form (local_train_wide.hip: one workgroup per client, the batch
// walked in 64-row blocks, any batch size) shares with its host side, local_train_host.cpp: the
// geometry of its workspace and its one entry point.  No device code here.
#pragma once

#include "common.h"

namespace fs {

constexpr int WD_WAVES = 8;
constexpr int WD_BLOCK = 64;              // batch rows per block (four 16-row MFMA tiles)
constexpr int WD_MAX_GRID = 512;          // workgroups of a parallel launch: a persistent grid walks d_order beyond
constexpr int WD_ERR_BYTES = 256;         // the workspace's last block (this form never writes it)

// padded classes: one or two 16-class MFMA tiles
constexpr int wd_nc(int C) { return C <= 16 ? 16 : 32; }
// workgroups launched: one walks a chain, at most WD_MAX_GRID walk parallel clients
constexpr int wd_grid(int N, int chained) { return chained ? 1 : (N < WD_MAX_GRID ? N : WD_MAX_GRID); }
// rows of one workgroup's gradient slot for batches of at most `bmax` rows (whole blocks)
constexpr int64_t wd_slot_rows(int64_t bmax) { return (bmax + WD_BLOCK - 1) / WD_BLOCK * WD_BLOCK; }

// The workspace: [grid] slots of [slot_rows][wd_nc(C)] floats -- a step's d CE / d z of every
// batch row, written by pass 1 and read by pass 2 of the workgroup that owns the slot -- then
// the error block.
struct WideWS {
  float* g;
  int64_t slot_floats;
  int slot_rows;
};

int launch_local_train_wide(const LTParams& P, const WideWS& X, int grid, hipStream_t st);

}  // namespace fs

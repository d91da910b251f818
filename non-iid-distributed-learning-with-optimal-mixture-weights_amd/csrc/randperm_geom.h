// Launch geometry of the capped shuffle replay (randperm.hip, round.hip): host arithmetic only,
// no device code -- plain C++, so a host program can include it on its own.
//
// The capped replay is a persistent launch of at most max_blocks workgroups.  A workgroup holds up
// to RP_MAX_WAVES waves; wave w of workgroup b replays passes b * waves + w, + total, + 2 total, ...
// (total = workgroups * waves), each wave on an LDS region of its own.
#pragma once

#include <algorithm>
#include <cstdint>

namespace fs {

constexpr int RP_MT_N = 624;                   // MT19937 state words
constexpr int RP_MAX_WAVES = 16;               // waves per capped workgroup (1024 threads)
constexpr int64_t RP_LDS_BYTES = 160 * 1024;   // LDS of a CU
constexpr int RP_LANE_PASSES = 64;             // passes of one wave of the per-lane form (max_n <= 64)
constexpr int RP_XCDS = 8;                     // workgroups are dealt round-robin over the XCDs

// words of one wave's LDS region: MT state, the tempered draws and (in_lds) the permutation,
// rounded to 16 bytes
inline int64_t rp_region_words(int64_t max_n, bool in_lds) {
  return (2 * (int64_t)RP_MT_N + (in_lds ? max_n : 0) + 3) / 4 * 4;
}

// the permutation lives in LDS where one region fits a CU's LDS (the uncapped kernel's rule)
inline bool rp_in_lds(int64_t max_n) { return 4 * (2 * (int64_t)RP_MT_N + max_n) <= RP_LDS_BYTES; }

// waves of one capped workgroup: as many LDS regions as fit a CU, at most 16 (per-lane form: 1)
inline int rp_waves(int64_t max_n) {
  if (max_n <= RP_LANE_PASSES) return 1;
  const int64_t region = 4 * rp_region_words(max_n, rp_in_lds(max_n));
  return (int)std::max<int64_t>(1, std::min<int64_t>(RP_MAX_WAVES, RP_LDS_BYTES / region));
}

// The cap for a replay of `npasses` passes (the shuffles of `rounds` rounds) beside training
// launches that leave `idle` CUs free.  0: no cap, the uncapped geometry.
//   * A multiple of 8: workgroup i goes to XCD i % 8, so the replay takes the same number of CUs
//     on every XCD and no XCD loses a CU its training workgroups need.
//   * At most half of each XCD's idle CUs: the training launches carry the fused evaluation on the
//     idle CUs, and its blocks cannot share a CU with a replay workgroup (LDS).  With half of them
//     left the evaluation takes two turns on them, still well inside the launch; with none left
//     it would wait for the replay's end and become the launch's tail (measured).
//   * The smallest such figure at which a wave (per-lane form: a workgroup, by blocks of 64) gets
//     at most `rounds` passes: a pass costs about half a client's training round (both are serial
//     in the client's rows), so the replay ends well inside the `rounds` rounds it has, and takes
//     no more CUs from the evaluation than that needs.  No figure qualifies: no cap.
//   * Passes too long for the LDS (rp_in_lds) shuffle in global memory: no cap, the uncapped kernel.
inline int rp_cap_blocks(int idle, int64_t npasses, int64_t max_n, int rounds) {
  if (!rp_in_lds(max_n)) return 0;
  const int per_xcd = idle / RP_XCDS / 2;
  const int64_t unit = max_n <= RP_LANE_PASSES ? RP_LANE_PASSES : 1;     // passes of one wave's turn
  const int64_t turns = (npasses + unit - 1) / unit;
  const int waves = rp_waves(max_n);
  for (int take = 1; take <= per_xcd; ++take) {
    const int64_t w = (int64_t)RP_XCDS * take * waves;
    if ((turns + w - 1) / w <= std::max(1, rounds)) return RP_XCDS * take;
  }
  return 0;
}

struct RpGeom {
  int blocks;        // workgroups (<= max_blocks)
  int waves;         // waves per workgroup (per-lane form: 1)
  int64_t lds;       // dynamic LDS bytes per workgroup (per-lane form: 0, its LDS is static)
};

// one wave per pass (max_n > 64): as many waves per workgroup as regions fit the LDS, at most 16,
// and no more workgroups than the passes need
inline RpGeom rp_capped_geom(int64_t npasses, int64_t max_n, int max_blocks) {
  const int64_t region = 4 * rp_region_words(max_n, rp_in_lds(max_n));
  const int waves = rp_waves(max_n);
  const int64_t need = (npasses + waves - 1) / waves;
  return {(int)std::max<int64_t>(1, std::min<int64_t>(max_blocks, need)), waves, region * waves};
}

// per-lane form (max_n <= 64): workgroups of one wave loop over the blocks of 64 passes
inline RpGeom rp_capped_lanes_geom(int64_t npasses, int max_blocks) {
  const int64_t need = (npasses + RP_LANE_PASSES - 1) / RP_LANE_PASSES;
  return {(int)std::max<int64_t>(1, std::min<int64_t>(max_blocks, need)), 1, 0};
}

// fs_randperm_device (include/fedsim.h) with a cap: max_blocks > 0 runs the replay in the capped
// geometry above, 0 in the C ABI's (one workgroup per pass; per-lane form: per 64 passes).  The
// same bits either way.  `stream` is a hipStream_t.
int randperm_device(const int64_t* d_seeds, const int64_t* d_n, const int64_t* d_off, int64_t npasses, int64_t max_n,
                    int32_t* d_out, uint32_t* d_err, int max_blocks, void* stream);

}  // namespace fs

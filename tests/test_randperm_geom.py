"""Host arithmetic of the capped shuffle replay (csrc/randperm_geom.h): needs no GPU.

The header is plain C++; a small program compiled here with the host compiler prints, for a grid
of (idle CUs, passes, max_n), the cap, the launch geometry and how often the wave / stride map of
randperm_capped_kernel (wave `id` of `total` replays passes id, id + total, ...) and the block loop
of the per-lane form visit every pass.  Checked:
  * the cap for (idle CUs, passes, max_n, rounds) is a multiple of 8, at most half the idle CUs
    of every XCD (the fused evaluation keeps the other half), the smallest such figure that
    leaves a wave at most `rounds` passes, and 0 (no cap) where none does or a pass may be too
    long for the LDS;
  * the workgroups never exceed the cap, the waves per workgroup are 1..16 and their LDS regions
    (2 x 624 words plus, in LDS, max_n ints each, 16-byte aligned) fit a CU's 160 KB;
  * every pass 0 .. P - 1 is visited exactly once: P = 1, waves - 1, waves + 1 (waves = the
    launch's total), 1,600 (a chunk of the headline) and 20,000 (a chunk of config 4).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'non-iid-distributed-learning-with-optimal-mixture-weights_amd', 'csrc')

PROGRAM = r'''
#include <cstdio>
#include <vector>
#include "randperm_geom.h"
using namespace fs;

// visits of every pass under the kernel's map: wave id = block * waves + wave, stride = total
static void visits(int64_t P, const RpGeom& g, int64_t& lo, int64_t& hi) {
  std::vector<int> seen((size_t)P, 0);
  const int64_t total = (int64_t)g.blocks * g.waves;
  for (int b = 0; b < g.blocks; ++b)
    for (int w = 0; w < g.waves; ++w)
      for (int64_t p = (int64_t)b * g.waves + w; p < P; p += total) ++seen[(size_t)p];
  lo = hi = seen[0];
  for (int v : seen) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
}

// the per-lane form: block blk (blk = b, b + blocks, ...) holds passes 64 blk .. 64 blk + 63
static void lane_visits(int64_t P, const RpGeom& g, int64_t& lo, int64_t& hi) {
  std::vector<int> seen((size_t)P, 0);
  for (int b = 0; b < g.blocks; ++b)
    for (int64_t blk = b; blk * 64 < P; blk += g.blocks)
      for (int l = 0; l < 64; ++l)
        if (blk * 64 + l < P) ++seen[(size_t)(blk * 64 + l)];
  lo = hi = seen[0];
  for (int v : seen) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
}

int main() {
  const int idles[] = {0, 1, 7, 8, 15, 16, 31, 32, 56, 63, 250, 256};
  const int64_t max_ns[] = {65, 512, 700, 2000, 10000, 40000, 41000, 100000};
  const int64_t cap_ns[] = {1, 40, 64, 65, 512, 10000, 41000};
  const int64_t cap_Ps[] = {1, 200, 1600, 4800, 20000};
  const int rounds[] = {1, 3, 8, 64};
  for (int idle : idles)
    for (int64_t max_n : cap_ns)
      for (int64_t P : cap_Ps)
        for (int r : rounds)
          std::printf("cap %d %lld %lld %d %d %d\n", idle, (long long)max_n, (long long)P, r,
                      rp_cap_blocks(idle, P, max_n, r), rp_waves(max_n));
  for (int cap : {8, 16, 56, 248}) {
    for (int64_t max_n : max_ns) {
      const RpGeom g0 = rp_capped_geom(1600, max_n, cap);
      const int64_t total = (int64_t)cap * g0.waves;
      const int64_t Ps[] = {1, total - 1, total + 1, 1600, 20000};
      for (int64_t P : Ps) {
        if (P < 1) continue;
        const RpGeom g = rp_capped_geom(P, max_n, cap);
        int64_t lo, hi;
        visits(P, g, lo, hi);
        std::printf("geom %d %lld %lld %d %d %lld %lld %d %lld %lld\n", cap, (long long)max_n, (long long)P, g.blocks,
                    g.waves, (long long)g.lds, (long long)rp_region_words(max_n, rp_in_lds(max_n)),
                    (int)rp_in_lds(max_n), (long long)lo, (long long)hi);
      }
    }
    const int64_t Ps[] = {1, 63, 64, 65, 64 * (int64_t)cap - 1, 64 * (int64_t)cap + 1, 1600, 20000};
    for (int64_t P : Ps) {
      const RpGeom g = rp_capped_lanes_geom(P, cap);
      int64_t lo, hi;
      lane_visits(P, g, lo, hi);
      std::printf("lanes %d %lld %d %d %lld %lld\n", cap, (long long)P, g.blocks, g.waves, (long long)lo, (long long)hi);
    }
  }
  return 0;
}
'''


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    # the compilers the library's own build needs (csrc/Makefile): g++, else hipcc's host compiler
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++') or \
        (hipcc if os.path.exists(hipcc) else shutil.which('hipcc'))
    assert cxx, 'no host C++ compiler: the library cannot be built here either'
    d = tmp_path_factory.mktemp('rp_geom')
    src, exe = os.path.join(d, 'geom.cpp'), os.path.join(d, 'geom')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    subprocess.run([cxx, '-std=c++17', '-O1', '-I', CSRC, src, '-o', exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return [ln.split() for ln in out.splitlines()]


def test_cap_is_a_multiple_of_8_within_the_idle_cus(lines):
    caps = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == 'cap']
    assert len(caps) == 12 * 7 * 5 * 4
    got = {}
    for idle, max_n, P, rounds, cap, waves in caps:
        got[idle, max_n, P, rounds] = cap
        assert cap % 8 == 0 and 0 <= cap <= idle
        assert cap // 8 <= idle // 8 // 2              # at most half of an XCD's idle CUs
        turns = -(-P // 64) if max_n <= 64 else P      # the per-lane form: blocks of 64 passes
        fits = [8 * k for k in range(1, idle // 16 + 1) if -(-turns // (8 * k * waves)) <= rounds]
        if 4 * (2 * 624 + max_n) > 160 * 1024:
            fits = []                                  # shuffled in global memory: the uncapped kernel
        assert cap == (fits[0] if fits else 0)         # the smallest that ends in time, else no cap
    assert got[56, 512, 1600, 8] == 16                 # the headline's chunk: 2 CUs per XCD, 7 passes per wave
    assert got[56, 512, 200, 1] == 16                  # ... and its per-round replay
    assert got[15, 512, 1600, 8] == 0 and got[0, 512, 1600, 8] == 0
    assert got[16, 40, 1600, 8] == 8                   # per-lane form: 25 blocks on 8 workgroups


def test_waves_and_regions_fit_the_lds(lines):
    geoms = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == 'geom']
    assert geoms
    for cap, max_n, P, blocks, waves, lds, region, in_lds, lo, hi in geoms:
        assert 1 <= blocks <= cap
        assert 1 <= waves <= 16
        assert region % 4 == 0 and region >= 2 * 624 + (max_n if in_lds else 0)
        assert lds == 4 * region * waves and lds <= 160 * 1024
        assert in_lds == (4 * (2 * 624 + max_n) <= 160 * 1024)
        # as many waves as fit: one more region would not, unless 16 are in
        assert waves == 16 or 4 * region * (waves + 1) > 160 * 1024
        assert blocks == min(cap, -(-P // waves))
    by_n = {g[1]: g for g in geoms if g[0] == 16 and g[2] == 1600}
    assert by_n[512][3:5] == [16, 16]                  # the headline: 16 workgroups of 16 waves
    assert by_n[10000][4] == 3 and by_n[41000][4] == 16 and by_n[41000][7] == 0


def test_every_pass_is_replayed_exactly_once(lines):
    n = 0
    for ln in lines:
        if ln[0] in ('geom', 'lanes'):
            assert ln[-2:] == ['1', '1'], ln
            n += 1
    assert n > 100
    lanes = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == 'lanes']
    for cap, P, blocks, waves, lo, hi in lanes:
        assert waves == 1 and blocks == min(cap, -(-P // 64))

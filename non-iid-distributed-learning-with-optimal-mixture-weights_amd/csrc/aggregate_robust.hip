// fs_aggregate_robust: the coordinate-wise beta-trimmed mean and median (Yin, Chen, Ramchandran,
// Bartlett, ICML 2018) of the M rows d_sel (NULL: rows 0..M-1) of d_W_all.  The first aggregate
// here that is not a fold: it needs two order statistics per coordinate across the M rows, so its
// work is selection in LDS, not HBM bytes.  The rule and its summation order: include/fedsim.h.
//
// Geometry.  A workgroup of 256 threads owns a stripe of W consecutive columns (W = 32: 128 B of
// every row; 16 and 8 for the M that no longer fit 32 columns into the CU's 160 KiB).  It
//   1. stages the stripe of all M rows into LDS as monotone 32-bit keys, column-major with the odd
//      pitch M | 1 (so the W columns of one k fall into different banks): one float4 load per row
//      element, 8 row loads in flight per thread, the sel ids of the next group of 8 loaded before
//      this group's rows are waited for, no load under a condition (row and column are clamped,
//      the LDS write and the final store are what the conditions guard);
//   2. runs the two radix selects (ranks b+1 and M-b) of every column with 4-bit digits, most
//      significant first: the T = 256 / W threads of a column walk its keys k-strided and count
//      the digits of the keys that match the select's prefix into 16 LDS counters (ds_add, two
//      16-bit counters to a dword, never cleared between the passes: a thread subtracts what it read
//      last; 8 key reads in flight per thread), all of them then read the counters and take the
//      same step.  While the two prefixes agree one histogram serves both selects.  Counts are
//      integers: the order of the atomics cannot reach the result.  The last pass leaves, for
//      each threshold, how many keys lie below it and how many equal it -- the tie counts need
//      no pass of their own;
//   3. sums the strictly-inside values in double, each thread its k-strided slice in ascending k
//      (skipped when n <= 2: nothing lies strictly between two neighbouring ranks), joins the T
//      slices by the fixed pairwise tree in LDS, adds the two tie terms count * value (a term with
//      count 0 is left out: 0 * Inf), divides by n and rounds once to float.
// The deferred evaluation's finaliser rides as an extra last workgroup, as on the folds.
#include "aggregate_sel.h"
#include "common.h"
#include "finalize.h"

namespace fs {

#pragma clang fp contract(off)

constexpr int RB_NT = 256;                                   // threads of a workgroup
constexpr int RB_LDS = 160 * 1024;                           // the CU's LDS
constexpr int RB_HP = 17;                                    // dwords of a column's two histograms (2 * 8, + 1: banks)
constexpr int RB_AUX = 2304;                                 // bytes: the histograms (32 * 17 * 4), then the slices' sums (256 * 8)
constexpr int RB_KEYS = (RB_LDS - RB_AUX) / 4;               // keys a workgroup can stage
constexpr int RB_GRP = 8;                                    // row loads in flight per thread

static_assert(RB_AUX >= 32 * RB_HP * 4 && RB_AUX >= RB_NT * 8 && RB_AUX % 16 == 0, "the aux region holds either use");

__host__ __device__ constexpr int rb_pitch(int M) { return M | 1; }
// the largest M at W columns: W * (M | 1) <= RB_KEYS
constexpr int rb_max_m(int W) { return ((RB_KEYS / W) & 1) ? RB_KEYS / W : RB_KEYS / W - 1; }
constexpr int RB_MAX_M32 = rb_max_m(32), RB_MAX_M16 = rb_max_m(16), RB_MAX_M8 = rb_max_m(8);
static_assert(RB_MAX_M32 >= 1250 && RB_MAX_M8 >= 2048 && RB_MAX_M8 <= 65535, "the widths' ranges");

__device__ __forceinline__ uint32_t rb_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rb_val(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// one select's step after a pass: the digit whose cumulative count first reaches rem.  h: the
// pass's 16 counts, two to a dword (the counters are never cleared: the caller passes differences,
// which cannot borrow across the halves -- a half only grows, by at most 8 * M <= 40,376 in all)
__device__ __forceinline__ void rb_step(const uint32_t* h, int shift, uint32_t& prefix, int& rem, int& eq) {
  int cum = 0, d = 15, before = 0, cnt = 0;
  bool found = false;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = (int)((h[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu);
    if (!found && cum + c >= rem) {
      found = true;
      d = j;
      before = cum;
      cnt = c;
    }
    cum += c;
  }
  prefix |= (uint32_t)d << shift;
  rem -= before;
  eq = cnt;
}

template <int W, bool SEL>
__global__ __launch_bounds__(RB_NT) void aggregate_robust_kernel(const float* __restrict__ Wall, int64_t stride,
                                                                 const int32_t* __restrict__ sel, int M, int64_t len4,
                                                                 int b, float* __restrict__ out, EvalFinalize fin) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rb_lds[];
  if (fin.part && blockIdx.x == gridDim.x - 1) {
    eval_finalize_block(fin.part, fin.nb, fin.n, fin.out, reinterpret_cast<double(*)[256]>(rb_lds));
    return;
  }
  constexpr int T = RB_NT / W;          // threads (slices) per column
  constexpr int Q4 = W / 4;             // float4 per row of the stripe
  constexpr int RP = RB_NT / Q4;        // rows a workgroup loads at once
  uint32_t* hist = rb_lds;              // [W][RB_HP]
  double* part = reinterpret_cast<double*>(rb_lds);   // [T][W], after the selects
  uint32_t* keys = rb_lds + RB_AUX / 4; // [W][pitch]
  const int pitch = rb_pitch(M);
  const int tid = threadIdx.x;

  // ---- 1. stage ----
  {
    const int q = tid % Q4, r = tid / Q4;
    int64_t c4 = (int64_t)blockIdx.x * Q4 + q;
    if (c4 >= len4) c4 = len4 - 1;      // a ragged last stripe: a valid column, never stored
    const float* base = Wall + 4 * c4;
    uint32_t* kq = keys + (4 * q) * pitch;
    int row[RB_GRP];
#pragma unroll
    for (int u = 0; u < RB_GRP; ++u) {
      const int k = min(u * RP + r, M - 1);
      row[u] = SEL ? sel[k] : k;
    }
    for (int k0 = 0; k0 < M; k0 += RB_GRP * RP) {
      float4 v[RB_GRP];
#pragma unroll
      for (int u = 0; u < RB_GRP; ++u) v[u] = ld4(base + (int64_t)row[u] * stride);
#pragma unroll
      for (int u = 0; u < RB_GRP; ++u) {
        const int k = min(k0 + RB_GRP * RP + u * RP + r, M - 1);
        row[u] = SEL ? sel[k] : k;
      }
#pragma unroll
      for (int u = 0; u < RB_GRP; ++u) {
        const int k = k0 + u * RP + r;
        if (k < M) {
          kq[k] = rb_key(v[u].x);
          kq[pitch + k] = rb_key(v[u].y);
          kq[2 * pitch + k] = rb_key(v[u].z);
          kq[3 * pitch + k] = rb_key(v[u].w);
        }
      }
    }
  }

  // ---- 2. the two selects ----
  const int c = tid % W, s = tid / W;
  const uint32_t* kc = keys + c * pitch;
  uint32_t* hc = hist + c * RB_HP;
  uint32_t plo = 0, phi = 0;
  int rlo = b + 1, rhi = M - b, elo = 0, ehi = 0;
  bool same = true;
  uint32_t seen[16];                    // the counters as this thread last read them
#pragma unroll
  for (int j = 0; j < 16; ++j) seen[j] = 0u;
  for (int i = tid; i < W * RB_HP; i += RB_NT) hist[i] = 0u;
  __syncthreads();                      // the staged keys and the cleared counters
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 28 - 4 * pass;
    const uint32_t mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 4));
    // RB_GRP key reads in flight, then their counts (the index is clamped, the count is what the
    // condition guards)
    for (int k0 = s; k0 < M; k0 += RB_GRP * T) {
      uint32_t key[RB_GRP];
#pragma unroll
      for (int u = 0; u < RB_GRP; ++u) key[u] = kc[min(k0 + u * T, M - 1)];
#pragma unroll
      for (int u = 0; u < RB_GRP; ++u) {
        if (k0 + u * T < M) {
          const uint32_t d = (key[u] >> shift) & 15u;
          const uint32_t one = 1u << ((d & 1u) * 16);
          if (((key[u] ^ plo) & mask) == 0u) atomicAdd(&hc[d >> 1], one);
          if (!same && ((key[u] ^ phi) & mask) == 0u) atomicAdd(&hc[8 + (d >> 1)], one);
        }
      }
    }
    __syncthreads();
    uint32_t h[8], g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t a = hc[j], c2 = hc[8 + j];
      h[j] = a - seen[j];
      g[j] = same ? h[j] : c2 - seen[8 + j];
      seen[j] = a;
      seen[8 + j] = c2;
    }
    rb_step(h, shift, plo, rlo, elo);
    rb_step(g, shift, phi, rhi, ehi);
    same = same && plo == phi;
    __syncthreads();                    // the counters are read before the next pass adds to them
  }
  // plo, phi: the keys at ranks b+1 and M-b; below them lie b + 1 - rlo and M - b - rhi keys, equal
  // to them are elo and ehi
  const int n = M - 2 * b;
  int clo, chi;                          // kept copies of the two thresholds
  if (plo == phi) {
    clo = n;
    chi = 0;
  } else {
    clo = (b + 1 - rlo) + elo - b;
    chi = rhi;
  }

  // ---- 3. the sum ----
  double acc = 0.0;
  if (n > 2) {
    for (int k0 = s; k0 < M; k0 += RB_GRP * T) {
      uint32_t key[RB_GRP];
#pragma unroll
      for (int u = 0; u < RB_GRP; ++u) key[u] = kc[min(k0 + u * T, M - 1)];
#pragma unroll
      for (int u = 0; u < RB_GRP; ++u)
        if (k0 + u * T < M && key[u] > plo && key[u] < phi) acc += (double)rb_val(key[u]);
    }
    part[s * W + c] = acc;
    __syncthreads();
    if (s == 0) {
      double p[T];
#pragma unroll
      for (int j = 0; j < T; ++j) p[j] = part[j * W + c];
#pragma unroll
      for (int h2 = 1; h2 < T; h2 *= 2)
#pragma unroll
        for (int j = 0; j < T; j += 2 * h2) p[j] += p[j + h2];
      acc = p[0];
    }
  }
  if (s == 0) {
    const int64_t col = (int64_t)blockIdx.x * W + c;
    if (col < 4 * len4) {
      const double tlo = (double)clo * (double)rb_val(plo);
      double sum = n > 2 ? acc + tlo : tlo;                     // (clo >= 1 always: rank b+1 is kept)
      if (chi > 0) sum += (double)chi * (double)rb_val(phi);
      out[col] = (float)(sum / (double)n);
    }
  }
}

static int rb_width(int M) { return M <= RB_MAX_M32 ? 32 : M <= RB_MAX_M16 ? 16 : 8; }

// dynamic LDS beyond the 64 KB a kernel gets unasked (set once per kernel, to the whole CU's)
template <int W, bool SEL>
static int rb_launch(const float* Wall, int64_t stride, const int32_t* sel, int M, int64_t len, int b, float* out,
                     const EvalFinalize& fin, hipStream_t st) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&aggregate_robust_kernel<W, SEL>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, RB_LDS);
  if (attr != hipSuccess) return fail(FS_EHIP, std::string("fs_aggregate_robust: ") + hipGetErrorString(attr));
  size_t lds = (size_t)RB_AUX + (size_t)W * rb_pitch(M) * 4;
  if (fin.part) lds = std::max(lds, (size_t)(2 * 256 * sizeof(double)));
  const int64_t blocks = (len + W - 1) / W + (fin.part ? 1 : 0);
  hipLaunchKernelGGL((aggregate_robust_kernel<W, SEL>), dim3((unsigned)blocks), dim3(RB_NT), lds, st, Wall, stride, sel,
                     M, len / 4, b, out, fin);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int aggregate_robust_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len, int b,
                            float* d_out, const EvalFinalize* fin, hipStream_t st) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(M <= RB_MAX_M8, "M is larger than fs_aggregate_robust_max_m()");
  FS_REQUIRE(b >= 0 && 2 * (int64_t)b < M, "the trim count needs 0 <= 2b < M");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_out, "null pointer");
  const EvalFinalize none{nullptr, 0, 0, nullptr};
  const EvalFinalize& f = fin ? *fin : none;
  const int W = rb_width(M);
  if (d_sel) {
    if (W == 32) return rb_launch<32, true>(d_W_all, stride, d_sel, M, len, b, d_out, f, st);
    if (W == 16) return rb_launch<16, true>(d_W_all, stride, d_sel, M, len, b, d_out, f, st);
    return rb_launch<8, true>(d_W_all, stride, d_sel, M, len, b, d_out, f, st);
  }
  if (W == 32) return rb_launch<32, false>(d_W_all, stride, d_sel, M, len, b, d_out, f, st);
  if (W == 16) return rb_launch<16, false>(d_W_all, stride, d_sel, M, len, b, d_out, f, st);
  return rb_launch<8, false>(d_W_all, stride, d_sel, M, len, b, d_out, f, st);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_robust_max_m(void) { return RB_MAX_M8; }

extern "C" int fs_aggregate_robust(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len, int b,
                                   float* d_out, void* stream) {
  return aggregate_robust_launch(d_W_all, stride, d_sel, M, len, b, d_out, nullptr, reinterpret_cast<hipStream_t>(stream));
}

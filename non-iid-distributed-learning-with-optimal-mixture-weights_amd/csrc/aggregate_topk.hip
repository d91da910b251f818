// fs_topk_threshold, fs_aggregate_topk -- top-k sparsified uploads with error feedback (Aji & Heafield
// 2017; Stich, Cordonnier & Jaggi, NeurIPS 2018; Sattler et al. 2019).  Over the M sampled rows
// W_k = d_W_all[row_k], x = d_W_g on entry, the residual rows e_k = d_e[row_k] (d_e == NULL: none) and
// 1 <= kcount <= len, every float operation rounded separately:
//
//   a_k[i]  = fl(fl(W_k[i] - x[i]) + e_k[i])                      (no memory: fl(W_k[i] - x[i]))
//   key(v)  = bits(v) & 0x7fffffff                                  (magnitude order; Inf above finite, NaN above Inf)
//   tau_k   = the kcount-th largest key of the row;  i is kept iff key(a_k[i]) >= tau_k
//   e_k[i] <- kept ? +0 : a_k[i]
//   W_g[i] <- fl(x[i] + sum_k fl(q_k * (kept ? a_k[i] : +0)))      (k ascending, fs_aggregate's regimes)
//
// Stage A (topk_threshold_kernel): one workgroup of 1024 threads per sampled row.  Pass 0 forms a_k
// from W_k, x and e_k and stores it INTO e_k (with memory), histogramming the keys' top digit on the
// way; three more passes over a_k (read back from e_k: the row was just written, an L2 / MALL hit;
// without memory re-formed from W_k and x) refine the threshold digit by digit -- a most-significant-
// digit-first radix select on the 31-bit keys, digits of 8, 8, 8 and 7 bits.  The counts are integer
// LDS atomics (order-independent), so tau_k and n_k are exact and the same on every run.  No float
// atomics, no global atomics, no cross-workgroup wait, no workspace, no allocation.
//
// Stage B (TopkRule, a rule of aggregate_fold.h): the fold of fl(q_k * s_k) in FedNova's mode-2
// regimes, reading ONE row stream -- a_k from e_k (without memory: W_k, and x once per thread) --
// and storing zeros over the kept positions of e_k.  Every (k, i) belongs to exactly one thread in
// every regime (a sub-range or chunk of k at one float4 position), so the in-place store is race-free.
//
// Data flow per call, in floats: A reads 2 M len (+ x, cached) and writes M len, re-reads M len three
// times from cache; B reads M len and writes the kept float4s.  Re-forming a_k in B instead would
// read 3 M len there (5 M len + the passes in all against 4 M len).
#include "aggregate_fold.h"
#include "aggregate_sel.h"

namespace fs {

#pragma clang fp contract(off)

constexpr int TK_THREADS = 1024;     // stage A: threads of a row's workgroup
constexpr int TK_BINS = 256;         // bins of a digit's histogram
constexpr int TK_COPIES = 32;        // histogram copies ((wave & 7) * 4 + (lane & 3)): the exponent digit of
                                     // a row of like-sized values lands in a handful of bins
constexpr int TK_LD = TK_BINS + 1;   // copy stride (odd: the same bin of two copies in different banks)

__device__ __forceinline__ uint32_t topk_key(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// a_k at one float4 position, formed from W_k, x and (MEM) e_k
template <bool MEM>
__device__ __forceinline__ float4 topk_form(const float* w, const float* x, const float* e, int64_t i) {
  float4 a = sub4(ld4(w + 4 * i), ld4(x + 4 * i));
  if (MEM) a = add4(a, ld4(e + 4 * i));
  return a;
}

template <bool SEL, bool MEM>
__global__ __launch_bounds__(TK_THREADS) void topk_threshold_kernel(const float* __restrict__ W, int64_t stride,
                                                                    const int32_t* __restrict__ sel, int64_t len4,
                                                                    const float* __restrict__ x, float* E, int kcount,
                                                                    uint32_t* __restrict__ tau,
                                                                    int32_t* __restrict__ kept) {
  __shared__ uint32_t hist[TK_COPIES * TK_LD];
  __shared__ uint32_t tot[TK_BINS];
  __shared__ uint32_t found[3];        // the digit, the keys above it, the keys in it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = blockIdx.x;
  const int64_t row = fold_row<SEL>(sel, k);
  const float* w = W + row * stride;
  float* e = MEM ? E + row * stride : nullptr;
  uint32_t* h = hist + ((wave & 7) * 4 + (lane & 3)) * TK_LD;

  uint32_t prefix = 0, pmask = 0;      // the threshold's digits found so far, and their bits
  uint32_t need = (uint32_t)kcount;    // the threshold is the need-th largest key under the prefix
  uint32_t greater = 0;                // keys above every key under the prefix
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = pass == 3 ? 0 : 23 - 8 * pass;          // 23, 15, 7, 0
    const uint32_t dmask = pass == 3 ? 0x7fu : 0xffu;
    for (int j = tid; j < TK_COPIES * TK_LD; j += TK_THREADS) hist[j] = 0;
    __syncthreads();
    for (int64_t i = tid; i < len4; i += TK_THREADS) {
      float4 a;
      if (pass == 0 || !MEM) {
        a = topk_form<MEM>(w, x, e, i);
        if (MEM && pass == 0) st4(e + 4 * i, a);               // (read back below by this same thread)
      } else {
        a = ld4(e + 4 * i);
      }
      const uint32_t key[4] = {topk_key(a.x), topk_key(a.y), topk_key(a.z), topk_key(a.w)};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if ((key[c] & pmask) == prefix) atomicAdd(&h[(key[c] >> shift) & dmask], 1u);
    }
    __syncthreads();
    if (tid < TK_BINS) {
      uint32_t s = 0;
#pragma unroll 8
      for (int c = 0; c < TK_COPIES; ++c) s += hist[c * TK_LD + tid];
      tot[tid] = s;
    }
    __syncthreads();
    if (wave == 0) {
      // lane l holds bins 4l .. 4l+3; above = the count of the bins above them (a suffix scan over the lanes)
      uint32_t b[4], mine = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        b[c] = tot[4 * lane + c];
        mine += b[c];
      }
      uint32_t incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_down(incl, d, 64);
        if (lane + d < 64) incl += o;
      }
      uint32_t above = incl - mine;
#pragma unroll
      for (int c = 3; c >= 0; --c) {
        if (above < need && need <= above + b[c]) {           // exactly one bin of one lane
          found[0] = (uint32_t)(4 * lane + c);
          found[1] = above;
          found[2] = b[c];
        }
        above += b[c];
      }
    }
    __syncthreads();
    prefix |= found[0] << shift;
    pmask |= dmask << shift;
    greater += found[1];
    need -= found[1];
    // (the next pass's zeroing of hist follows a barrier; found is rewritten only after two more)
  }
  if (tid == 0) {
    tau[k] = prefix;
    kept[k] = (int32_t)(greater + found[2]);
  }
}

// ---- stage B: the thresholded fold ---------------------------------------------------------------------
__device__ __forceinline__ float topk_pick(float a, uint32_t t, float& rest) {
  const bool kp = topk_key(a) >= t;
  rest = kp ? 0.f : a;
  return kp ? a : 0.f;
}

// The left fold of fl(q_k * s_k), k = k0 .. k1-1, at one float4 position, in clamped groups of 8
// (fold_group's schedule: the 8 row loads, weights and thresholds before the first fold; a short last
// group re-reads the range's last row and skips the folds).  MEM: R is the residual buffer holding
// a_k, and a float4 with a kept position is stored back with those positions zeroed -- after every
// load of its group, and no later group reads the row again.  Else R is d_W_all and a_k = fl(W_k - x).
template <bool SEL, bool MEM>
__device__ __forceinline__ float4 topk_fold_range(const float* R, int64_t stride, const int32_t* __restrict__ sel,
                                                  const float* __restrict__ q, const uint32_t* __restrict__ tau,
                                                  float4 x, int k0, int k1) {
  float4 acc = zero4();
  const int last = k1 - 1;
  for (int k = k0; k < k1; k += 8) {
    int64_t off[8];
    float4 v[8];
    float qv[8];
    uint32_t tv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) off[u] = (int64_t)fold_row<SEL>(sel, min(k + u, last)) * stride;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ku = min(k + u, last);
      v[u] = ld4(R + off[u]);
      qv[u] = q[ku];
      tv[u] = tau[ku];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k + u < k1) {
        const float4 a = MEM ? v[u] : sub4(v[u], x);
        float4 s, r;
        s.x = topk_pick(a.x, tv[u], r.x);
        s.y = topk_pick(a.y, tv[u], r.y);
        s.z = topk_pick(a.z, tv[u], r.z);
        s.w = topk_pick(a.w, tv[u], r.w);
        const float4 t = scaled4(qv[u], s);
        if (u == 0 && k == k0)
          acc = t;
        else
          acc = add4(acc, t);
        if (MEM) {
          const bool any = topk_key(a.x) >= tv[u] || topk_key(a.y) >= tv[u] || topk_key(a.z) >= tv[u] ||
                           topk_key(a.w) >= tv[u];
          if (any) st4(const_cast<float*>(R) + off[u], r);
        }
      }
  }
  return acc;
}

// every thread of a position without memory reads x (its terms subtract it); with memory only the
// one that finishes, which stores x + delta
template <bool MEM>
struct TopkFinish {
  static constexpr int SETS = 1;
  static constexpr bool RIDES = true;
  float* W_g;
  struct Ctx {
    float4 x = zero4();
  };
  __device__ __forceinline__ Ctx load(int64_t i, bool fin) const {
    Ctx c;
    if (!MEM || fin) c.x = ld4(W_g + 4 * i);
    return c;
  }
  __device__ __forceinline__ void finish(int64_t i, const Ctx& cx, const Acc<1>& t) const {
    st4(W_g + 4 * i, add4(cx.x, t.a[0]));
  }
};

template <bool SEL, bool MEM>
struct TopkRule {
  using Finish = TopkFinish<MEM>;
  Finish f;
  const int32_t* sel;     // [M] row ids (SEL), else rows 0..M-1
  const float* q;         // [M]
  const uint32_t* tau;    // [M] threshold keys
  __device__ __forceinline__ Acc<1> fold(const float* R, int64_t stride, const typename Finish::Ctx& cx, int k0, int k1,
                                         bool) const {
    return {{topk_fold_range<SEL, MEM>(R, stride, sel, q, tau, cx.x, k0, k1)}};
  }
};

static int topk_check(const char* fn, const float* d_W_all, int64_t stride, int M, int64_t len, int64_t kcount,
                      const float* d_W_g, const float* d_e, const float* d_tau, const int32_t* d_kept) {
#define TK_REQUIRE(cond, msg)                                                  \
  do {                                                                         \
    if (!(cond)) return ::fs::fail(FS_EINVAL, std::string(fn) + ": " + (msg)); \
  } while (0)
  TK_REQUIRE(M >= 1, "M must be >= 1");
  TK_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  TK_REQUIRE(len <= 0x7fffffff, "len must be below 2^31 (the kept counts are int32)");
  TK_REQUIRE(kcount >= 1 && kcount <= len, "kcount must be in [1, len]");
  TK_REQUIRE(d_W_all && d_W_g && d_tau && d_kept, "null pointer");
  TK_REQUIRE(!d_e || (d_e != d_W_all && d_e != d_W_g), "d_e must not be d_W_all or d_W_g");
#undef TK_REQUIRE
  return FS_OK;
}

static int topk_threshold_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                                 const float* d_W_g, float* d_e, int kcount, float* d_tau, int32_t* d_kept,
                                 hipStream_t st) {
  uint32_t* tau = reinterpret_cast<uint32_t*>(d_tau);
#define TK_GO(S, E)                                                                                              \
  hipLaunchKernelGGL((topk_threshold_kernel<S, E>), dim3((unsigned)M), dim3(TK_THREADS), 0, st, d_W_all, stride, \
                     d_sel, len / 4, d_W_g, d_e, kcount, tau, d_kept)
  if (d_sel) {
    if (d_e) TK_GO(true, true); else TK_GO(true, false);
  } else {
    if (d_e) TK_GO(false, true); else TK_GO(false, false);
  }
#undef TK_GO
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int aggregate_topk_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                          int64_t len, int64_t kcount, float* d_W_g, float* d_e, float* d_tau, int32_t* d_kept,
                          float* d_ws, int64_t ws_floats, int chunks, void* d_sws, int64_t sws_bytes,
                          const EvalFinalize* fin, hipStream_t st) {
  int rc = topk_check("fs_aggregate_topk", d_W_all, stride, M, len, kcount, d_W_g, d_e, d_tau, d_kept);
  if (rc != FS_OK) return rc;
  FS_REQUIRE(d_q, "null pointer");
  FS_REQUIRE(sws_bytes >= aggregate_topk_ws_bytes(M, len), "d_sws is too small (fs_aggregate_topk_ws_bytes(M, len))");
  (void)d_sws;
  rc = topk_threshold_launch(d_W_all, stride, d_sel, M, len, d_W_g, d_e, (int)kcount, d_tau, d_kept, st);
  if (rc != FS_OK) return rc;
  const uint32_t* tau = reinterpret_cast<const uint32_t*>(d_tau);
  // with memory the fold's row stream is the residual buffer (a_k), else the clients' rows
  const float* R = d_e ? d_e : d_W_all;
#define TK_GO(S, E) \
  return fold_dispatch(R, stride, TopkRule<S, E>{{d_W_g}, d_sel, d_q, tau}, M, len, d_ws, ws_floats, chunks, fin, st)
  if (d_sel) {
    if (d_e) TK_GO(true, true);
    TK_GO(true, false);
  }
  if (d_e) TK_GO(false, true);
  TK_GO(false, false);
#undef TK_GO
}

int64_t aggregate_topk_ws_bytes(int, int64_t) { return 0; }   // the select keeps its counts in LDS

}  // namespace fs

using namespace fs;

extern "C" int64_t fs_aggregate_topk_ws_bytes(int M, int64_t len) { return aggregate_topk_ws_bytes(M, len); }

extern "C" int fs_topk_threshold(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                                 const float* d_W_g, float* d_e, int64_t kcount, float* d_tau, int32_t* d_kept,
                                 void* d_ws, int64_t ws_bytes, void* stream) {
  const int rc = topk_check("fs_topk_threshold", d_W_all, stride, M, len, kcount, d_W_g, d_e, d_tau, d_kept);
  if (rc != FS_OK) return rc;
  FS_REQUIRE(ws_bytes >= aggregate_topk_ws_bytes(M, len), "d_ws is too small (fs_aggregate_topk_ws_bytes(M, len))");
  (void)d_ws;
  return topk_threshold_launch(d_W_all, stride, d_sel, M, len, d_W_g, d_e, (int)kcount, d_tau, d_kept,
                               reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_aggregate_topk(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                                 int64_t len, int64_t kcount, float* d_W_g, float* d_e, float* d_tau, int32_t* d_kept,
                                 float* d_ws, int64_t ws_floats, int chunks, void* d_sws, int64_t sws_bytes,
                                 void* stream) {
  return aggregate_topk_launch(d_W_all, stride, d_sel, d_q, M, len, kcount, d_W_g, d_e, d_tau, d_kept, d_ws, ws_floats,
                               chunks, d_sws, sws_bytes, nullptr, reinterpret_cast<hipStream_t>(stream));
}

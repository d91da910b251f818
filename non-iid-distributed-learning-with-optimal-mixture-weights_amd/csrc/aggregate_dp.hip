// fs_dp_norms, fs_dp_coef, fs_dp_noise, fs_aggregate_dp -- DP-FedAvg's server step (McMahan, Ramage,
// Talwar & Zhang, ICLR 2018; Geyer, Klein & Nabi 2017; the adaptive clip of Andrew, Thakkar, McMahan &
// Ramaswamy, NeurIPS 2021): per-client norm clipping and Gaussian noise on the aggregate.  Over the
// M sampled rows W_k = d_W_all[row_k], x = d_W_g on entry, weights q_k, clip S, noise multiplier z,
// seed s and round t, every float operation rounded separately:
//
//   d_k   = fl(W_k - x)
//   n_k   = sum_i d_k[i]^2                    float inside a wave's share, double above it
//   r_k   = sqrt(n_k),  s_k = r_k <= S ? 1 : S / r_k                  (double)
//   c_k   = f32(q_k * s_k);  a row whose n_k is NaN or Inf is dropped: c_k = 0
//   Delta = sum_k (c_k == 0 ? +0 : fl(c_k * d_k))                     (k ascending, fs_aggregate_opt's regimes)
//   sigma = (z * S) * max_k q_k                                       (double; z == 0: 0)
//   x'    = fl(fl(x + Delta) + fl(f32(sigma) * g[i]))                 (z == 0: fl(x + Delta))
//
// Three stages, because a row's clip factor needs the whole row before its first term is folded.
//
// Stage A, the norm pass (dp_norms_kernel, dp_norms_sum_kernel): workgroup (bx, by) holds 256 float4
// positions and the 8 rows 8 by .. 8 by + 7; a thread forms e = ((dx^2 + dy^2) + dz^2) + dw^2 for
// each of its 8 rows from one coalesced float4 load per row, and the 8 terms are summed over the
// wave's 64 lanes by the reduce-scatter of lanes.h (class_totals<8>: three scatter levels, three
// butterfly levels, a fixed tree).  That float -- one wave's share of one row -- goes to the partial
// table nt[column][M], column = 4 bx + wave; every (column, k) is written exactly once, a lane past
// len4 or a row past M works on clamped loads and contributes zero or is not stored.  The second
// kernel sums a row's columns in double in a fixed order, one workgroup per row.  No atomics; the
// same bits on every call, and for rows gathered through d_sel.
//   ROUNDINGS: a square's path to its wave share holds at most 10 float roundings (the square, 3
//   sums in the thread, 6 levels across the lanes); all terms are non-negative, so n_k is within
//   10 x 2^-24 relative of the exact sum of squares of the float differences (the double sum above
//   adds a few 2^-53).  Squares that overflow float make the share, and so n_k, +Inf: the row is
//   dropped, as is a row holding a NaN or an Inf.
//
// Stage B (dp_coef_kernel): one workgroup.  c_k and r_k per row, then b = #{k kept : r_k <= S}, the
// dropped count and max_k q_k by integer / max trees (order-independent), the state
// {S, sigma, b, dropped, S_next} and, with the adaptive clip, S_next = S exp(-eta ((b + sigma_b g_b) / M
// - gamma)) written back to the device clip after every c_k has been formed from S.
//
// Stage C (DpRule, a rule of aggregate_fold.h): fs_aggregate_opt's fold -- clamped load schedule,
// regimes, chunks, stage-2 tree -- of the term above, and a finish that adds the position's noise.
// The noise is a field over the float4 positions, independent of the launch geometry: position i
// takes Philox4x32-10 at counter (i, t, stream, 0), key (s mod 2^32, s >> 32), u_j = (w_j + 0.5) 2^-32
// and two Box-Muller pairs, all in double, each normal rounded once to float (|g| <= sqrt(66 ln 2)).
// Where the parameters are rows of cols_ld floats of which only the first cols_d are real (a model
// padded to its leading dimension), the padding takes no noise and stays exactly zero.
// The finish touches no LDS and runs in the thread that writes the position, so the deferred
// evaluation's finaliser may ride on the one-launch form as it does on fs_aggregate_opt's: RIDES.
//
// Data flow in floats: A reads M len (+ x per 8 rows, cached), B touches M-sized data, C reads
// M len again (cache hits where M len fits the Infinity Cache) and writes len.  No float atomics, no
// global atomics, no cross-workgroup wait, no allocation, no host synchronisation.
#include "aggregate_fold.h"
#include "aggregate_sel.h"
#include "lanes.h"

namespace fs {

#pragma clang fp contract(off)

constexpr double DP_DBL_MAX = 1.7976931348623157e308;

// ---- Philox4x32-10 (Salmon, Moraes, Dror & Shaw, SC 2011) and the normals of one block ---------------
struct Philox4 {
  uint32_t w[4];
};

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ double dp_unit(uint32_t w) { return ((double)w + 0.5) * 2.3283064365386963e-10; }

// (g0, g1) from (w0, w1): sqrt(-2 ln u0) (cos, sin)(2 pi u1), in double, each rounded once
__device__ __forceinline__ void dp_pair(uint32_t w0, uint32_t w1, float& g0, float& g1) {
  const double rad = sqrt(-2.0 * log(dp_unit(w0)));
  const double ang = 6.283185307179586 * dp_unit(w1);
  g0 = (float)(rad * cos(ang));
  g1 = (float)(rad * sin(ang));
}

__device__ __forceinline__ float4 dp_normals(uint32_t i, uint32_t t, uint32_t stream, uint32_t k0, uint32_t k1) {
  const Philox4 p = philox4x32_10(i, t, stream, 0u, k0, k1);
  float4 g;
  dp_pair(p.w[0], p.w[1], g.x, g.y);
  dp_pair(p.w[2], p.w[3], g.z, g.w);
  return g;
}

__global__ __launch_bounds__(256) void dp_noise_kernel(uint32_t t, uint32_t stream, uint32_t k0, uint32_t k1,
                                                      int64_t len4, float* __restrict__ g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < len4) st4(g + 4 * i, dp_normals((uint32_t)i, t, stream, k0, k1));
}

// ---- stage A: the norm pass ------------------------------------------------------------------------------
template <bool SEL>
__global__ __launch_bounds__(256) void dp_norms_kernel(const float* __restrict__ W, int64_t stride,
                                                      const int32_t* __restrict__ sel, int M, int64_t len4,
                                                      const float* __restrict__ W_g, float* __restrict__ nt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < len4;
  const int64_t ic = live ? i : len4 - 1;
  const int k0 = 8 * (int)blockIdx.y;
  float4 v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u)
    v[u] = ld4(W + (int64_t)fold_row<SEL>(sel, min(k0 + u, M - 1)) * stride + 4 * ic);
  const float4 x = ld4(W_g + 4 * ic);
  float e[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float4 d = sub4(v[u], x);
    const float s = ((d.x * d.x + d.y * d.y) + d.z * d.z) + d.w * d.w;
    e[u] = live ? s : 0.f;
  }
  // every lane of the wave is active here; lane l ends with the wave's total of row k0 + l / 8
  const float tot = class_totals<8>(e, lane);
  const int k = k0 + (lane >> 3);
  if ((lane & 7) == 0 && k < M) nt[((int64_t)blockIdx.x * 4 + wave) * M + k] = tot;
}

// n[k] = the sum of row k's `cols` wave shares, in double: one workgroup per row, thread t the
// columns t, t + 256, ... in order, then the 256 sums by the halving tree -- a fixed order
__global__ __launch_bounds__(256) void dp_norms_sum_kernel(const float* __restrict__ nt, int64_t cols, int M,
                                                          double* __restrict__ n) {
  __shared__ double sums[256];
  const int k = blockIdx.x;
  double acc = 0.0;
  for (int64_t c = threadIdx.x; c < cols; c += 256) acc += (double)nt[c * M + k];
  sums[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sums[threadIdx.x] += sums[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) n[k] = sums[0];
}

static int64_t dp_cols(int64_t len4) { return (len4 + 255) / 256 * 4; }

// bytes of d_sws: n [M] double, then the table [columns][M] float
int64_t aggregate_dp_ws_bytes(int M, int64_t len) {
  if (M < 1 || len < 4) return 0;
  return (int64_t)M * 8 + dp_cols(len / 4) * M * 4;
}

// ---- stage B: the coefficients and the round's state ---------------------------------------------------
struct DpParams {
  double S, z;            // the clip (read from d_clip instead when adaptive) and the noise multiplier
  uint32_t t, k0, k1;     // round and Philox key
  int adaptive;
  double gamma, eta, sigma_b;
};

__global__ __launch_bounds__(256) void dp_coef_kernel(const double* __restrict__ n, const float* __restrict__ q,
                                                     float quni, int M, DpParams p, double* clip,
                                                     float* __restrict__ c, double* __restrict__ r,
                                                     double* __restrict__ state) {
  __shared__ int sb[256], sd[256];
  __shared__ float sq[256];
  const int tid = threadIdx.x;
  const double S = p.adaptive ? clip[0] : p.S;
  int b = 0, dr = 0;
  float mq = -INFINITY;                                    // (fmaxf's neutral element; M >= 1)
  for (int k = tid; k < M; k += 256) {
    const double nk = n[k];
    const float qk = q ? q[k] : quni;
    const bool finite = nk <= DP_DBL_MAX;                 // (a NaN fails)
    const double rk = sqrt(nk);
    const double sk = rk <= S ? 1.0 : S / rk;
    c[k] = finite ? (float)((double)qk * sk) : 0.f;
    r[k] = rk;
    b += finite && rk <= S;
    dr += !finite;
    mq = fmaxf(mq, qk);
  }
  sb[tid] = b;
  sd[tid] = dr;
  sq[tid] = mq;
  __syncthreads();                                         // (every thread has read the clip)
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      sb[tid] += sb[tid + h];
      sd[tid] += sd[tid + h];
      sq[tid] = fmaxf(sq[tid], sq[tid + h]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double bb = (double)sb[0];
    const double sigma = p.z == 0.0 ? 0.0 : (p.z * S) * (double)sq[0];
    double Sn = S;
    if (p.adaptive) {
      const Philox4 w = philox4x32_10(0u, p.t, 1u, 0u, p.k0, p.k1);
      float gb, unused;
      dp_pair(w.w[0], w.w[1], gb, unused);
      const double bt = bb + p.sigma_b * (double)gb;
      Sn = S * exp(-(p.eta * (bt / (double)M - p.gamma)));
      clip[0] = Sn;
    }
    state[0] = S;
    state[1] = sigma;
    state[2] = bb;
    state[3] = (double)sd[0];
    state[4] = Sn;
  }
}

// ---- stage C: the clipped fold ---------------------------------------------------------------------------
// fl(c_k * fl(W[row_k] - x)), or +0 where c_k == 0 (a select: a dropped row may hold NaN or Inf)
struct DpTerm {
  static constexpr int NC = 1, SETS = 1;
  const float* coef[1];   // c [M]
  float4 x;
  __device__ __forceinline__ Acc<1> term(bool, const float (&cf)[1], float4 w) const {
    const float4 t = scaled4(cf[0], sub4(w, x));
    return {{cf[0] == 0.f ? zero4() : t}};
  }
};

// every thread of a position reads x (its terms subtract it); the one that finishes adds the
// position's noise scaled by the state's sigma and stores
struct DpFinish {
  static constexpr int SETS = 1;
  static constexpr bool RIDES = true;
  float* W_g;
  const double* state;    // sigma at [1]
  uint32_t t, k0, k1;
  int noisy;              // z > 0
  int64_t cols_ld, cols_d;   // noise only where (element index mod cols_ld) < cols_d (cols_ld = 0: everywhere)
  struct Ctx {
    float4 x = zero4();
  };
  __device__ __forceinline__ Ctx load(int64_t i, bool) const {
    Ctx c;
    c.x = ld4(W_g + 4 * i);
    return c;
  }
  __device__ __forceinline__ void finish(int64_t i, const Ctx& cx, const Acc<1>& a) const {
    float4 y = add4(cx.x, a.a[0]);
    if (noisy) {
      const float4 n = add4(y, scaled4((float)state[1], dp_normals((uint32_t)i, t, 0u, k0, k1)));
      // (cols_ld is a multiple of 4: a float4 lies in one row of cols_ld)
      const int64_t c0 = cols_ld ? (4 * i) % cols_ld : 0, lim = cols_ld ? cols_d : 4;
      y.x = c0 < lim ? n.x : y.x;
      y.y = c0 + 1 < lim ? n.y : y.y;
      y.z = c0 + 2 < lim ? n.z : y.z;
      y.w = c0 + 3 < lim ? n.w : y.w;
    }
    st4(W_g + 4 * i, y);
  }
};

template <bool SEL>
struct DpRule {
  using Finish = DpFinish;
  Finish f;
  const int32_t* sel;   // [M] row ids (SEL), else rows 0..M-1
  const float* c;       // [M]
  __device__ __forceinline__ Acc<1> fold(const float* __restrict__ W, int64_t stride, const Finish::Ctx& cx, int k0,
                                         int k1, bool) const {
    return fold_range_clamped<SEL>(W, stride, sel, DpTerm{{c}, cx.x}, k0, k1);
  }
};

// ---- checks and launches ---------------------------------------------------------------------------------
#define DP_REQUIRE(cond, msg)                                                  \
  do {                                                                         \
    if (!(cond)) return ::fs::fail(FS_EINVAL, std::string(fn) + ": " + (msg)); \
  } while (0)

static int dp_check_rows(const char* fn, const float* d_W_all, int64_t stride, int M, int64_t len,
                         const float* d_W_g) {
  DP_REQUIRE(M >= 1, "M must be >= 1");
  DP_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  DP_REQUIRE(len / 4 <= 0xffffffffLL, "len must be below 2^34 (the noise counter is 32 bits of float4 positions)");
  DP_REQUIRE(d_W_all && d_W_g, "null pointer");
  return FS_OK;
}

static int dp_check_rule(const char* fn, double S, double z, int adaptive, double gamma, double eta, double sigma_b,
                         int t, const double* d_clip) {
  DP_REQUIRE(S > 0.0, "the clip S must be > 0 (+Inf: no clipping)");
  DP_REQUIRE(z >= 0.0 && z <= DP_DBL_MAX, "the noise multiplier z must be finite and >= 0");
  DP_REQUIRE(z == 0.0 || S <= DP_DBL_MAX, "noise (z > 0) needs a finite clip");
  DP_REQUIRE(t >= 0, "t must be >= 0");
  if (adaptive) {
    DP_REQUIRE(d_clip, "the adaptive clip needs d_clip");
    DP_REQUIRE(S <= DP_DBL_MAX, "the adaptive clip needs a finite clip");
    DP_REQUIRE(gamma >= 0.0 && gamma <= 1.0, "the adaptive quantile must be in [0, 1]");
    DP_REQUIRE(eta >= 0.0 && eta <= DP_DBL_MAX, "the adaptive lr must be finite and >= 0");
    DP_REQUIRE(sigma_b >= 0.0 && sigma_b <= DP_DBL_MAX, "the adaptive count noise must be finite and >= 0");
  }
  return FS_OK;
}
#undef DP_REQUIRE

static int dp_norms_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                           const float* d_W_g, double* d_n, float* nt, hipStream_t st) {
  const int64_t len4 = len / 4;
  const dim3 grid((unsigned)((len4 + 255) / 256), (unsigned)((M + 7) / 8));
  if (d_sel)
    hipLaunchKernelGGL(dp_norms_kernel<true>, grid, dim3(256), 0, st, d_W_all, stride, d_sel, M, len4, d_W_g, nt);
  else
    hipLaunchKernelGGL(dp_norms_kernel<false>, grid, dim3(256), 0, st, d_W_all, stride, d_sel, M, len4, d_W_g, nt);
  hipLaunchKernelGGL(dp_norms_sum_kernel, dim3((unsigned)M), dim3(256), 0, st, nt, dp_cols(len4), M, d_n);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

static DpParams dp_params(double S, double z, uint64_t seed, int t, int adaptive, double gamma, double eta,
                          double sigma_b) {
  return {S, z, (uint32_t)t, (uint32_t)seed, (uint32_t)(seed >> 32), adaptive ? 1 : 0, gamma, eta, sigma_b};
}

static int dp_coef_launch(const double* d_n, const float* d_q, int M, const DpParams& p, double* d_clip, float* d_c,
                          double* d_r, double* d_state, hipStream_t st) {
  hipLaunchKernelGGL(dp_coef_kernel, dim3(1), dim3(256), 0, st, d_n, d_q, (float)(1.0 / (double)M), M, p, d_clip, d_c,
                     d_r, d_state);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int aggregate_dp_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                        int64_t len, double S, double z, uint64_t seed, int t, int adaptive, double gamma, double eta,
                        double sigma_b, double* d_clip, int64_t cols_ld, int64_t cols_d, float* d_W_g, float* d_c,
                        double* d_r, double* d_state, float* d_ws, int64_t ws_floats, int chunks, void* d_sws,
                        int64_t sws_bytes, const EvalFinalize* fin, hipStream_t st) {
  const char* fn = "fs_aggregate_dp";
  int rc = dp_check_rows(fn, d_W_all, stride, M, len, d_W_g);
  if (rc != FS_OK) return rc;
  rc = dp_check_rule(fn, S, z, adaptive, gamma, eta, sigma_b, t, d_clip);
  if (rc != FS_OK) return rc;
  FS_REQUIRE(d_c && d_r && d_state && d_sws, "null pointer");
  FS_REQUIRE(cols_ld == 0 || (cols_ld >= 4 && cols_ld % 4 == 0 && len % cols_ld == 0 && cols_d >= 1 && cols_d <= cols_ld),
             "cols_ld must be 0 or a multiple of 4 that divides len, with 1 <= cols_d <= cols_ld");
  FS_REQUIRE(sws_bytes >= aggregate_dp_ws_bytes(M, len), "d_sws is too small (fs_aggregate_dp_ws_bytes(M, len))");
  double* n = reinterpret_cast<double*>(d_sws);
  float* nt = reinterpret_cast<float*>(n + M);
  rc = dp_norms_launch(d_W_all, stride, d_sel, M, len, d_W_g, n, nt, st);
  if (rc != FS_OK) return rc;
  const DpParams p = dp_params(S, z, seed, t, adaptive, gamma, eta, sigma_b);
  rc = dp_coef_launch(n, d_q, M, p, d_clip, d_c, d_r, d_state, st);
  if (rc != FS_OK) return rc;
  const DpFinish f{d_W_g, d_state, p.t, p.k0, p.k1, z > 0.0 ? 1 : 0, cols_ld, cols_d};
  if (d_sel) return fold_dispatch(d_W_all, stride, DpRule<true>{f, d_sel, d_c}, M, len, d_ws, ws_floats, chunks, fin, st);
  return fold_dispatch(d_W_all, stride, DpRule<false>{f, d_sel, d_c}, M, len, d_ws, ws_floats, chunks, fin, st);
}

}  // namespace fs

using namespace fs;

extern "C" int64_t fs_aggregate_dp_ws_bytes(int M, int64_t len) { return aggregate_dp_ws_bytes(M, len); }

extern "C" int fs_dp_norms(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                           const float* d_W_g, double* d_n, void* d_sws, int64_t sws_bytes, void* stream) {
  const int rc = dp_check_rows("fs_dp_norms", d_W_all, stride, M, len, d_W_g);
  if (rc != FS_OK) return rc;
  FS_REQUIRE(d_n && d_sws, "null pointer");
  FS_REQUIRE(sws_bytes >= aggregate_dp_ws_bytes(M, len), "d_sws is too small (fs_aggregate_dp_ws_bytes(M, len))");
  float* nt = reinterpret_cast<float*>(reinterpret_cast<double*>(d_sws) + M);
  return dp_norms_launch(d_W_all, stride, d_sel, M, len, d_W_g, d_n, nt, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_dp_coef(const double* d_n, const float* d_q, int M, double S, double z, uint64_t seed, int t,
                          int adaptive, double gamma, double eta, double sigma_b, double* d_clip, float* d_c,
                          double* d_r, double* d_state, void* stream) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  const int rc = dp_check_rule("fs_dp_coef", S, z, adaptive, gamma, eta, sigma_b, t, d_clip);
  if (rc != FS_OK) return rc;
  FS_REQUIRE(d_n && d_c && d_r && d_state, "null pointer");
  return dp_coef_launch(d_n, d_q, M, dp_params(S, z, seed, t, adaptive, gamma, eta, sigma_b), d_clip, d_c, d_r,
                        d_state, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_dp_noise(uint64_t seed, int t, int noise_stream, int64_t len, float* d_g, void* stream) {
  FS_REQUIRE(len >= 4 && len % 4 == 0 && len / 4 <= 0xffffffffLL, "len must be a multiple of 4 below 2^34");
  FS_REQUIRE(t >= 0 && noise_stream >= 0, "t and the stream must be >= 0");
  FS_REQUIRE(d_g, "null pointer");
  const int64_t len4 = len / 4;
  hipLaunchKernelGGL(dp_noise_kernel, dim3((unsigned)((len4 + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (uint32_t)t, (uint32_t)noise_stream, (uint32_t)seed,
                     (uint32_t)(seed >> 32), len4, d_g);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" int fs_aggregate_dp(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                               int64_t len, double S, double z, uint64_t seed, int t, int adaptive, double gamma,
                               double eta, double sigma_b, double* d_clip, int64_t cols_ld, int64_t cols_d,
                               float* d_W_g, float* d_c, double* d_r, double* d_state, float* d_ws, int64_t ws_floats,
                               int chunks, void* d_sws, int64_t sws_bytes, void* stream) {
  return aggregate_dp_launch(d_W_all, stride, d_sel, d_q, M, len, S, z, seed, t, adaptive, gamma, eta, sigma_b, d_clip,
                             cols_ld, cols_d, d_W_g, d_c, d_r, d_state, d_ws, ws_floats, chunks, d_sws, sws_bytes, nullptr,
                             reinterpret_cast<hipStream_t>(stream));
}

// fs_aggregate_krum: Krum and Multi-Krum (Blanchard, El Mhamdi, Guerraoui, Stainer, NeurIPS 2017) over
// the M rows d_sel (NULL: rows 0..M-1) of d_W_all.  The first aggregate here that is bound by the
// matrix pipe: the M x M squared distances between the rows are a symmetric rank-len update of the
// centred rows U_k = fl(W_k - x).  The rule, its orders and the bound: include/fedsim.h.
//
// Stage 1, fs_krum_distances, two launches.
//   krum_gram_kernel.  A 256-thread workgroup (one wave per SIMD, two workgroups per CU) owns one
//     128 x 128 tile pair (ti <= tj) of G = U U^T and one of S slices of the contraction (split-K:
//     at M = 100 there is one tile pair, so the len axis is what fills the chip).  Per K-step of 32
//     it stages the 128 B of its 128 + 128 rows (128 on a diagonal tile: one image serves both
//     operands) through registers, subtracts x there -- no centred copy exists in HBM -- and writes
//     the 16-B chunk c of row r at slot c ^ ((r >> 1) & 7), so that the ds_read_b128 of a 32-row
//     block covers the banks once (mix_z.hip's image).  Two LDS buffers: the loads of step k + 1 are
//     in flight under the 64 MFMAs (v_mfma_f32_32x32x2_f32) of step k; one barrier per step.  Each
//     wave owns 64 x 64 of the tile.  No load stands under a condition: a row past M is row M - 1
//     again, a chunk past the slice's end is chunk 0 again and replaced by zeros in registers.
//     The partial tile goes to the workspace as [slice][pair][128][128].
//     Workgroup -> (slice, pair): blocks b and b + 8 share an XCD, so each XCD gets one contiguous
//     run of the slice-major list: the workgroups it runs at once are neighbouring tile pairs of one
//     slice and share their row panels in its L2.
//   krum_dist_kernel.  16 workgroups per tile pair, 8 rows each: G_ab and the diagonal entries it
//     needs are the sums of their S partials in ascending slice order (8 loads in flight per
//     element: with one tile pair and a hundred slices this launch is a chain of load latencies),
//     D from them, the triangle written directly and mirrored through an LDS transpose.  A diagonal
//     tile is used above its diagonal only.
// Stage 2, fs_krum_select, three launches.
//   krum_score_kernel.  One workgroup per row a: the row's bits into LDS, an 8-pass radix select
//     (4-bit digits, most significant first) of rank n among the b != a; the digit counts are wave
//     ballots summed in scalar registers, joined over the 4 waves through LDS -- no atomics.  Then
//     the slices' double sums and the fixed tree.
//   krum_rank_kernel.  16 rows per workgroup, 16 threads per row: the row's rank under (score,
//     position), each thread counting over a sixteenth of the scores, joined by shuffles.
//   krum_pick_kernel.  One workgroup of 1024 threads: a block prefix sum of the flags rank < m, the
//     ids out in ascending position, and the fold's m weights f32(1 / m).
// Then the gathered fold, aggregate_sel_launch, with the pending finaliser of a deferred evaluation.
#include "aggregate_sel.h"
#include "common.h"
#include "finalize.h"

namespace fs {

#pragma clang fp contract(off)

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int KR_MAX_M = 5120;                 // rows: the score kernel's LDS row; 5 ids per thread of the pick kernel
constexpr int KR_T = 128;                      // rows of a tile
constexpr int KR_BK = 32;                      // floats of a K-step
constexpr int KR_ROWB = KR_BK * 4;             // 128 B per row per K-step
constexpr int KR_IMG = KR_T * KR_ROWB;         // 16 KB: one operand's image
constexpr int KR_TILE = KR_T * KR_T;           // floats of a partial tile
constexpr int KR_MIN_STEPS = 8;                // K-steps a slice has at least
constexpr int KR_TARGET_WG = 512;              // workgroups the split aims at (two per CU)
constexpr int KR_RB = 8;                       // rows of a tile one krum_dist_kernel workgroup forms
constexpr int KR_GRP = 8;                      // partial loads in flight per element
constexpr int KR_PICK_NT = 1024;

struct KrumGeom {
  int T, P, S, kc;                             // tiles per side, tile pairs, slices, K-steps per slice
};

// the split: a function of M and len alone (never of the device), so the bits are too
__host__ __device__ inline KrumGeom krum_geom(int M, int64_t len) {
  KrumGeom g;
  g.T = (M + KR_T - 1) / KR_T;
  g.P = g.T * (g.T + 1) / 2;
  const int64_t nk = (len + KR_BK - 1) / KR_BK;
  const int64_t smax = KR_TARGET_WG / g.P > 1 ? KR_TARGET_WG / g.P : 1;
  int64_t kc = (nk + smax - 1) / smax;
  if (kc < KR_MIN_STEPS) kc = KR_MIN_STEPS;
  g.kc = (int)kc;
  g.S = (int)((nk + kc - 1) / kc);
  return g;
}

__host__ __device__ inline int krum_ldd(int M) { return (M + 3) & ~3; }

// tile pair p of the row-by-row list (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void krum_pair(int p, int T, int& ti, int& tj) {
  int row = 0, n = T;
  while (p >= n) {
    p -= n;
    ++row;
    --n;
  }
  ti = row;
  tj = row + p;
}
__device__ __forceinline__ int krum_diag_pair(int t, int T) { return t * T - t * (t - 1) / 2; }

__device__ __forceinline__ floatx16 kr_mfma(float a, float b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float4 kr_centre(float4 w, float4 x, bool valid) {
  float4 u;
  u.x = valid ? w.x - x.x : 0.f;
  u.y = valid ? w.y - x.y : 0.f;
  u.z = valid ? w.z - x.z : 0.f;
  u.w = valid ? w.w - x.w : 0.f;
  return u;
}

// one K-step's MFMAs from one buffer: lane (row lr of a 32-row block, half h) reads chunk 2 kq + h,
// so MFMA (kq, j) adds the products of k = 8 kq + j (h = 0) and k = 8 kq + 4 + j (h = 1)
__device__ __forceinline__ void kr_kstep(const char* buf, int a_off, int b_off, const int (&frag)[4],
                                         floatx16 (&acc)[2][2]) {
#pragma unroll
  for (int kq = 0; kq < 4; ++kq) {
    float4 a[2], b[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) a[mb] = *reinterpret_cast<const float4*>(buf + a_off + mb * 32 * KR_ROWB + frag[kq]);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) b[nb] = *reinterpret_cast<const float4*>(buf + b_off + nb * 32 * KR_ROWB + frag[kq]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = kr_mfma(comp(a[mb], j), comp(b[nb], j), acc[mb][nb]);
  }
}

template <bool SEL>
__global__ __launch_bounds__(256, 2) void krum_gram_kernel(const float* __restrict__ Wall, int64_t stride,
                                                           const int32_t* __restrict__ sel, int M, int64_t len,
                                                           const float* __restrict__ x, int T, int P, int S, int kc,
                                                           float* __restrict__ part) {
  __shared__ __attribute__((aligned(1024))) char lds0[2 * KR_IMG];
  __shared__ __attribute__((aligned(1024))) char lds1[2 * KR_IMG];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

  // ---- this workgroup's (slice, pair): a contiguous run of the slice-major list per XCD ----
  const int total = P * S;
  const int bx = blockIdx.x, xcd = bx & 7, idx = bx >> 3;
  const int base = total >> 3, rem = total & 7;
  const int t = xcd * base + min(xcd, rem) + idx;
  const int s = t / P, p = t - s * P;
  int ti, tj;
  krum_pair(p, T, ti, tj);
  const bool diag = ti == tj;

  // ---- staging: thread (chunk c, rows r0 + 32 i) of either operand ----
  const int c = tid & 7, r0 = tid >> 3;
  const float* srcA[4];
  const float* srcB[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ka = min(ti * KR_T + r0 + 32 * i, M - 1), kb = min(tj * KR_T + r0 + 32 * i, M - 1);
    srcA[i] = Wall + (int64_t)(SEL ? sel[ka] : ka) * stride;
    srcB[i] = Wall + (int64_t)(SEL ? sel[kb] : kb) * stride;
  }
  const int dst = r0 * KR_ROWB + ((c ^ ((r0 >> 1) & 7)) << 4);   // + 32 i rows: the swizzle term is the same

  // ---- fragments ----
  const int wm = w >> 1, wn = w & 1, lr = lane & 31, h = lane >> 5;
  int frag[4];
#pragma unroll
  for (int kq = 0; kq < 4; ++kq) frag[kq] = lr * KR_ROWB + (((2 * kq + h) ^ ((lr >> 1) & 7)) << 4);
  const int a_off = (wm * 64) * KR_ROWB;
  const int b_off = (diag ? 0 : KR_IMG) + (wn * 64) * KR_ROWB;

  floatx16 acc[2][2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

  const int64_t k0 = (int64_t)s * kc * KR_BK;
  const int64_t kend = min(k0 + (int64_t)kc * KR_BK, len);
  const int steps = (int)((kend - k0 + KR_BK - 1) / KR_BK);      // >= 1: S = ceil(nk / kc)

  float4 ra[4], rb[4], rx;
  bool valid;
  auto fetch = [&](int st) {
    const int64_t kk = k0 + (int64_t)st * KR_BK + 4 * c;
    valid = kk < kend;                      // (len and the slice bounds are multiples of 4)
    const int64_t kl = valid ? kk : 0;
    rx = ld4(x + kl);
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = ld4(srcA[i] + kl);
    if (!diag) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rb[i] = ld4(srcB[i] + kl);
    }
  };
  auto stage = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<float4*>(buf + dst + i * 32 * KR_ROWB) = kr_centre(ra[i], rx, valid);
    if (!diag) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(buf + KR_IMG + dst + i * 32 * KR_ROWB) = kr_centre(rb[i], rx, valid);
    }
  };

  fetch(0);
  stage(lds0);
  for (int st = 0; st < steps; st += 2) {
    __syncthreads();
    if (st + 1 < steps) fetch(st + 1);
    kr_kstep(lds0, a_off, b_off, frag, acc);
    if (st + 1 < steps) stage(lds1);
    __syncthreads();
    if (st + 1 < steps) {
      if (st + 2 < steps) fetch(st + 2);
      kr_kstep(lds1, a_off, b_off, frag, acc);
      if (st + 2 < steps) stage(lds0);
    }
  }

  // ---- the partial tile: D[i][j] of a 32 x 32 block, reg r: i = (r & 3) + 8 (r >> 2) + 4 h, j = lane & 31 ----
  float* out = part + ((int64_t)s * P + p) * KR_TILE;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = wm * 64 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const int j = wn * 64 + nb * 32 + lr;
        out[i * KR_T + j] = acc[mb][nb][r];
      }
}

__device__ __forceinline__ float krum_partial_sum(const float* __restrict__ part, int P, int S, int p, int e) {
  const float* q = part + (int64_t)p * KR_TILE + e;
  const int64_t step = (int64_t)P * KR_TILE;
  float g = q[0];
  for (int s0 = 1; s0 < S; s0 += KR_GRP) {
    float v[KR_GRP];
#pragma unroll
    for (int u = 0; u < KR_GRP; ++u) v[u] = q[(int64_t)min(s0 + u, S - 1) * step];   // clamped: the add is guarded
#pragma unroll
    for (int u = 0; u < KR_GRP; ++u)
      if (s0 + u < S) g += v[u];
  }
  return g;
}

__global__ __launch_bounds__(256) void krum_dist_kernel(const float* __restrict__ part, int M, int T, int P, int S,
                                                        float* __restrict__ D, int ldD) {
  __shared__ float dgr[KR_RB], dgc[KR_T];
  __shared__ float tile[KR_RB][KR_T + 1];
  const int tid = threadIdx.x;
  const int p = blockIdx.x / (KR_T / KR_RB), rb = blockIdx.x % (KR_T / KR_RB);
  int ti, tj;
  krum_pair(p, T, ti, tj);
  if (tid < KR_RB + KR_T) {
    const bool isrow = tid < KR_RB;
    const int i = isrow ? rb * KR_RB + tid : tid - KR_RB;
    const float g = krum_partial_sum(part, P, S, krum_diag_pair(isrow ? ti : tj, T), i * KR_T + i);
    if (isrow) dgr[tid] = g;
    else dgc[tid - KR_RB] = g;
  }
  __syncthreads();
  {
    const int j = tid & (KR_T - 1);
#pragma unroll
    for (int u = 0; u < KR_RB / 2; ++u) {
      const int il = (tid >> 7) + 2 * u, i = rb * KR_RB + il;
      const float g = krum_partial_sum(part, P, S, p, i * KR_T + j);
      float d = (dgr[il] + dgc[j]) - 2.f * g;
      if ((__float_as_uint(d) & 0x7F800000u) == 0x7F800000u) d = __uint_as_float(0x7F800000u);   // NaN, +-Inf
      d = fmaxf(d, 0.f);
      tile[il][j] = d;
      const int a = ti * KR_T + i, b = tj * KR_T + j;
      if (a < M && b < M) {
        if (ti < tj || i < j) D[(int64_t)a * ldD + b] = d;
        else if (i == j) D[(int64_t)a * ldD + a] = 0.f;
      }
    }
  }
  __syncthreads();
  {
    const int il = tid & (KR_RB - 1), i = rb * KR_RB + il;
#pragma unroll
    for (int u = 0; u < KR_T / (256 / KR_RB); ++u) {
      const int j = tid / KR_RB + (256 / KR_RB) * u;
      const int a = ti * KR_T + i, b = tj * KR_T + j;
      if (a < M && b < M && (ti < tj || i < j)) D[(int64_t)b * ldD + a] = tile[il][j];
    }
  }
}

// ---- stage 2 ----
__global__ __launch_bounds__(256) void krum_score_kernel(const float* __restrict__ D, int ldD, int M, int n,
                                                         double* __restrict__ score) {
  __shared__ uint32_t keys[KR_MAX_M];
  __shared__ int wh[4][16];
  __shared__ double part[256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int a = blockIdx.x;
  const float* row = D + (int64_t)a * ldD;
  for (int b = tid; b < M; b += 256) keys[b] = __float_as_uint(row[b]);
  __syncthreads();
  uint32_t prefix = 0;
  int rem = n;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 28 - 4 * pass;
    const uint32_t mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 4));
    int cnt[16];                           // this wave's digit counts: uniform, in scalar registers
#pragma unroll
    for (int j = 0; j < 16; ++j) cnt[j] = 0;
    for (int b0 = w * 64; b0 < M; b0 += 256) {
      const int b = b0 + lane;
      const uint32_t key = keys[min(b, M - 1)];
      const bool in = b < M && b != a && ((key ^ prefix) & mask) == 0u;
      const int d = in ? (int)((key >> shift) & 15u) : 16;
#pragma unroll
      for (int j = 0; j < 16; ++j) cnt[j] += __popcll(__ballot(d == j));
    }
    {
      int mine = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) mine = lane == j ? cnt[j] : mine;
      if (lane < 16) wh[w][lane] = mine;
    }
    __syncthreads();
    int cum = 0, dsel = 15, before = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int cj = wh[0][j] + wh[1][j] + wh[2][j] + wh[3][j];
      if (!found && cum + cj >= rem) {
        found = true;
        dsel = j;
        before = cum;
      }
      cum += cj;
    }
    prefix |= (uint32_t)dsel << shift;
    rem -= before;
    __syncthreads();                       // the counts are read before the next pass writes them
  }
  // prefix: the bits at rank n; n - rem values lie strictly below it, rem copies of it are kept
  double acc = 0.0;
  for (int b = tid; b < M; b += 256) {
    const uint32_t key = keys[b];
    if (b != a && key < prefix) acc += (double)__uint_as_float(key);
  }
  part[tid] = acc;
  __syncthreads();
  for (int h2 = 1; h2 < 256; h2 *= 2) {
    if ((tid & (2 * h2 - 1)) == 0) part[tid] += part[tid + h2];
    __syncthreads();
  }
  if (tid == 0) score[a] = part[0] + (double)rem * (double)__uint_as_float(prefix);
}

// rank[a] = #{b : (s_b, b) < (s_a, a)}; the scores' bits order them (they are >= 0; NaN above +Inf)
__global__ __launch_bounds__(256) void krum_rank_kernel(const double* __restrict__ score, int M,
                                                        int32_t* __restrict__ rank) {
  const int tid = threadIdx.x, part = tid & 15;
  const int a = blockIdx.x * 16 + (tid >> 4), ac = min(a, M - 1);
  const unsigned long long sa = (unsigned long long)__double_as_longlong(score[ac]);
  int r = 0;
  for (int b0 = 0; b0 < M; b0 += 16 * KR_GRP) {
    unsigned long long sb[KR_GRP];
#pragma unroll
    for (int u = 0; u < KR_GRP; ++u)
      sb[u] = (unsigned long long)__double_as_longlong(score[min(b0 + 16 * u + part, M - 1)]);
#pragma unroll
    for (int u = 0; u < KR_GRP; ++u) {
      const int b = b0 + 16 * u + part;
      r += (b < M && (sb[u] < sa || (sb[u] == sa && b < ac))) ? 1 : 0;
    }
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
  if (part == 0 && a < M) rank[a] = r;
}

__global__ __launch_bounds__(KR_PICK_NT) void krum_pick_kernel(const int32_t* __restrict__ rank, int M, int m,
                                                               const int32_t* __restrict__ sel,
                                                               int32_t* __restrict__ pick, float* __restrict__ q,
                                                               float qv) {
  __shared__ int cnt[KR_PICK_NT];
  const int tid = threadIdx.x;
  const int per = (M + KR_PICK_NT - 1) / KR_PICK_NT;       // <= 5
  const int lo = min(tid * per, M), hi = min(lo + per, M);
  int mine = 0;
  for (int a = lo; a < hi; ++a) mine += rank[a] < m ? 1 : 0;
  cnt[tid] = mine;
  __syncthreads();
  for (int off = 1; off < KR_PICK_NT; off <<= 1) {
    const int v = tid >= off ? cnt[tid - off] : 0;
    __syncthreads();
    cnt[tid] += v;
    __syncthreads();
  }
  int pos = cnt[tid] - mine;
  for (int a = lo; a < hi; ++a)
    if (rank[a] < m && pos < m) pick[pos++] = sel ? sel[a] : a;
  if (q)
    for (int i = tid; i < m; i += KR_PICK_NT) q[i] = qv;
}

// ---- host ----
static int64_t krum_part_bytes(int M, int64_t len) {
  const KrumGeom g = krum_geom(M, len);
  return (int64_t)g.S * g.P * KR_TILE * 4;
}
// the partials of every M' <= M (the split follows the tile count, not M)
static int64_t krum_part_bytes_upto(int M, int64_t len) {
  int64_t best = 0;
  for (int t = 1; t <= (M + KR_T - 1) / KR_T; ++t) best = std::max(best, krum_part_bytes(std::min(t * KR_T, M), len));
  return best;
}
static int64_t krum_d_floats(int M) { return (int64_t)(M + 2) * krum_ldd(M); }   // D, the fold's weights, the ranks

static int krum_check_rows(const float* d_W_all, int64_t stride, int M, int64_t len, const float* d_x) {
  FS_REQUIRE(M >= 3, "M must be >= 3");
  FS_REQUIRE(M <= KR_MAX_M, "M is larger than fs_aggregate_krum_max_m()");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(len <= ((int64_t)1 << 40), "len too large");
  FS_REQUIRE(d_W_all && d_x, "null pointer");
  return FS_OK;
}
static int krum_check_fm(int M, int f, int m) {
  FS_REQUIRE(M >= 3, "M must be >= 3");
  FS_REQUIRE(M <= KR_MAX_M, "M is larger than fs_aggregate_krum_max_m()");
  FS_REQUIRE(f >= 0, "f must be >= 0");
  FS_REQUIRE(M - f - 2 >= 1, "M - f - 2 must be >= 1");
  FS_REQUIRE(m >= 1 && m <= M - f, "m must be in [1, M - f]");
  return FS_OK;
}

static int krum_distances_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                                 const float* d_x, float* d_D, float* d_part, hipStream_t st) {
  const KrumGeom g = krum_geom(M, len);
  const unsigned grid = (unsigned)(g.P * g.S);
  if (d_sel)
    hipLaunchKernelGGL(krum_gram_kernel<true>, dim3(grid), dim3(256), 0, st, d_W_all, stride, d_sel, M, len, d_x, g.T,
                       g.P, g.S, g.kc, d_part);
  else
    hipLaunchKernelGGL(krum_gram_kernel<false>, dim3(grid), dim3(256), 0, st, d_W_all, stride, d_sel, M, len, d_x,
                       g.T, g.P, g.S, g.kc, d_part);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(krum_dist_kernel, dim3((unsigned)(g.P * (KR_T / KR_RB))), dim3(256), 0, st, d_part, M, g.T, g.P,
                     g.S, d_D, krum_ldd(M));
  FS_LAUNCH_CHECK();
  return FS_OK;
}

static int krum_select_launch(const float* d_D, int M, int f, int m, const int32_t* d_sel, double* d_score,
                              int32_t* d_pick, float* d_q, int32_t* d_rank, hipStream_t st) {
  hipLaunchKernelGGL(krum_score_kernel, dim3((unsigned)M), dim3(256), 0, st, d_D, krum_ldd(M), M, M - f - 2, d_score);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(krum_rank_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, st, d_score, M, d_rank);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(krum_pick_kernel, dim3(1), dim3(KR_PICK_NT), 0, st, d_rank, M, m, d_sel, d_pick, d_q,
                     (float)(1.0 / (double)m));
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int aggregate_krum_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                          const float* d_x, int f, int m, float* d_out, int32_t* d_pick, double* d_score, void* d_ws,
                          int64_t ws_bytes, float* d_agg_ws, int64_t agg_ws_floats, int chunks,
                          const EvalFinalize* fin, hipStream_t st) {
  int rc = krum_check_rows(d_W_all, stride, M, len, d_x);
  if (rc != FS_OK) return rc;
  rc = krum_check_fm(M, f, m);
  if (rc != FS_OK) return rc;
  FS_REQUIRE(d_out && d_pick && d_score && d_ws, "null pointer");
  FS_REQUIRE(ws_bytes >= krum_d_floats(M) * 4 + krum_part_bytes(M, len), "the workspace is too small (fs_aggregate_krum_ws_bytes)");
  float* D = static_cast<float*>(d_ws);
  float* q = D + (int64_t)M * krum_ldd(M);
  int32_t* rank = reinterpret_cast<int32_t*>(q + krum_ldd(M));
  float* part = D + krum_d_floats(M);
  rc = krum_distances_launch(d_W_all, stride, d_sel, M, len, d_x, D, part, st);
  if (rc != FS_OK) return rc;
  rc = krum_select_launch(D, M, f, m, d_sel, d_score, d_pick, q, rank, st);
  if (rc != FS_OK) return rc;
  return aggregate_sel_launch(d_W_all, stride, d_pick, q, m, len, d_out, d_agg_ws, agg_ws_floats, chunks, fin, st);
}

int64_t aggregate_krum_ws_bytes(int M, int64_t len) {
  if (M < 1 || len < 1) return 0;
  return krum_d_floats(M) * 4 + krum_part_bytes_upto(M, len);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_krum_max_m(void) { return KR_MAX_M; }

extern "C" int fs_krum_split(int M, int64_t len, int* splits, int* ksteps) {
  FS_REQUIRE(M >= 1 && len >= 1 && splits && ksteps, "bad arguments");
  const KrumGeom g = krum_geom(M, len);
  *splits = g.S;
  *ksteps = g.kc;
  return FS_OK;
}

extern "C" int64_t fs_krum_distances_ws_bytes(int M, int64_t len) {
  return (M < 1 || len < 1) ? 0 : krum_part_bytes_upto(M, len);
}

extern "C" int64_t fs_aggregate_krum_ws_bytes(int M, int64_t len) { return aggregate_krum_ws_bytes(M, len); }

extern "C" int fs_krum_distances(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                                 const float* d_x, float* d_D, void* d_ws, int64_t ws_bytes, void* stream) {
  const int rc = krum_check_rows(d_W_all, stride, M, len, d_x);
  if (rc != FS_OK) return rc;
  FS_REQUIRE(d_D && d_ws, "null pointer");
  FS_REQUIRE(ws_bytes >= krum_part_bytes(M, len), "the workspace is too small (fs_krum_distances_ws_bytes)");
  return krum_distances_launch(d_W_all, stride, d_sel, M, len, d_x, d_D, static_cast<float*>(d_ws),
                               reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_krum_select(const float* d_D, int M, int f, int m, const int32_t* d_sel, double* d_score,
                              int32_t* d_pick, float* d_q, int32_t* d_rank, void* stream) {
  const int rc = krum_check_fm(M, f, m);
  if (rc != FS_OK) return rc;
  FS_REQUIRE(d_D && d_score && d_pick && d_rank, "null pointer");
  return krum_select_launch(d_D, M, f, m, d_sel, d_score, d_pick, d_q, d_rank, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_aggregate_krum(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                                 const float* d_x, int f, int m, float* d_out, int32_t* d_pick, double* d_score,
                                 void* d_ws, int64_t ws_bytes, float* d_agg_ws, int64_t agg_ws_floats, int chunks,
                                 void* stream) {
  return aggregate_krum_launch(d_W_all, stride, d_sel, M, len, d_x, f, m, d_out, d_pick, d_score, d_ws, ws_bytes,
                               d_agg_ws, agg_ws_floats, chunks, nullptr, reinterpret_cast<hipStream_t>(stream));
}

// fs_local_train_mse -- per-client local SGD under nn.MSELoss at ONE output column.
//
// Replaces train_loop's regression branch (the reference's functions/tools.py:177-215 with the
// criterion of tools.py:183-184) as called by FedAvg / FedProx / FedAMW / Centralized /
// Distributed / FedAMW_OneShot with type='regression', num_classes = 1.
//
// The model is a vector of ld floats, so none of the class-tiled MFMA forms fits: forward and
// backward are a GEMV and a rank-|b| update.  One 512-thread workgroup (8 waves) owns one
// client (parallel clients: grid N in LPT order) or walks the chain (chained clients) and runs
// all E * ceil(n_j / B) dependent steps without leaving the kernel.  No cross-workgroup
// exchange, no spin, no workspace.
//   weights   w lives in registers for the whole client: thread t owns the float4 column
//             groups t, t + 512, ... (NG of them, 1..8 -> ld <= 16384).  The thread that
//             accumulates grad[d] is the thread that holds w[d], so w never crosses lanes and
//             chained clients need no hand-off (the rule of local_train.hip:21-23).
//   forward   every thread loads its column slice of the shuffled rows (16 B per lane, a wave
//             reads 1 KB of contiguous bytes of one row per instruction) and FMAs into one
//             partial dot per row; a wave reduces its RC partial dots with a transposing
//             butterfly (RC + log2(64 / RC) - 1 shuffles instead of 6 RC), lane (r * 64 / RC)
//             writes row r's wave total to LDS; ONE barrier.
//   residual  every wave redundantly sums the 8 wave totals (lane r = row r, fixed order),
//             g_r = (2 / |b|) (o_r - y_r); the update reads g_r by v_readlane.
//   update    grad = sum_r g_r x_r, the rows in chunks of RC = 8 / NG (32 VGPRs of rows, ~100
//             VGPRs in all: two workgroups share a CU, which is what hides the load latency of
//             many short clients; larger chunks measured slower, see LM_RC_BASE).  Where the
//             batch is one chunk (KEEP: B <= RC) the update consumes the SAME row registers the
//             forward loaded; else each chunk is re-read (L2-resident by then).
//             w -= lr (grad + mu (w - w_a)/||w - w_a|| + lam w/||w||); the two squared norms for
//             the next step are reduced in the same pass (one LDS slot per wave, read after the
//             next step's barrier).  The prox anchor is re-read from L2.
//   early     the shuffle is fixed before the launch, so the next step's row addresses do not
//             depend on w: under KEEP the next step's rows are issued as soon as the gradient
//             pass has read the row registers -- ahead of the update, the norm reduction and
//             the next forward's first FMA, so HBM latency sits beside the dependent chain.
//             (A whole batch does not fit twice: 32 x 2048 floats are half of a CU's 512 KB
//             register file.  Beyond one chunk the overlap comes from the second workgroup on
//             the CU, not from loads issued before the barrier.)
// Rows >= |b| of a ragged batch read a valid row and get g_r = 0; padded columns D..ld-1 hold
// x = 0, w = 0 and stay exactly 0.
#include "common.h"
#include "mse_rows.h"

namespace fs {

constexpr int LM_WAVES = 8;
constexpr int LM_THREADS = LM_WAVES * kWave;
constexpr int LM_MAXB = 64;
constexpr int LM_WIN = 2048;   // shuffled (row, target) pairs of the client staged in LDS at once

struct LMParams {
  const float* phi;
  int64_t ld;
  const int64_t* row_off;
  const float* y;
  const int32_t* perms;
  const int32_t* order;
  int N, B, E;
  float lr, mu, lam;
  int prox, reg, chained;
  const float* W_start;
  float* W_out;
  double* loss;
};

struct LMShared {
  int erow[LM_WIN];                       // global feature row of each staged position
  float ey[LM_WIN];                       // its target
  float part[2][LM_WAVES][LM_MAXB];       // per-wave row totals, double-buffered by step parity
  float red[2][LM_WAVES][2];              // per-wave squared norms (prox, ridge) of the update
  float pro[LM_WAVES];
};

#ifndef LM_RC_BASE
#define LM_RC_BASE 8       // rows x float4 groups a thread holds at once (32 VGPRs of rows: ~100 VGPRs in
                           // all, so two workgroups share a CU.  Measured at the config-4 / config-2
                           // shapes, ms per launch: 4 -> 0.373 / 0.508, 8 -> 0.361 / 0.412, 16 -> 0.456 /
                           // 0.605, 32 (24 spilled VGPRs) -> 0.623 / 0.813)
#endif
#ifndef LM_KEEP
#define LM_KEEP 1
#endif
constexpr int lm_rc(int NG) { return LM_RC_BASE / NG > 0 ? LM_RC_BASE / NG : 1; }

template <int NG, bool KEEP>
__global__ __launch_bounds__(LM_THREADS) void local_train_mse_kernel(LMParams P) {
  constexpr int RC = lm_rc(NG);              // rows held in registers at once
  __shared__ LMShared sh;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int64_t ld = P.ld;
  const int ngrp = (int)(ld >> 2);           // float4 column groups of a row
  const int B = P.B;
  const int E = P.E;
  const int nclients = P.chained ? P.N : 1;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  int xoff[NG];
  bool vg[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int G = tid + LM_THREADS * g;
    vg[g] = G < ngrp;
    xoff[g] = vg[g] ? 4 * G : 0;
  }
  int it = 0;   // global step counter (parity of the double-buffered LDS slots)

  for (int k = 0; k < nclients; ++k) {
    const int j = P.chained ? k : (P.order ? P.order[blockIdx.x] : (int)blockIdx.x);
    const int64_t row0 = P.row_off[j];
    const int n = (int)(P.row_off[j + 1] - row0);
    const float* start = (P.chained && j > 0) ? P.W_out + (int64_t)(j - 1) * ld : P.W_start;
    const float* anchor = start;   // global_model = deepcopy(model)  (tools.py:180)
    float* Wj = P.W_out + (int64_t)j * ld;
    const int nb = (n + B - 1) / B;
    const int steps = E * nb;

    float4 wv[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) wv[g] = vg[g] ? ld4(start + xoff[g]) : zero4;

    if (steps == 0) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (vg[g]) st4(Wj + xoff[g], wv[g]);
      if (tid == 0) P.loss[j] = 0.0;
      __syncthreads();
      continue;
    }

    // ||w_start||^2 for the ridge term of the first step (the prox norm starts at 0)
    float wn2 = 0.f, pn2 = 0.f;
    if (P.reg) {
      float acc = 0.f;
#pragma unroll
      for (int g = 0; g < NG; ++g) acc = dot4(wv[g], wv[g], acc);
      acc = wave_sum(acc);
      if (lane == 0) sh.pro[w] = acc;
      __syncthreads();
      for (int i = 0; i < LM_WAVES; ++i) wn2 += sh.pro[i];
    }

    const int total = E * n;                 // the client's E shuffles are contiguous (engine.py layout)
    const int32_t* pp = P.perms + (int64_t)E * row0;
    int wbase = 0, wcnt = 0;                 // staged window [wbase, wbase + wcnt) of the flat shuffle
    float4 x[RC][NG];
    double lsum = 0.0;
    // stage the shuffled (row, target) pairs from flat position f on; called by every thread
    auto stage = [&](int f) {
      __syncthreads();                       // every wave is done with the previous window
      wbase = f;
      wcnt = min(LM_WIN, total - f);
      for (int i = tid; i < wcnt; i += LM_THREADS) {
        const int li = pp[f + i];
        sh.erow[i] = (int)(row0 + li);
        sh.ey[i] = P.y[row0 + li];
      }
      __syncthreads();
    };
    // this thread's column slice of chunk c of the batch at window position wp0 (bcx rows)
    auto load_rows = [&](int wp0, int bcx, int c) {
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        const int rr = c * RC + r;
        const int row = __builtin_amdgcn_readfirstlane(sh.erow[wp0 + (rr < bcx ? rr : 0)]);
        const float* xp = P.phi + (int64_t)row * ld;
#pragma unroll
        for (int g = 0; g < NG; ++g) x[r][g] = ld4(xp + xoff[g]);
      }
    };
    stage(0);
    if (KEEP) load_rows(0, min(B, n), 0);

    for (int st = 0; st < steps; ++st, ++it) {
      const int e = st / nb;
      const int s = st - e * nb;
      const int par = it & 1;
      const int bc = min(B, n - s * B);
      const int f = e * n + s * B;           // flat position of this batch
      const int wp = f - wbase;
      const int nch = KEEP ? 1 : (bc + RC - 1) / RC;   // KEEP: B <= RC, one chunk
      // the next step: the flat shuffle is consecutive across epochs
      const int f2 = f + bc;
      const int bc2 = (st + 1 < steps) ? min(B, n - ((s + 1 == nb) ? 0 : (s + 1) * B)) : 0;

      // ---------------- forward: o_r = x_r . w ----------------
      for (int c = 0; c < nch; ++c) {
        if (!KEEP) load_rows(wp, bc, c);
        float d[RC];
#pragma unroll
        for (int r = 0; r < RC; ++r) {
          float a = 0.f;
#pragma unroll
          for (int g = 0; g < NG; ++g) a = dot4(x[r][g], wv[g], a);
          d[r] = a;
        }
        const float tot = reduce_rows<RC>(d, lane);
        if ((lane & (64 / RC - 1)) == 0) sh.part[par][w][c * RC + ((lane * RC) >> 6)] = tot;
      }
      lds_barrier();   // the wave totals of this step; the previous step's norm partials

      if (st > 0) {
        pn2 = 0.f;
        wn2 = 0.f;
#pragma unroll
        for (int i = 0; i < LM_WAVES; ++i) {
          pn2 += sh.red[par ^ 1][i][0];
          wn2 += sh.red[par ^ 1][i][1];
        }
      }

      // ------- residual (every wave, lane r = row r; fixed-order sum of the wave totals) -------
      float gres = 0.f;
      {
        const bool valid = lane < bc;
        float o = 0.f;
#pragma unroll
        for (int i = 0; i < LM_WAVES; ++i) o += sh.part[par][i][lane];
        const float res = valid ? o - sh.ey[wp + (valid ? lane : 0)] : 0.f;
        gres = (2.0f / (float)bc) * res;               // d MSE_mean / d o  (tools.py:184, 210)
        if (e == E - 1 && w == 0) {
          const float sq = wave_sum(res * res);
          if (lane == 0) {
            float loss = sq / (float)bc;                       // nn.MSELoss(reduction='mean')
            if (P.prox) loss = loss + P.mu * sqrtf(pn2);       // + mu * ||w - w_a||   (tools.py:197, 203-205)
            if (P.reg) loss = loss + P.lam * sqrtf(wn2);       // + lambda * ||w||_F   (tools.py:201, 203, 207)
            lsum += (double)loss * (double)bc;                 // Meter.update(loss.item(), |b|)
          }
        }
      }

      // ---------------- backward + fused SGD/prox/ridge update ----------------
      float4 av[NG];
      if (P.prox) {
#pragma unroll
        for (int g = 0; g < NG; ++g) av[g] = vg[g] ? ld4(anchor + xoff[g]) : zero4;
      } else {
#pragma unroll
        for (int g = 0; g < NG; ++g) av[g] = zero4;
      }
      float4 ga[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) ga[g] = zero4;
      for (int c = 0; c < nch; ++c) {
        if (!KEEP) load_rows(wp, bc, c);
#pragma unroll
        for (int r = 0; r < RC; ++r) {
          const float gr = lane_value(gres, (c * RC + r) & 63);
#pragma unroll
          for (int g = 0; g < NG; ++g) ga[g] = fma4(gr, x[r][g], ga[g]);
        }
      }
      if (bc2 > 0) {
        if (f2 + bc2 > wbase + wcnt) stage(f2);   // (rare: a client with more than LM_WIN shuffled rows)
        // KEEP: the row registers are free, and the next step's row addresses depend on the
        // shuffle, not on w: its rows are issued here, ahead of the update, the norm reduction
        // and the next forward's first FMA
        if (KEEP) load_rows(f2 - wbase, bc2, 0);
      }
      const float sp = (P.prox && pn2 > 0.f) ? P.mu / sqrtf(pn2) : 0.f;
      const float sr = (P.reg && wn2 > 0.f) ? P.lam / sqrtf(wn2) : 0.f;
      const float lr = P.lr;
      float npn = 0.f, nwn = 0.f;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        float o[4];
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const float wc = comp(wv[g], e4);
          const float ac = comp(av[g], e4);
          float gr = comp(ga[g], e4);
          if (P.prox) gr = gr + (wc - ac) * sp;
          if (P.reg) gr = gr + wc * sr;
          o[e4] = vg[g] ? wc - lr * gr : 0.f;
          const float dp = o[e4] - ac;
          npn += dp * dp;
          nwn += o[e4] * o[e4];
        }
        wv[g] = make_float4(o[0], o[1], o[2], o[3]);
      }
      if (P.prox || P.reg) {
        npn = wave_sum(npn);
        nwn = wave_sum(nwn);
        if (lane == 0) {
          sh.red[par][w][0] = npn;
          sh.red[par][w][1] = nwn;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (vg[g]) st4(Wj + xoff[g], wv[g]);
    if (tid == 0) P.loss[j] = lsum / (double)n;
    __syncthreads();   // chained: the next client reads Wj (its own lanes' stores) and reuses the LDS
  }
}

template <int NG>
static void launch_lm(const LMParams& P, int grid, hipStream_t st) {
  constexpr int RC = lm_rc(NG);
  if (LM_KEEP && NG < 8 && P.B <= RC)   // (NG = 8: one row per chunk; nothing to keep)
    hipLaunchKernelGGL((local_train_mse_kernel<NG, true>), dim3(grid), dim3(LM_THREADS), 0, st, P);
  else
    hipLaunchKernelGGL((local_train_mse_kernel<NG, false>), dim3(grid), dim3(LM_THREADS), 0, st, P);
}

int local_train_mse(const float* d_phi, int64_t ld, const int64_t* d_row_off, const float* d_y,
                    const int32_t* d_perms, const int32_t* d_order, int N, int B, int E, float lr, float mu,
                    int prox, float lam, int reg, int chained, const float* d_W_start, float* d_W_out,
                    double* d_loss, hipStream_t st) {
  FS_REQUIRE(N >= 1, "N must be >= 1");
  FS_REQUIRE(d_phi && d_row_off && d_y && d_perms && d_W_start && d_W_out && d_loss, "null pointer");
  if (B < 1 || B > LM_MAXB) return fail(FS_EUNSUPPORTED, "fs_local_train_mse: batch_size must be in [1, 64]");
  if (E < 0) return fail(FS_EUNSUPPORTED, "fs_local_train_mse: epoch must be >= 0");
  if (ld < 64 || ld % 64 != 0 || ld > 16384)
    return fail(FS_EUNSUPPORTED, "fs_local_train_mse: ld must be a multiple of 64 in [64, 16384]");
  LMParams P{d_phi, ld, d_row_off, d_y, d_perms, d_order, N, B, E, lr, mu, lam,
             prox ? 1 : 0, reg ? 1 : 0, chained ? 1 : 0, d_W_start, d_W_out, d_loss};
  const int grid = chained ? 1 : N;
  const int groups = (int)((ld / 4 + LM_THREADS - 1) / LM_THREADS);
  if (groups <= 1) launch_lm<1>(P, grid, st);
  else if (groups <= 2) launch_lm<2>(P, grid, st);
  else if (groups <= 4) launch_lm<4>(P, grid, st);
  else launch_lm<8>(P, grid, st);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace fs

extern "C" int fs_local_train_mse(const float* d_phi, int64_t ld, const int64_t* d_row_off, const float* d_y,
                                  const int32_t* d_perms, const int32_t* d_order, int N, int B, int E, float lr,
                                  float mu, int prox, float lam, int reg, int chained, const float* d_W_start,
                                  float* d_W_out, double* d_loss, void* stream) {
  return fs::local_train_mse(d_phi, ld, d_row_off, d_y, d_perms, d_order, N, B, E, lr, mu, prox, lam, reg, chained,
                             d_W_start, d_W_out, d_loss, reinterpret_cast<hipStream_t>(stream));
}

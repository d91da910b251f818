// fs_mix_solve_mse -- FedAMW's mixture-weight SGD under nn.MSELoss at one output column.
//
// Replaces the p-SGD of the reference's functions/tools.py:441-453 (FedAMW, momentum 0.9,
// tools.py:423) and 304-316 (FedAMW_OneShot, momentum 0, tools.py:301) with the criterion of
// tools.py:421-422 / 299-300, on Z[v][n] = x_v . w_n as fs_mix_z writes it at C = 1
// ([n_val][ldN], ldN = N rounded up to 4, padding columns 0):
//   out_b = sum_n p_n Z[v_b][n];  L = mean_b (out_b - y_b)^2
//   grad_n = (2 / |b|) sum_b (out_b - y_b) Z[v_b][n]
//   buf = grad on the optimiser's very first step, else momentum * buf + grad;  p -= lr_p * buf
//
// One persistent 4-wave workgroup.  p and buf are lane-owned in registers (thread t owns the
// float4 client groups t, t + 256, ...: NG = 1, 2, 4 -> N <= 4096).  Per step every thread
// loads its slice of the |b| Z rows (16 B per lane, a wave reads contiguous bytes of a row),
// FMAs into |b| partial dots, a transposing butterfly reduces them in-wave, lane-indexed wave
// totals go through LDS with one barrier; every wave redundantly forms the residuals (lane b =
// row b) and the gradient pass reads them by v_readlane.  Where the batch fits the registers
// twice (KEEP: Bv <= 16 / NG rows) the NEXT step's Z rows are issued before the barrier -- they
// depend on the shuffle, not on p -- and the gradient pass consumes the rows the forward
// loaded; otherwise the rows are re-read (L2-resident).  The shuffled row index and target of
// the next step are fetched ahead as well (lane b = row b; the index two steps ahead).
#include "common.h"
#include "mse_rows.h"

namespace fs {

constexpr int MM_WAVES = 4;
constexpr int MM_THREADS = MM_WAVES * kWave;
constexpr int MM_MAXB = 64;
constexpr int MM_MAXN = 4096;

template <int NG, bool KEEP>
__global__ __launch_bounds__(MM_THREADS) void mix_solve_mse_kernel(const float* __restrict__ Z,
                                                                   const float* __restrict__ y,
                                                                   const int32_t* __restrict__ perms, int N,
                                                                   int n_val, int epochs, int Bv, float lr_p,
                                                                   float momentum, float* __restrict__ p_io,
                                                                   float* __restrict__ buf_io, int* first_flag) {
  constexpr int RC = 16 / NG;               // rows held in registers at once (twice under KEEP)
  __shared__ float part[2][MM_WAVES][MM_MAXB];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int ldN = (N + 3) & ~3;
  const int ngrp = ldN >> 2;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  int first = *first_flag;
  const int nb = (n_val + Bv - 1) / Bv;
  const int total = epochs * nb;

  int xoff[NG];
  bool vg[NG];
  float4 pv[NG], bv[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int G = tid + MM_THREADS * g;
    vg[g] = G < ngrp;
    xoff[g] = vg[g] ? 4 * G : 0;
    float pe[4], be[4];
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      const int nidx = 4 * G + e4;
      const bool ok = vg[g] && nidx < N;     // d_p / d_buf hold N floats, not ldN
      pe[e4] = ok ? p_io[nidx] : 0.f;
      be[e4] = ok ? buf_io[nidx] : 0.f;
    }
    pv[g] = make_float4(pe[0], pe[1], pe[2], pe[3]);
    bv[g] = make_float4(be[0], be[1], be[2], be[3]);
  }
  if (total == 0) return;

  // lane b = row b of the step: its validation row and target, fetched one step ahead
  auto step_bc = [&](int st) { return min(Bv, n_val - (st % nb) * Bv); };
  auto step_pos = [&](int st) { return (int64_t)(st / nb) * n_val + (int64_t)(st % nb) * Bv; };
  int bc = step_bc(0);
  int vcur = perms[step_pos(0) + min(lane, bc - 1)];
  float ycur = y[vcur];
  // the shuffled index is fetched TWO steps ahead (its dependants -- the target and the Z rows of
  // the next step -- are issued one step ahead, so no step waits for an index load)
  int vnext = total > 1 ? perms[step_pos(1) + min(lane, step_bc(1) - 1)] : vcur;

  float4 x[RC][NG], xn[KEEP ? RC : 1][NG];
  if (KEEP) {
#pragma unroll
    for (int r = 0; r < RC; ++r) {
      const int v = __builtin_amdgcn_readlane(vcur, r);
      const float* zp = Z + (int64_t)v * ldN;
#pragma unroll
      for (int g = 0; g < NG; ++g) x[r][g] = ld4(zp + xoff[g]);
    }
  }

  for (int st = 0; st < total; ++st) {
    const int par = st & 1;
    const int nch = (bc + RC - 1) / RC;
    const bool has_next = st + 1 < total;
    const int bc2 = has_next ? step_bc(st + 1) : 1;
    int vn2 = vnext;
    if (st + 2 < total) vn2 = perms[step_pos(st + 2) + min(lane, step_bc(st + 2) - 1)];
    const float ynext = has_next ? y[vnext] : ycur;

    // ---------------- forward: out_b = Z[v_b] . p ----------------
    for (int c = 0; c < nch; ++c) {
      if (!KEEP) {
#pragma unroll
        for (int r = 0; r < RC; ++r) {
          const int v = __builtin_amdgcn_readlane(vcur, (c * RC + r) & 63);   // lanes >= bc hold row bc - 1
          const float* zp = Z + (int64_t)v * ldN;
#pragma unroll
          for (int g = 0; g < NG; ++g) x[r][g] = ld4(zp + xoff[g]);
        }
      }
      float d[RC];
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        float a = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) a = dot4(x[r][g], pv[g], a);
        d[r] = a;
      }
      const float tot = reduce_rows<RC>(d, lane);
      if ((lane & (64 / RC - 1)) == 0) part[par][w][c * RC + ((lane * RC) >> 6)] = tot;
    }
    if (KEEP && has_next) {
      // the next step's Z rows: they depend on the shuffle, not on p
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        const int v = __builtin_amdgcn_readlane(vnext, r);
        const float* zp = Z + (int64_t)v * ldN;
#pragma unroll
        for (int g = 0; g < NG; ++g) xn[r][g] = ld4(zp + xoff[g]);
      }
    }
    lds_barrier();

    // ------- residual (every wave, lane b = row b; fixed-order sum of the wave totals) -------
    float o = 0.f;
#pragma unroll
    for (int i = 0; i < MM_WAVES; ++i) o += part[par][i][lane];
    const float res = lane < bc ? o - ycur : 0.f;
    const float gres = (2.0f / (float)bc) * res;        // d MSE_mean / d out_b

    // ---------------- grad_n = sum_b g_b Z[v_b][n], momentum, step ----------------
    float4 ga[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) ga[g] = zero4;
    for (int c = 0; c < nch; ++c) {
      if (!KEEP) {
#pragma unroll
        for (int r = 0; r < RC; ++r) {
          const int v = __builtin_amdgcn_readlane(vcur, (c * RC + r) & 63);
          const float* zp = Z + (int64_t)v * ldN;
#pragma unroll
          for (int g = 0; g < NG; ++g) x[r][g] = ld4(zp + xoff[g]);
        }
      }
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        const float gr = lane_value(gres, (c * RC + r) & 63);
#pragma unroll
        for (int g = 0; g < NG; ++g) ga[g] = fma4(gr, x[r][g], ga[g]);
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      float pe[4], be[4];
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const float gr = comp(ga[g], e4);
        // (lanes past ldN read group 0's columns: their p and buf stay 0 and add nothing to the dots)
        be[e4] = !vg[g] ? 0.f : (first ? gr : momentum * comp(bv[g], e4) + gr);   // torch.optim.SGD: buf = grad on step 1
        pe[e4] = !vg[g] ? 0.f : comp(pv[g], e4) - lr_p * be[e4];
      }
      bv[g] = make_float4(be[0], be[1], be[2], be[3]);
      pv[g] = make_float4(pe[0], pe[1], pe[2], pe[3]);
    }
    first = 0;
    if (KEEP && has_next) {
#pragma unroll
      for (int r = 0; r < RC; ++r)
#pragma unroll
        for (int g = 0; g < NG; ++g) x[r][g] = xn[r][g];
    }
    vcur = vnext;
    ycur = ynext;
    vnext = vn2;
    bc = bc2;
  }

#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (!vg[g]) continue;
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      const int nidx = xoff[g] + e4;
      if (nidx < N) {
        p_io[nidx] = comp(pv[g], e4);
        buf_io[nidx] = comp(bv[g], e4);
      }
    }
  }
  if (tid == 0) *first_flag = 0;
}

template <int NG>
static void launch_mm(int Bv, hipStream_t st, const float* Z, const float* y, const int32_t* perms, int N, int n_val,
                      int epochs, float lr_p, float momentum, float* p, float* buf, int* first) {
  if (Bv <= 16 / NG)
    hipLaunchKernelGGL((mix_solve_mse_kernel<NG, true>), dim3(1), dim3(MM_THREADS), 0, st, Z, y, perms, N, n_val,
                       epochs, Bv, lr_p, momentum, p, buf, first);
  else
    hipLaunchKernelGGL((mix_solve_mse_kernel<NG, false>), dim3(1), dim3(MM_THREADS), 0, st, Z, y, perms, N, n_val,
                       epochs, Bv, lr_p, momentum, p, buf, first);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_mix_solve_mse(const float* d_Z, const float* d_y, const int32_t* d_perms, int N, int n_val,
                                int epochs, int Bv, float lr_p, float momentum, float* d_p, float* d_buf,
                                int* d_first, void* d_ws, int64_t ws_bytes, void* stream) {
  FS_REQUIRE(N >= 1 && n_val >= 1 && epochs >= 0, "bad sizes");
  FS_REQUIRE(d_Z && d_y && d_perms && d_p && d_buf && d_first, "null pointer");
  if (Bv < 1 || Bv > MM_MAXB) return fail(FS_EUNSUPPORTED, "fs_mix_solve_mse: valid batch size must be in [1, 64]");
  if (N > MM_MAXN) return fail(FS_EUNSUPPORTED, "fs_mix_solve_mse: N must be <= 4096 (no multi-CU form)");
  (void)d_ws;       // one workgroup: no exchange, the error block stays clear
  (void)ws_bytes;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int groups = (((N + 3) >> 2) + MM_THREADS - 1) / MM_THREADS;
  if (groups <= 1) launch_mm<1>(Bv, st, d_Z, d_y, d_perms, N, n_val, epochs, lr_p, momentum, d_p, d_buf, d_first);
  else if (groups <= 2) launch_mm<2>(Bv, st, d_Z, d_y, d_perms, N, n_val, epochs, lr_p, momentum, d_p, d_buf, d_first);
  else launch_mm<4>(Bv, st, d_Z, d_y, d_perms, N, n_val, epochs, lr_p, momentum, d_p, d_buf, d_first);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

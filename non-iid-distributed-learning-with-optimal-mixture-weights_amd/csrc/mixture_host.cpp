// The host side of the FedAMW p-solve (fs_mix_solve, fs_mix_solve_blocked): which solver a
// shape gets, its geometry, the exchange workspace, the L2 prefetch helpers and every measured
// tuning policy -- one pure function, mix_plan -- and the launch that follows the plan.  Host
// code only (the kernels are in mixture.hip behind the launch_mix_* entry points of
// mixture_forms.h), so no kernel revision (_lib.source_revision) covers this file.
#include "mixture_forms.h"

namespace fs {

struct MixShape {
  int N, C, nv, epochs, Bv;
};

// Z and the perms within the 32-bit offsets of the buffer-descriptor solvers
static bool off32(const MixShape& s) {
  const int64_t zb = (int64_t)s.nv * s.C * mix_ldn(s.N) * 4;
  return zb < ((int64_t)1 << 31) && (int64_t)s.epochs * s.nv < ((int64_t)1 << 31);
}

// ---- geometry of the multi-CU solvers ---------------------------------------------------

static int64_t mc_xbytes(int K) { return (int64_t)sizeof(unsigned long long) * 2 * (K * MC_SLOT + MC_TOT); }

// exchange form: two hops, except at S = 8 (one) -- r02n, N = 100, C = 10, us per step, one hop /
// two hops (Z issued after the exchange): S = 64 (K = 2) 5.50 / 4.14, S = 32 (K = 4) 4.43 / 2.90,
// S = 16 (K = 7) 3.95 / 2.87, S = 8 (K = 13) 3.25 / 3.79
// (the next Z slice is issued after the exchange -- r02i, us per step, (hops, issued at the top /
// after hop 1 / after the exchange): N = 1000, C = 10, K = 32: (1, top) 6.61, (2, top) 6.03,
// (2, hop 1) 5.45, (2, exchange) 5.44; N = 300, C = 4, K = 19: 4.33 / 4.34 / 4.08 / 3.38)
static int mc_hops(int K, int S) { return (K >= 2 && S >= 16) ? 2 : 1; }

// the exchange kernels' spin bound (fs_tuning.spin_limit) and the injected-timeout test knob
// (the kernels report a timeout at the first exchange when the bound they get is 0)
static unsigned mc_spin_limit(const fs_tuning& t) {
  if (t.inject_timeout) return 0u;
  return t.spin_limit ? t.spin_limit : MC_SPIN_LIMIT;
}

// slice width for N clients (0: not covered): S clients per workgroup, K = ceil(ldN / S) <= 32
static int mc_slice(int N) {
  const int ldN = mix_ldn(N);
  for (int s : {8, 16, 32, 64})
    if ((ldN + s - 1) / s <= MC_KMAX && (s > 8 || ldN <= 128)) return s;
  return 0;
}

static int mc_k(int N) { return (mix_ldn(N) + mc_slice(N) - 1) / mc_slice(N); }

static bool mc_shape(int N, int C, int Bv) { return mc_slice(N) != 0 && C <= 16 && Bv <= 16; }

// the shapes qmc's exchange is laid out for (its workgroup bound depends on the lane width)
static bool qmc_shape(int N, int C, int Bv) { return N > 128 && C <= 16 && Bv <= 16; }

// qmc workgroups at nk clients per lane
static int qmc_k(int N, int nk) { return (mix_ldn(N) + 16 * nk - 1) / (16 * nk); }

// clients per lane: 4 (64 per workgroup) wherever K = ceil(N / 64) <= 16 workgroups, else 8
// (C <= 10 only).  Round 4 (profiles/r04/qmc_lane_ab*.txt, us per step, 8 vs 4): N = 1000
// C = 10 3.60-3.71 vs 3.30; N = 300 3.00 vs 2.50; N = 520 3.23 vs 2.73 -- half the gather per CU
// outweighs the hop's 16 partners since the hop re-polls all missing partners at once (round 2,
// polling them one after another, measured the two the same).  fs_tuning.mix_qmc_lane_clients
// forces one.
static int qmc_nk(int N, int C, const fs_tuning& t) {
  const int f = t.mix_qmc_lane_clients;
  if (C > 10 || f == 4) return 4;
  if (f == 8) return 8;
  return qmc_k(N, 4) <= QMC_KMAX ? 4 : 8;
}

// s_sleep(1) units before a step's first poll (fs_tuning.mix_poll_delay: 0 = by shape, -1 =
// none, n > 0 = n).  By shape from the sweeps (profiles/r04/qmc_poll_delay*.txt, us per step,
// none / best, at helper lead 6): N = 1000, C = 10 (K = 16) 3.24 / 2.73 at 14 (12-16 within 1 %);
// N = 1000, C = 4 2.86 / 2.28 at 8 (2.49 at 16); N = 300 2.41 / 1.95 at 8; N = 520 2.68 / 2.07 at 8.
// At lead 8 (the qmc default since) the K = 16 optimum moved to 10: 2.48 vs 2.58 us at 14
// (profiles/r04/qmc_delay_lead_grid.txt).
static int qmc_poll_delay(int K, int C, const fs_tuning& t) {
  if (t.mix_poll_delay < 0) return 0;
  if (t.mix_poll_delay > 0) return t.mix_poll_delay;
  return (K >= 12 && C >= 8) ? 10 : 8;
}

// ---- dynamic LDS of the LDS-resident solvers --------------------------------------------

// staged: two batches of Z rows + p, buf and the wave partials
static size_t staged_lds(const MixShape& s) {
  return sizeof(float) * (2 * (size_t)s.Bv * s.C * mix_ldn(s.N) + 2 * (size_t)s.N + (size_t)MS_WAVES * s.N);
}

static size_t global_lds(const MixShape& s) {
  return sizeof(float) * (2 * (size_t)s.N + 2 * MS_MAXB * (size_t)s.C) + sizeof(int) * 2 * MS_MAXB;
}

// ---- the solver table -------------------------------------------------------------------
// By shape: one wave for N <= 16, C <= 4; the quarter-wave solver (+ L2 prefetch helpers) for
// N <= 64, C <= 16 or N <= 128, C <= 10; the register solvers where an instance covers the
// shape (no cross-CU exchange: ~1-2.5 us per step); for N > 256 the multi-CU quarter-wave
// solver (one exchange hop per step; 3.9 us at N = 1000, C = 10) where it covers, else the
// multi-CU solver (two hops, ~4-7 us per step, 7-11x the single-workgroup staged / global
// solvers at N = 200..1000, C = 10); else those.

// one wave where it measured fastest (N <= 16, C = 3..4: 0.616 vs 0.62 us per step against quad)
static bool wave_auto(const MixShape& s) { return s.N <= 16 && s.C >= 3 && s.C <= 4 && s.Bv <= 16; }

struct MixSolver {
  int solver;
  bool (*covers)(const MixShape&, const fs_tuning&);   // a kernel instance runs the shape
  bool (*aut)(const MixShape&);                         // fs_tuning.mix_solver = 0 may choose it
};

// in order of precedence: mix_plan takes the first entry that may be chosen and covers
static const MixSolver kMixSolvers[] = {
    // two classes, N <= 16 (config 1): the one-wave binary solver
    {FS_SOLVER_BIN, [](const MixShape& s, const fs_tuning&) { return s.N <= 16 && s.C <= 2 && s.Bv <= 16 && off32(s); },
     [](const MixShape& s) { return s.N <= 16 && s.C <= 2; }},
    {FS_SOLVER_WAVE, [](const MixShape& s, const fs_tuning&) { return s.N <= 16 && s.C <= 4 && s.Bv <= 16; }, wave_auto},
    // instances: 4 clients per lane to N = 64 (C <= 16), 8 to N = 128 (C <= 10)
    {FS_SOLVER_QUAD,
     [](const MixShape& s, const fs_tuning&) {
       return s.Bv <= 16 && (s.N <= 64 ? s.C <= 16 : (s.N <= 128 && s.C <= 10)) && off32(s);
     },
     [](const MixShape& s) { return !wave_auto(s); }},
    // form 2 (two rows per wave) where it measured faster: N in (128, 256], NK = 4 (2.0 vs 4.1 us
    // per step at N = 256, C = 4); below that the one-row form is as fast or faster (r02g).
    // Instances: C <= 10 to N = 128, C <= 4 to N = 256
    {FS_SOLVER_REG2,
     [](const MixShape& s, const fs_tuning&) {
       return s.Bv <= 2 * M2_WAVES && s.N <= 256 && s.C <= (s.N <= 128 ? 10 : 4) && off32(s);
     },
     [](const MixShape& s) { return s.N > 128; }},
    // instances: C <= 24 to N = 64, C <= 10 to N = 128, C <= 4 to N = 256
    {FS_SOLVER_REG,
     [](const MixShape& s, const fs_tuning&) {
       return s.Bv <= MR_WAVES && s.N <= 256 && s.C <= (s.N <= 64 ? 24 : (s.N <= 128 ? 10 : 4));
     },
     [](const MixShape&) { return true; }},
    // the multi-CU quarter-wave solver where the single-workgroup register solvers end (N > 256)
    {FS_SOLVER_QMC,
     [](const MixShape& s, const fs_tuning& t) {
       return qmc_shape(s.N, s.C, s.Bv) && qmc_k(s.N, qmc_nk(s.N, s.C, t)) <= QMC_KMAX && off32(s);
     },
     [](const MixShape& s) { return s.N > 256; }},
    {FS_SOLVER_MC, [](const MixShape& s, const fs_tuning&) { return mc_shape(s.N, s.C, s.Bv); },
     [](const MixShape&) { return true; }},
    // LDS-staged solver: two batches of Z rows + p, buf and the wave partials must fit
    {FS_SOLVER_STAGED,
     [](const MixShape& s, const fs_tuning&) {
       return s.N <= 64 * MS2_NK && s.C <= 16 && staged_lds(s) <= 150 * 1024 &&
              (size_t)s.Bv * (s.C * mix_ldn(s.N) / 4) <= (size_t)MS_THREADS * MS2_PER_THREAD;
     },
     [](const MixShape&) { return true; }},
    {FS_SOLVER_GLOBAL, [](const MixShape& s, const fs_tuning&) { return global_lds(s) <= 160 * 1024; },
     [](const MixShape&) { return true; }},
};

// by shape, or forced by fs_tuning.mix_solver (tests, diagnostics); a forced solver that does
// not cover the shape falls through to staged, then global.  0: N too large for any solver
static int mix_choose(const MixShape& s, const fs_tuning& t) {
  const int want = t.mix_solver;
  for (const MixSolver& e : kMixSolvers) {
    const bool fallback = e.solver == FS_SOLVER_GLOBAL || (e.solver == FS_SOLVER_STAGED && want != FS_SOLVER_GLOBAL);
    if ((want == FS_SOLVER_AUTO ? e.aut(s) : (want == e.solver || fallback)) && e.covers(s, t)) return e.solver;
  }
  return 0;
}

// L2 prefetch helpers (fs_tuning.mix_prefetch: 0 = by solver, -1 = none, n): 4 for the
// quarter-wave solver, whose gather they speed up (r02s2k, 1.42-1.47 -> 1.35-1.43 us per step
// at config 2), 24 for qmc, none for the others, where they measured nothing; the progress word
// lives in the error block (byte 128)
// (quad: only when Z outgrows the L2s -- at config 1's 0.6 MB the helpers cost 3 %, r02s2c1)
static int mix_helpers(const MixPlan& P, const MixShape& s, const fs_tuning& t) {
  const bool z_big = (int64_t)s.nv * s.C * mix_ldn(s.N) * 4 > ((int64_t)16 << 20);
  const int h = t.mix_prefetch > 0 ? t.mix_prefetch
                : (t.mix_prefetch < 0 ? 0 : ((P.solver == FS_SOLVER_QUAD && z_big) ? 4 : (P.solver == FS_SOLVER_QMC ? 24 : 0)));
  switch (P.solver) {   // where the helper workgroups of each solver's grid run
    case FS_SOLVER_QUAD:
    case FS_SOLVER_REG: return std::min(h, 31);                  // the solver's XCD, one CU each
    case FS_SOLVER_QMC: return std::min(h, 32 - P.K);            // the solvers' XCD has 32 CUs
    case FS_SOLVER_MC: return std::min(h, (MC_XCDS - 1) * P.K);  // the grid's other-XCD blocks
    default: return 0;                                           // the other solvers run none
  }
}

// default lead: 16 steps for the quarter-wave solver; 8 for qmc, whose helpers (round 4:
// LDS-DMA pieces, the solver's progress published every step) keep a few steps of rows in
// the XCD's 4 MB L2 ahead of the solver -- at config 5 before the first-poll delay, 24
// helpers, leads 4 / 6 / 8 / 12: 3.85 / 3.62 / 3.76 / 3.81 us per step, none: 4.40
// (profiles/r04/mix_solve_helper_sweep.txt); with it (16 helpers at K = 16), leads 6 / 8 / 10
// / 12 / 16: 2.70-2.72 / 2.58 / 2.62-2.63 / 2.65 / 2.66, and at N = 300 1.96 for 6 and 8
// (profiles/r04/qmc_lead_sweep.txt); at N = 800 (K = 13) 8 is faster (2.33 vs 2.38-2.40), at
// N = 520 (K = 9) 6 (2.08 vs 2.18-2.24, profiles/r04/qmc_lead_sweep2.txt): 8 from K = 12, as
// the first-poll delay's step (qmc_poll_delay)
static int mix_lead(const MixPlan& P, const fs_tuning& t) {
  if (t.mix_prefetch_lead > 0) return t.mix_prefetch_lead;
  return P.solver == FS_SOLVER_QMC ? (P.K >= 12 ? 8 : 6) : 16;
}

// The solver that will launch for this shape under this tuning, and everything its launch
// needs.  Pure: no device state, no HIP call.  `blocks` > 1 is fs_mix_solve_blocked's Z layout
// (read by qmc only; the choice does not depend on it).
MixPlan mix_plan(int N, int C, int n_val, int epochs, int Bv, int blocks, const fs_tuning& t) {
  const MixShape s{N, C, n_val, epochs, Bv};
  MixPlan P;
  P.solver = mix_choose(s, t);
  P.zR = blocks;
  switch (P.solver) {
    case FS_SOLVER_QMC:
      P.nk = qmc_nk(N, C, t);
      P.K = qmc_k(N, P.nk);
      P.poll_delay = qmc_poll_delay(P.K, C, t);
      break;
    case FS_SOLVER_MC:
      P.S = mc_slice(N);
      P.K = mc_k(N);
      P.hops = mc_hops(P.K, P.S);
      break;
    case FS_SOLVER_STAGED: P.lds = staged_lds(s); break;
    case FS_SOLVER_GLOBAL: P.lds = global_lds(s); break;
  }
  const bool exchange = P.solver == FS_SOLVER_QMC || P.solver == FS_SOLVER_MC;
  if (exchange) P.spin_limit = mc_spin_limit(t);
  // quad, bin: softmax on v_exp_f32 / v_rcp_f32 (e / sum) by default: config 2 1.28-1.29 ->
  // 1.21-1.23 us per step (r02s2fx), within the fp32 tolerance of the oracle like every other
  // solver; fs_tuning.mix_exact_softmax: torch's exp(o - m - log(sum)) form with libm expf / logf
  P.fast_softmax = (P.solver == FS_SOLVER_QUAD || P.solver == FS_SOLVER_BIN) && !t.mix_exact_softmax;
  // quad's loader waves: config 2's instance (8 clients per lane, 10 classes) by default,
  // fs_tuning.mix_quad_loaders = -1 off
  // (2 classes in the register ring, 8 through the LDS ring: 0.837-0.839 us per step against
  // 0.851-0.856 with 3 and 0.851-0.874 with 1, profiles/r04/quad_loader_split.txt)
  P.loaders = P.solver == FS_SOLVER_QUAD && N > 64 && C > 8 && P.fast_softmax && t.mix_quad_loaders >= 0;
  P.helpers = mix_helpers(P, s, t);
  P.lead = P.helpers > 0 ? mix_lead(P, t) : 0;
  P.ws_bytes = exchange ? mc_xbytes(P.K) + MC_ERR_BYTES : (P.helpers > 0 ? MC_ERR_BYTES : 0);
  return P;
}

// the calling thread's last launch: its solver (fs_mix_solve_last_mode) and, of the qmc
// solver, its workgroups K and clients per lane (fs_mix_solve_last_layout: 0, 0 otherwise)
static thread_local int t_last_solver = 0, t_last_k = 0, t_last_nk = 0;

// place the caller's workspace, clear what the launch needs cleared, launch the plan's solver
static int mix_launch(MixArgs a, MixPlan plan, void* d_ws, int64_t ws_bytes, hipStream_t st) {
  const bool exchange = plan.solver == FS_SOLVER_QMC || plan.solver == FS_SOLVER_MC;
  if (exchange && (!d_ws || ws_bytes < plan.ws_bytes))
    return fail(FS_EINVAL, "fs_mix_solve: workspace too small (see fs_mix_solve_ws_bytes)");
  const bool has_err = d_ws && ws_bytes >= MC_ERR_BYTES;
  if (!has_err) plan.helpers = plan.lead = 0;   // helpers only warm the cache: none without their progress word
  unsigned* err = has_err ? reinterpret_cast<unsigned*>(reinterpret_cast<char*>(d_ws) + ws_bytes - MC_ERR_BYTES) : nullptr;
  hipError_t e = hipSuccess;
  if (plan.helpers > 0) {
    a.prog = err + 128 / sizeof(unsigned);
    e = hipMemsetAsync(a.prog, 0, sizeof(unsigned), st);
  }
  if (exchange && e == hipSuccess) {
    a.xbuf = reinterpret_cast<unsigned long long*>(d_ws);
    a.err = err;
    e = hipMemsetAsync(a.xbuf, 0, (size_t)(plan.ws_bytes - MC_ERR_BYTES), st);
  }
  if (e != hipSuccess) return fail(FS_EHIP, std::string("fs_mix_solve: ") + hipGetErrorString(e));
  int rc = FS_OK;
  switch (plan.solver) {
    case FS_SOLVER_BIN: rc = launch_mix_bin(a, plan, st); break;
    case FS_SOLVER_WAVE: rc = launch_mix_wave(a, plan, st); break;
    case FS_SOLVER_QUAD: rc = launch_mix_quad(a, plan, st); break;
    case FS_SOLVER_REG2: rc = launch_mix_reg2(a, plan, st); break;
    case FS_SOLVER_REG: rc = launch_mix_reg(a, plan, st); break;
    case FS_SOLVER_QMC: rc = launch_mix_qmc(a, plan, st); break;
    case FS_SOLVER_MC: rc = launch_mix_mc(a, plan, st); break;
    case FS_SOLVER_STAGED: rc = launch_mix_staged(a, plan, st); break;
    case FS_SOLVER_GLOBAL: rc = launch_mix_global(a, plan, st); break;
    default: rc = fail(FS_EINVAL, "fs_mix_solve: N too large for the LDS-resident mixture solve");
  }
  if (rc != FS_OK) return rc;
  t_last_solver = plan.solver;
  t_last_k = plan.K;
  t_last_nk = plan.nk;
  return FS_OK;
}

}  // namespace fs

using namespace fs;

extern "C" int fs_mix_solve_last_mode(void) { return t_last_solver; }

extern "C" int fs_mix_solve_last_layout(int* workgroups, int* lane_clients) {
  FS_REQUIRE(workgroups && lane_clients, "null pointer");
  const bool q = t_last_solver == FS_SOLVER_QMC;
  *workgroups = q ? t_last_k : 0;
  *lane_clients = q ? t_last_nk : 0;
  return FS_OK;
}

// independent of the tuning: the larger of what mc and qmc (at either lane width) can ask for
extern "C" int64_t fs_mix_solve_ws_bytes(int N, int C, int Bv) {
  if (N < 1) return MC_ERR_BYTES;
  const int64_t mc = mc_shape(N, C, Bv) ? mc_xbytes(mc_k(N)) : 0;
  const int64_t qmc = qmc_shape(N, C, Bv) ? mc_xbytes(qmc_k(N, 4)) : 0;   // the larger K of either lane width
  return std::max(mc, qmc) + MC_ERR_BYTES;
}

extern "C" int fs_mix_solve_plan(int N, int C, int n_val, int epochs, int Bv, int blocks, fs_mix_plan* out) {
  FS_REQUIRE(N >= 1 && C >= 1 && n_val >= 1 && epochs >= 0 && blocks >= 1, "bad sizes");
  FS_REQUIRE(Bv >= 1 && Bv <= MS_MAXB, "valid batch size must be in [1, 64]");
  FS_REQUIRE(out, "null pointer");
  const MixPlan P = mix_plan(N, C, n_val, epochs, Bv, blocks, tuning());
  FS_REQUIRE(P.solver, "N too large for the LDS-resident mixture solve");
  const bool q = P.solver == FS_SOLVER_QMC;
  *out = fs_mix_plan{P.solver, q ? P.K : 0, q ? P.nk : 0, P.helpers, P.lead, P.poll_delay, P.ws_bytes};
  return FS_OK;
}

extern "C" int fs_mix_solve(const float* d_Z, const int32_t* d_labels, const int32_t* d_perms, int N, int C,
                            int n_val, int epochs, int Bv, float lr_p, float momentum, float* d_p, float* d_buf,
                            int* d_first, void* d_ws, int64_t ws_bytes, void* stream) {
  FS_REQUIRE(N >= 1 && C >= 1 && n_val >= 1 && epochs >= 0, "bad sizes");
  FS_REQUIRE(Bv >= 1 && Bv <= MS_MAXB, "valid batch size must be in [1, 64]");
  FS_REQUIRE(d_Z && d_labels && d_perms && d_p && d_buf && d_first, "null pointer");
  const MixPlan plan = mix_plan(N, C, n_val, epochs, Bv, 1, tuning());
  FS_REQUIRE(plan.solver, "N too large for the LDS-resident mixture solve");
  if (int rc = mix_launch(MixArgs{d_Z, d_labels, d_perms, N, C, n_val, epochs, Bv, lr_p, momentum, d_p, d_buf, d_first},
                          plan, d_ws, ws_bytes, reinterpret_cast<hipStream_t>(stream)))
    return rc;
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" int fs_mix_solve_blocked_covers(int N, int C, int n_val, int epochs, int Bv) {
  return N >= 1 && C >= 1 && n_val >= 1 && epochs >= 0 &&
         mix_plan(N, C, n_val, epochs, Bv, 2, tuning()).solver == FS_SOLVER_QMC;
}

extern "C" int fs_mix_solve_blocked(const float* d_Z, int blocks, const int32_t* d_labels, const int32_t* d_perms,
                                    int N, int C, int n_val, int epochs, int Bv, float lr_p, float momentum, float* d_p,
                                    float* d_buf, int* d_first, void* d_ws, int64_t ws_bytes, void* stream) {
  FS_REQUIRE(N >= 1 && C >= 1 && n_val >= 1 && epochs >= 0, "bad sizes");
  FS_REQUIRE(blocks >= 1 && N % (4 * blocks) == 0, "N must be a multiple of 4 * blocks");
  FS_REQUIRE(Bv >= 1 && Bv <= MS_MAXB, "valid batch size must be in [1, 64]");
  FS_REQUIRE(d_Z && d_labels && d_perms && d_p && d_buf && d_first, "null pointer");
  const MixPlan plan = mix_plan(N, C, n_val, epochs, Bv, blocks, tuning());
  if (plan.solver != FS_SOLVER_QMC)
    return fail(FS_EUNSUPPORTED, "fs_mix_solve_blocked: the rank-blocked Z layout is read by the qmc solver only "
                                 "(N > 256, C <= 16, Bv <= 16); use fs_mix_solve on the standard layout");
  if (int rc = mix_launch(MixArgs{d_Z, d_labels, d_perms, N, C, n_val, epochs, Bv, lr_p, momentum, d_p, d_buf, d_first},
                          plan, d_ws, ws_bytes, reinterpret_cast<hipStream_t>(stream)))
    return rc;
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// Host side of fs_local_train: the geometry of every exchanging form (split with its team
// instances, pair, pipe), the planner (fs_local_train_plan), the exchange workspace's layout and
// hand-off tags, the launch setup the forms share, the wide form's workspace (local_train_wide.h:
// one workgroup per client, nothing exchanged), and fs_local_train's validation and dispatch.
// Host code only (built without a device pass): the kernels and their instance selection stay in
// local_train*.hip, behind one launch_<form>_instance each (local_train_forms.h), so an edit
// here changes no kernel revision (_lib.source_revision).
#include <mutex>
#include <unordered_map>

#include "local_train_wide.h"
#include "scaffold.h"
#include "split_common.h"

namespace fs {

static_assert(SP_ERR_BYTES == PR_ERR_BYTES && SP_ERR_BYTES == PP_ERR_BYTES && SP_ERR_BYTES == WD_ERR_BYTES,
              "one error block for every form");

// CUs of the current device (cached)
static int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
  }
  return cus;
}

// The launch generation of a workspace (SplitWS::tag_base = generation << 20).  0 or 1 (the
// caller then clears the granules): a workspace's first use, every 4095 launches (the
// generation wraps), and a launch whose client sequences may run 2^20 - 1 steps or more.
static unsigned exchange_generation(const void* ws, bool long_launch) {
  static std::mutex gm;
  static std::unordered_map<const void*, unsigned> gens;
  std::lock_guard<std::mutex> lk(gm);
  auto it = gens.find(ws);
  const unsigned prev = it == gens.end() ? 0u : it->second;
  const unsigned gen = (long_launch || prev >= 4095u) ? 0u : prev + 1u;
  gens[ws] = gen;
  return gen;
}

// the hand-off spin bound (fs_tuning.spin_limit, else the form's own); 0 = the injected-timeout test knob
static unsigned spin_bound(unsigned form_limit) {
  const fs_tuning t = tuning();
  if (t.inject_timeout) return 0u;
  return t.spin_limit ? t.spin_limit : form_limit;
}

// s_sleep(1) units before a step's first poll (fs_tuning.split_poll_delay: 0 = by width, -1 =
// none, n > 0 = n).  By width (profiles/r04/split_poll_delay_*.txt, launch ms): G = 16 (config 5)
// 5.35-5.37 without, 5.21-5.23 at 16, 5.29-5.31 at 24, 5.45-5.49 at 48; G = 2 (config 2) no gain
// while every poll ran two exchange slots.  With one slot (round 12: fewer loads pace a wave's
// polls) G = 2 gains (profiles/r12/c2_sweep*.txt, launch us): 257.6-260.3 without, 252.4 at 3,
// 252.5 at 4, 253.1-253.2 at 5, 254.6-254.9 at 12; the two-slot parent 260-264 at every delay.
// G = 4 likewise (config 3, FedProx, profiles/r12/c3_sweep.txt): 4,060-4,073 without -- slower than
// the two-slot parent's 3,973-3,989 -- 3,942-3,947 at 4, 3,926-3,928 at 8, 3,913-3,916 at 16
constexpr int SPLIT_PD_WIDE = 16, SPLIT_PD_G2 = 4;
static int split_poll_delay(int G, bool chained) {
  const int t = tuning().split_poll_delay;
  if (t < 0) return 0;
  if (t > 0) return t;
  if (chained) return 0;                 // one group: no other group's polls to yield to
  return G >= 4 ? SPLIT_PD_WIDE : SPLIT_PD_G2;
}

// ---- the forms' geometry -----------------------------------------------------------------------
// (RT = lt_rt(B) 16-row batch tiles, NT = ld / 64 feature tiles, G workgroups per group)

static size_t split_dyn_lds(int RT, int NT, int G, int teams) {
  const int tiles = (NT + G - 1) / G;
  return sizeof(float) * (size_t)teams * (size_t)(RT * 16) * (size_t)(tiles * 64 + 8);
}

static size_t split_static_lds(int RT, int NW, int teams) {
  const int NR = RT * 16;
  return (size_t)teams * ((size_t)NW * NR * 16 * 4 + 2 * (size_t)NR * 16 * 4 + 2 * NR * 4 + NW * 3 * 4 + 8) + 64 +
         4 * teams;
}

// can G workgroups split one client of this shape (teams = 2: two client lanes of 4 waves per
// workgroup)?
static bool split_fits(int C, int B, int NT, int G, int teams) {
  if (!(G == 2 || G == 4 || G == 8 || G == 16)) return false;
  if (C > 16 || B > 32 || NT < G) return false;
  const int RT = lt_rt(B);
  const int nw = SP_WAVES / teams;
  const int tiles = (NT + G - 1) / G;
  if ((tiles + nw - 1) / nw > SP_TPW) return false;
  if (G >= 8 && RT * 16 * C + 2 > 512) return false;   // exchanged values: at most 512
  return split_dyn_lds(RT, NT, G, teams) + split_static_lds(RT, nw, teams) <= 160 * 1024;
}

static size_t pair_dyn_lds(int RT) { return sizeof(float) * 2 * (size_t)(RT * 16) * (size_t)(PR_TILES * 64 + 8); }

static size_t pair_static_lds(int RT) {
  const int NR = RT * 16;
  return (size_t)PR_WAVES * NR * 16 * 4 + (size_t)NR * 16 * 4 + 2 * NR * 4 + 2 * PR_WAVES * 2 * 4 +
         PR_WAVES * 4 + 8 + 64;
}

// One exchanging form: which shapes it takes, what a group of G workgroups needs, how it launches.
struct Form {
  int flag;                             // its bit in G (FS_G_*; 0: the split form)
  int kernel;                           // FS_LT_* (a split launch may still choose its mb or dbuf instance)
  int lanes;                            // clients a group trains at a time
  int slots;                            // exchange slots per slice: a group owns slots * G * sz(RT) granules
  bool chains;                          // one group can walk chained clients
  bool poll_delay;                      // sleeps before a step's first poll (split_poll_delay)
  unsigned spin_limit;                  // its default spin bound
  size_t fuse_lds;                      // dynamic LDS the fused evaluation's workgroups need at least
  bool (*fits)(int C, int B, int NT, int G);
  int (*sz)(int RT);                    // granules per slot
  size_t (*lds)(int RT, int NT, int G); // dynamic LDS of one workgroup
  int (*launch)(const LTParams& P, int G, const SplitWS& X, int grid, size_t lds, hipStream_t st);
  const char* unfit;                    // fs_local_train's message for a shape outside `fits`
};

static int split_sz(int RT) { return RT * 16 * 16 + 4; }
constexpr size_t SPLIT_FUSE_LDS = sizeof(float) * SP_WAVES * 16 * 17;

static const Form SPLIT = {
    0, FS_LT_SPLIT, 1, 2, true, true, SP_SPIN_LIMIT, SPLIT_FUSE_LDS,
    [](int C, int B, int NT, int G) { return split_fits(C, B, NT, G, 1); }, split_sz,
    [](int RT, int NT, int G) { return split_dyn_lds(RT, NT, G, 1); }, launch_split_instance,
    "fs_local_train: slice too wide for one workgroup"};

// the team form: parallel clients at G = 4 or 8, two client lanes of 4 waves per workgroup
static const Form TEAMS = {
    FS_G_TEAMS, FS_LT_TEAMS, 2, 4, false, true, SP_SPIN_LIMIT, SPLIT_FUSE_LDS,
    [](int C, int B, int NT, int G) { return (G == 4 || G == 8) && split_fits(C, B, NT, G, 2); }, split_sz,
    [](int RT, int NT, int G) { return split_dyn_lds(RT, NT, G, 2); }, launch_teams_instance,
    "fs_local_train: slice too wide for one workgroup"};

// the pair form: parallel clients, two per group, 8 tiles per workgroup.  C <= 14: the two norms
// travel at classes 14 and 15 of row 0 of the (row, class) hand-off.  (It polls half a step
// after publishing: no poll delay.)
static const Form PAIR = {
    FS_G_PAIR, FS_LT_PAIR, 2, 5, false, false, PR_SPIN_LIMIT, 0,
    [](int C, int B, int NT, int G) {
      if (!(G == 2 || G == 4 || G == 8 || G == 16)) return false;
      if (C > 14 || B > 32 || NT != PR_TILES * G) return false;
      const int RT = lt_rt(B);
      return pair_dyn_lds(RT) + pair_static_lds(RT) <= 160 * 1024;
    },
    [](int RT) { return RT * 16 * 16 + 4 >= PR_THREADS ? RT * 16 * 16 + 4 : PR_THREADS; },
    [](int RT, int, int) { return pair_dyn_lds(RT); }, launch_pair_instance,
    "fs_local_train: the pair form needs C <= 14, B <= 32 and ld == 512 G"};

// the pipe form: full slices of 16 tiles, two 16-row batch tiles (its spin bound: the split form's)
static const Form PIPE = {
    FS_G_PIPE, FS_LT_PIPE, 1, 2, true, false, SP_SPIN_LIMIT, 0,
    [](int C, int B, int NT, int G) {
      if (!(G == 2 || G == 4 || G == 8 || G == 16)) return false;
      return C >= 1 && C <= 16 && B > 16 && B <= 32 && NT == PP_NTS * G;
    },
    [](int) { return PP_SZ; },
    [](int, int, int) { return sizeof(float) * (size_t)PP_NR * PP_RS; }, launch_pipe_instance,
    "fs_local_train: the pipe form needs ld = 1024 G (G = 2, 4, 8 or 16), 16 < B <= 32 and C <= 16"};

// the form a planned G names (G = width | FS_G_*)
static const Form& form_of(int G) {
  return (G & FS_G_PIPE) ? PIPE : (G & FS_G_PAIR) ? PAIR : (G & FS_G_TEAMS) ? TEAMS : SPLIT;
}

// groups in flight: one per G workgroups, one workgroup per CU, `lanes` clients per group at a
// time; a chain is one group's
static int form_groups(const Form& f, int N, int G, int chained, int cus) {
  return chained ? 1 : std::max(1, std::min((N + f.lanes - 1) / f.lanes, cus / G));
}

static int64_t form_xbuf_bytes(const Form& f, int ngroups, int G, int RT) {
  return (int64_t)ngroups * f.slots * G * f.sz(RT) * 8;
}

static int64_t form_ws_bytes(const Form& f, int N, int G, int B, int chained, int cus) {
  return form_xbuf_bytes(f, form_groups(f, N, G, chained, cus), G, lt_rt(B)) + SP_ERR_BYTES;
}

int split_idle_cus(int N, int C, int B, int64_t ld, int G, int chained) {
  if (G & FS_G_WIDE) return 0;           // one workgroup per client: not an exchanging launch
  const Form& f = form_of(G);
  const int g = G & (FS_G_PAIR - 1);
  const int cus = device_cus();
  if (chained || cus <= 0 || !f.fits(C, B, (int)(ld >> 6), g)) return 0;
  return std::max(0, cus - form_groups(f, N, g, 0, cus) * g);
}

// ---- the launch setup every exchanging form shares -----------------------------------------------

// fs_local_train's answer to a (form, shape, G) the form does not take, each with its own text
static int form_admits(const Form& f, const LTParams& P, int G, int NT) {
  if (&f == &TEAMS && (P.chained || !(G == 4 || G == 8)))
    return fail(FS_EUNSUPPORTED, "fs_local_train: the team form runs parallel clients at G = 4 or 8");
  if (&f == &PAIR && P.chained) return fail(FS_EINVAL, "fs_local_train: the pair form needs parallel clients");
  if (&f == &SPLIT || &f == &TEAMS) {
    if (!(G == 2 || G == 4 || G == 8 || G == 16)) return fail(FS_EINVAL, "fs_local_train: G must be 1, 2, 4, 8 or 16");
    if (P.C > 16 || P.B > 32) return fail(FS_EUNSUPPORTED, "fs_local_train: split clients need C <= 16, B <= 32");
    if (NT < G) return fail(FS_EUNSUPPORTED, "fs_local_train: fewer feature tiles than workgroups per client");
  }
  if (!f.fits(P.C, P.B, NT, G)) return fail(FS_EUNSUPPORTED, f.unfit);
  return FS_OK;
}

// Checks (P, G) against the form, the device and the workspace, lays the workspace out --
// [ngroups][slots][G][SZ] granules, then (diagnostic build) the stamps, the error block last --
// takes the launch generation and clears the granules where the tags alone cannot tell this
// launch's from an earlier one's, and sizes the grid and the dynamic LDS.
static int exchange_setup(const Form& f, const LTParams& P, int G, void* ws, int64_t ws_bytes, hipStream_t st,
                          SplitWS& X, int& grid, size_t& lds) {
  const int RT = lt_rt(P.B);
  const int NT = (int)(P.ld >> 6);
  if (int rc = form_admits(f, P, G, NT)) return rc;
  const int cus = device_cus();
  if (cus <= 0) return fail(FS_EHIP, "fs_local_train: no device");
  if (G > cus) return fail(FS_EUNSUPPORTED, "fs_local_train: G exceeds the CU count");
  const int ng = form_groups(f, P.N, G, P.chained, cus);
  const int64_t xbytes = form_xbuf_bytes(f, ng, G, RT);
  if (!ws || ws_bytes < xbytes + SP_ERR_BYTES) return fail(FS_EINVAL, "fs_local_train: workspace too small");
  char* base = reinterpret_cast<char*>(ws);
  X.xbuf = reinterpret_cast<unsigned long long*>(base);
  X.err = reinterpret_cast<unsigned*>(base + ws_bytes - SP_ERR_BYTES);   // last block: sticky
  X.SZ = f.sz(RT);
  X.ngroups = ng;
  X.spin_limit = spin_bound(f.spin_limit);
  X.poll_delay = f.poll_delay ? split_poll_delay(G, P.chained != 0) : 0;
  X.stamps = nullptr;
#ifdef FS_STAMPS
  X.stamps = reinterpret_cast<unsigned long long*>(base + xbytes);
#endif
  // Hand-off tags: (launch generation << 20) + step + 1 of the tag sequence, so a granule left
  // by an earlier launch never carries a tag this launch waits for.  The granules are cleared
  // when a workspace is first seen, every 4095 launches (the generation wraps) and for a
  // launch whose sequences may run 2^20 - 1 steps or more (then the generation is 0: tags are
  // the step + 1 alone, as after any clearing).
  // (a sequence walks the clients in snake order, at most ceil(N / (ng * lanes)); chained: all N)
  const int64_t seq_clients = P.chained ? P.N : (P.N + ng * f.lanes - 1) / (ng * f.lanes);
  const bool long_launch = P.max_client_steps <= 0 || P.max_client_steps * seq_clients >= (1 << 20) - 1;
  const unsigned gen = exchange_generation(ws, long_launch);
  X.tag_base = gen << 20;
  if (gen <= 1) {                      // first use, wrap or long launch: clear the granules
    hipError_t e = hipMemsetAsync(base, 0, (size_t)xbytes, st);
    if (e != hipSuccess) return fail(FS_EHIP, std::string("fs_local_train: ") + hipGetErrorString(e));
  }
  lds = f.lds(RT, NT, G);
  if (P.fuse_E > 0 && (P.chained || ng * G + P.fuse_E > cus || lds < f.fuse_lds))
    return fail(FS_EINVAL, "fs_local_train: no room for the fused evaluation");
  grid = P.chained ? 8 * G : ng * G + P.fuse_E;
  return FS_OK;
}

// ---- the wide form (local_train_wide.hip): one workgroup per client, any batch size ---------------
// Host arithmetic only (no device query): wd_grid(N, chained) workgroups, each with a slot of
// [wd_slot_rows(largest batch)][wd_nc(C)] floats, then the error block (never written).

// bmax: the largest effective batch, min(B, max_j n_j)
static int64_t wide_ws_bytes(int N, int C, int64_t bmax, int chained) {
  return (int64_t)wd_grid(N, chained) * wd_slot_rows(bmax) * wd_nc(C) * (int64_t)sizeof(float) + WD_ERR_BYTES;
}

// lays `grid` slots out over the workspace the caller planned: the slot is as many whole
// blocks of rows as the bytes before the error block give every workgroup
static int wide_setup(const LTParams& P, void* ws, int64_t ws_bytes, WideWS& X, int& grid) {
  grid = wd_grid(P.N, P.chained);
  if (!ws || ws_bytes < WD_ERR_BYTES) return fail(FS_EINVAL, "fs_local_train: workspace too small");
  const int64_t row_bytes = (int64_t)wd_nc(P.C) * (int64_t)sizeof(float);
  int64_t rows = (ws_bytes - WD_ERR_BYTES) / grid / row_bytes / WD_BLOCK * WD_BLOCK;
  // (no more than B asks for, and an int: client sizes are ints, so no batch is longer)
  rows = std::min<int64_t>({rows, wd_slot_rows((int64_t)P.B), (int64_t)INT32_MAX / WD_BLOCK * WD_BLOCK});
  if (P.E > 0 && rows < WD_BLOCK) return fail(FS_EINVAL, "fs_local_train: workspace too small");
  X.g = reinterpret_cast<float*>(ws);
  X.slot_rows = (int)rows;
  X.slot_floats = (int64_t)X.slot_rows * wd_nc(P.C);
  return FS_OK;
}

static thread_local int t_last_lt = 0;
void set_last_lt_kernel(int k) { t_last_lt = k; }

int local_train(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int32_t* d_labels,
                const int32_t* d_perms, const int32_t* d_order, int N, int C, int B, int E, float lr, float mu,
                int prox, float lam, int reg, int chained, const float* d_W_start, float* d_W_out,
                double* d_loss, int G, void* d_ws, int64_t ws_bytes, hipStream_t st,
                int64_t max_client_steps, const FuseEval* fuse) {
  FS_REQUIRE(N >= 1, "N must be >= 1");
  FS_REQUIRE(C >= 1 && C <= 32, "num_classes must be in [1, 32]");
  const bool wide = (G & FS_G_WIDE) != 0;
  FS_REQUIRE(B >= 1, "batch_size must be >= 1");
  FS_REQUIRE(wide || B <= 64, "batch_size above 64 needs the wide form (G = 1 | FS_G_WIDE, from fs_local_train_plan)");
  FS_REQUIRE(!wide || G == (1 | FS_G_WIDE), "the wide form runs one workgroup per client (G = 1 | FS_G_WIDE)");
  FS_REQUIRE(E >= 0, "epoch must be >= 0");
  FS_REQUIRE(ld >= 64 && ld % 64 == 0, "ld must be a positive multiple of 64");
  FS_REQUIRE(d_phi && d_row_off && d_labels && d_perms && d_W_start && d_W_out && d_loss, "null pointer");
  LTParams P{d_phi, ld, d_row_off, d_labels, d_perms, d_order, N, C, B, E, lr, mu, lam,
             prox ? 1 : 0, reg ? 1 : 0, chained ? 1 : 0, d_W_start, d_W_out, d_loss, max_client_steps};
  if (fuse && G > 1 && !wide && !chained) {
    P.fuse_phi = fuse->phi;
    P.fuse_y = fuse->y;
    P.fuse_n = fuse->n;
    P.fuse_E = fuse->E;
    P.fuse_part = fuse->part;
  }
  int rc;
  if (wide) {
    set_last_lt_kernel(FS_LT_WIDE);
    WideWS X;
    int grid = 0;
    rc = wide_setup(P, d_ws, ws_bytes, X, grid);
    if (rc == FS_OK) rc = launch_local_train_wide(P, X, grid, st);
  } else if (G > 1) {
    const Form& f = form_of(G);
    const int g = G & (FS_G_PAIR - 1);
    set_last_lt_kernel(f.kernel);
    SplitWS X;
    int grid = 0;
    size_t lds = 0;
    rc = exchange_setup(f, P, g, d_ws, ws_bytes, st, X, grid, lds);
    if (rc == FS_OK) rc = f.launch(P, g, X, grid, lds, st);
  } else {
    set_last_lt_kernel(FS_LT_SINGLE);
    rc = launch_local_train_single(P, st);
  }
  if (rc != FS_OK) return rc;
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// ---- SCAFFOLD (local_train_scaffold.hip): the single form with control variates -------------------
// One workgroup per client of d_order, no workspace and no planner: parallel clients,
// cross-entropy, B <= 64, no prox term.  Nothing is launched or written on a violation.
int local_train_scaffold(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int32_t* d_labels,
                         const int32_t* d_perms, const int32_t* d_order, int N, int C, int B, int E, float lr,
                         float lam, int reg, const float* d_W_start, const float* d_c, float* d_ci, float* d_W_out,
                         double* d_loss, hipStream_t st) {
  FS_REQUIRE(N >= 1, "N must be >= 1");
  FS_REQUIRE(C >= 1 && C <= 32, "num_classes must be in [1, 32]");
  FS_REQUIRE(B >= 1, "batch_size must be >= 1");
  if (B > 64)
    return fail(FS_EUNSUPPORTED, "fs_local_train_scaffold: batch_size above 64 is not provided (no wide form with variates)");
  FS_REQUIRE(E >= 0, "epoch must be >= 0");
  FS_REQUIRE(ld >= 64 && ld % 64 == 0, "ld must be a positive multiple of 64");
  FS_REQUIRE(lr > 0.f, "lr must be > 0 (the new variate divides by K * lr)");
  FS_REQUIRE(d_phi && d_row_off && d_labels && d_perms && d_W_start && d_c && d_ci && d_W_out && d_loss, "null pointer");
  const LTSParams P{d_phi, ld, d_row_off, d_labels, d_perms, d_order, N, C, B, E, lr, lam, reg ? 1 : 0,
                    d_W_start, d_c, d_ci, d_W_out, d_loss};
  const int rc = launch_local_train_scaffold(P, st);
  if (rc != FS_OK) return rc;
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace fs

using namespace fs;

extern "C" int fs_local_train_scaffold(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int32_t* d_labels,
                                       const int32_t* d_perms, const int32_t* d_order, int N, int C, int B, int E,
                                       float lr, float lam, int reg, const float* d_W_start, const float* d_c,
                                       float* d_ci, float* d_W_out, double* d_loss, void* stream) {
  return fs::local_train_scaffold(d_phi, ld, d_row_off, d_labels, d_perms, d_order, N, C, B, E, lr, lam, reg, d_W_start,
                                  d_c, d_ci, d_W_out, d_loss, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_local_train_last_kernel(void) { return t_last_lt; }

extern "C" int fs_local_train(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int32_t* d_labels,
                              const int32_t* d_perms, const int32_t* d_order, int N, int C, int B, int E,
                              float lr, float mu, int prox, float lam, int reg, int chained,
                              const float* d_W_start, float* d_W_out, double* d_loss, int G, void* d_ws,
                              int64_t ws_bytes, void* stream) {
  return fs::local_train(d_phi, ld, d_row_off, d_labels, d_perms, d_order, N, C, B, E, lr, mu, prox, lam, reg, chained,
                         d_W_start, d_W_out, d_loss, G, d_ws, ws_bytes, reinterpret_cast<hipStream_t>(stream), 0);
}

// Plan the launch: G = workgroups per client (1 = one workgroup walks each client; 2..16 =
// a group of G workgroups splits the feature dimension of one client at a time) and the
// workspace bytes it needs.  On entry *G_out is a request: 0 = let the planner choose,
// 1 = one workgroup per client, 2..16 = that group width if the shape allows it (else the
// planner's choice), width | FS_G_* = that form at that width, likewise.
// B > 64, or a request of 1 | FS_G_WIDE at any B: the wide form (1 | FS_G_WIDE), whose workspace
// is wd_grid(N, chained) slots for the largest effective batch, min(B, max_en / E) rows -- host
// arithmetic only, the same answer on every device.
// prox: the FedProx term is on (kept in the ABI; every split variant covers it).
// max_en = max_j E * n_j.
extern "C" int fs_local_train_plan(int N, int C, int B, int E, int64_t ld, int64_t max_en, int chained, int prox,
                                   int* G_out, int64_t* ws_bytes_out) {
  FS_REQUIRE(G_out && ws_bytes_out, "null pointer");
  FS_REQUIRE(N >= 1 && B >= 1 && ld >= 64 && ld % 64 == 0, "bad sizes");
  const int want = *G_out;
  *G_out = 1;
  *ws_bytes_out = 0;
  if (B > 64 || want == (1 | FS_G_WIDE)) {
    FS_REQUIRE(C >= 1 && C <= 32, "num_classes must be in [1, 32]");
    FS_REQUIRE(E >= 0 && (E == 0 || max_en >= 1), "the wide form needs max_en = max_j E * n_j");
    const int64_t max_n = E > 0 ? (max_en + E - 1) / E : 0;
    *G_out = 1 | FS_G_WIDE;
    *ws_bytes_out = wide_ws_bytes(N, C, std::min<int64_t>(B, max_n), chained);
    return FS_OK;
  }
  const int cus = device_cus();
  if (want == 1 || C > 16 || B > 32 || cus <= 0) return FS_OK;
  const int NT = (int)(ld >> 6);
  const fs_tuning tune = tuning();
  // does the form take this launch at width g, and the plan that says so
  auto offers = [&](const Form& f, int g) {
    return (f.chains || !chained) && f.fits(C, B, NT, g) && g <= cus;
  };
  auto plan = [&](const Form& f, int g) {
    *G_out = g | f.flag;
    *ws_bytes_out = form_ws_bytes(f, N, g, B, chained, cus);
    return FS_OK;
  };
  // an explicit request is answered by its own form where that form offers the width asked for
  // (else by the planner's choice below)
  const int wg = want & (FS_G_PAIR - 1);
  auto asked = [&](const Form& f) { return f.flag ? (want & f.flag) != 0 : (want > 1 && want < FS_G_PAIR); };
  if (asked(PIPE) && offers(PIPE, wg)) return plan(PIPE, wg);
  // the pipe form (fs_tuning.split_pipe = 1: wherever it fits; -1 = never; 0 = by shape: parallel
  // clients at G <= 4 where its groups walk several clients each -- config 4, 1,250 clients of 64
  // rows on 128 groups of 2: 395-409 vs 419-448 us per launch for the pair form (G = 4) and
  // 285-302 vs 300-310 us at config 2's 100 clients, where the split form stays
  // (profiles/r05/pipe_vs_forms.txt); config 5's G = 16: 6.5 vs 4.9 ms, not chosen)
  // (entered for an automatic choice or a pipe request only: an explicit split, pair or team
  // request is answered by its own form, never by the pipe form under split_pipe = 1)
  if ((want == 0 || (want & FS_G_PIPE)) && NT % 16 == 0 && tune.split_pipe >= 0) {
    const int g = NT / 16;
    const bool by_shape = tune.split_pipe == 0 && want == 0 && tune.train_form == 0 && !chained && !prox && g <= 4 &&
                          N > form_groups(PIPE, N, g, 0, cus);
    if ((tune.split_pipe > 0 || by_shape) && offers(PIPE, g)) return plan(PIPE, g);
  }
  for (const Form* f : {&TEAMS, &PAIR, &SPLIT})
    if (asked(*f) && offers(*f, wg)) return plan(*f, wg);
  // the team form by tuning (fs_tuning.split_teams = 1: wherever it fits, at the narrowest
  // width; 0 = by shape: not yet chosen automatically; -1 never)
  if (tune.split_teams > 0)
    for (int cand : {4, 8})
      if (offers(TEAMS, cand)) return plan(TEAMS, cand);
  int G = 0;
  if (chained) {
    // one group walks the chain: slice one step's batch (B x ld floats) to ~32 KB per CU
    const int64_t bytes = (int64_t)B * ld * 4;
    for (int cand : {2, 4, 8, 16})
      if (offers(SPLIT, cand)) {
        G = cand;
        if (bytes / cand <= 32 * 1024) break;
      }
  } else {
    // parallel clients: the narrowest split group that fits (most clients in flight, fewest
    // partners) -- FedProx too since its anchor is re-read, not register-resident (r02t, prox,
    // us per launch, G = 1 vs split: config 2 741 / 362, config 3 5955 / 5263, config 4
    // 580 / 508, config 5 11237 / 7003)
    for (int cand : {2, 4, 8, 16})
      if (offers(SPLIT, cand)) { G = cand; break; }
    // ... unless the pair form fits and its groups would walk several clients each (where it
    // measured faster: config 4 0.434 vs 0.457 ms; with one client per group, config 2, the
    // split form: 0.343 vs 0.366 ms -- profiles/r03/pair_ab.txt) and there is no prox term
    // (round 5, config 3: split G = 4 5.09-5.11 ms vs pair G = 8 5.24-5.26 and pipe G = 4
    // 5.25-5.27, profiles/r05/forms_config3_4.txt; round 3 had measured the pair form ahead,
    // 5.16 vs 5.26), or fs_tuning.train_form asks for it (1: never, 2: wherever it fits)
    if (tune.train_form != 1)
      for (int cand : {2, 4, 8, 16})
        if (offers(PAIR, cand) && (tune.train_form == 2 || G == 0 || (!prox && N > form_groups(SPLIT, N, G, 0, cus))))
          return plan(PAIR, cand);
  }
  return G == 0 ? FS_OK : plan(SPLIT, G);
}

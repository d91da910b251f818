// fs_plan -- the native round driver.
//
// One call enqueues the launches of one federated round of FedAvg / FedProx (and the
// local-training / aggregation / evaluation phases of FedAMW), replacing the per-round
// Python work of the reference's round loop (/root/reference/functions/tools.py:337-352,
// 364-379, 427-462):
//   TRAIN      fs_local_train over every client (train_loop, tools.py:340-343), losses
//              written straight into the [R][N] history
//   AGGREGATE  fs_aggregate: W_g = sum_j p_j W_j (tools.py:345-350)
//   EVAL       fs_eval of W_g on the test set into the [R][2] history (tools.py:351)
// The DataLoader shuffles of a round (tools.py:179, one RandomSampler permutation per
// client and epoch) are replayed bit-exactly (MT19937 + forward Fisher-Yates) into one of
// two slots on the plan's own side stream, so round t+1's shuffles are produced while
// round t trains:
//   shuffle_device = 1  fs_randperm_device (one wave per pass) after an async upload of
//                       the seeds from pinned memory -- a few hundred waves beside the
//                       local-training grid, no host work;
//   shuffle_device = 0  a persistent pool of host threads (as fs_randperm_batch) driven by
//                       a coordinator thread, then one async upload of the permutations.
// Events order the slots: a slot is rewritten only after the local training that
// consumed its previous contents, and a local training waits for its slot.
//
// Partial participation (ABI 22, fs_plan_shuffle_subset / fs_plan_round_subset): a round in
// which M <= N sampled clients train.  Only their M*E passes are replayed (into the usual slot
// at the usual offsets), the plan's training form is launched over the M clients through its
// `order` table on the unchanged W_out / loss history, and the aggregate gathers the M sampled
// rows (fs_aggregate_sel).  Rows of W_out and the history outside the sample are not touched.
//
// FedNova (ABI 23, fs_plan_set_nova): AGGREGATE of either kind of round launches fs_aggregate_nova
// (aggregate_nova.hip) instead, with the round's weights as q and d_W_g as the base it updates.
//
// SCAFFOLD (additive to ABI 23, fs_plan_set_scaffold): TRAIN launches fs_local_train_scaffold
// (local_train_scaffold.hip; the plan's G and workspace are ignored) and AGGREGATE launches
// fs_aggregate_scaffold (aggregate_scaffold.hip), which updates d_W_g and the server variate from one
// pass over the round's rows.  A deferred evaluation is never fused while it is on.
//
// FedOpt (additive to ABI 23, fs_plan_set_server_opt): AGGREGATE launches fs_aggregate_opt
// (aggregate_opt.hip), the mode-2 fold with a server optimizer step on its end, updating d_W_g and
// the moments in place.  TRAIN is untouched, and the deferred evaluation's finaliser rides on it.
//
// q-FedAvg (additive to ABI 23, fs_plan_set_qffl): AGGREGATE launches fs_aggregate_qffl
// (aggregate_qffl.hip), the mode-2 fold and the updates' squared norms from one pass, then the
// q-FFL step on d_W_g in place.  TRAIN is untouched, and the finaliser rides on the pass.
//
// Robust aggregation (additive to ABI 23, fs_plan_set_robust): AGGREGATE launches fs_aggregate_robust
// (aggregate_robust.hip), the coordinate-wise trimmed mean or median of the round's rows into
// d_W_g; the round's weights are not read.  TRAIN is untouched, and the finaliser rides on it.
//
// Krum / Multi-Krum (additive to ABI 23, fs_plan_set_krum): AGGREGATE launches fs_aggregate_krum
// (aggregate_krum.hip), the rows' pairwise distances, the scores, the pick and the gathered fold of
// the picked rows into d_W_g; the weights are not read.  TRAIN is untouched, and the finaliser
// rides on the fold.
//
// RFA (additive to ABI 23, fs_plan_set_rfa): AGGREGATE launches fs_aggregate_rfa (aggregate_rfa.hip),
// T smoothed Weiszfeld iterations over the round's rows from x = d_W_g into d_W_g, under the
// round's weights or uniform ones.  TRAIN is untouched, and the finaliser rides on the last step.
//
// FedTopK (additive to ABI 23, fs_plan_set_topk): AGGREGATE launches fs_aggregate_topk
// (aggregate_topk.hip), the per-row top-k threshold of the round's corrected updates and their
// thresholded fold onto d_W_g, the clients' residuals updated in place.  TRAIN is untouched, and the
// finaliser rides on the fold.
//
// DP-FedAvg (additive to ABI 23, fs_plan_set_dp): AGGREGATE launches fs_aggregate_dp
// (aggregate_dp.hip), the norm pass over the round's updates, their clip coefficients and the clipped
// fold onto d_W_g with the round's Gaussian noise, t the round index of the call.  TRAIN is
// untouched, and the finaliser rides on the fold.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <deque>
#include <thread>
#include <vector>

#include <chrono>
#include <cmath>
#include <cstdio>

#include "aggregate_sel.h"
#include "common.h"
#include "finalize.h"
#include "mse_rows.h"
#include "mt_replay.h"
#include "randperm_geom.h"
#include "scaffold.h"

// RP_CAPPED = 0 (build macro, A/B): the plan's replays keep the uncapped geometry everywhere
#ifndef RP_CAPPED
#define RP_CAPPED 1
#endif

namespace fs {

// Persistent worker pool: run(n, fn) calls fn(i) for i in [0, n) on all workers + the caller.
class Pool {
 public:
  explicit Pool(int nthreads) {
    for (int t = 1; t < nthreads; ++t) th_.emplace_back([this] { loop(); });
  }
  ~Pool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
      ++gen_;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  void run(int64_t n, const std::function<void(int64_t)>& fn) {
    if (th_.empty() || n <= 1) {
      for (int64_t i = 0; i < n; ++i) fn(i);
      return;
    }
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = &fn;
      n_ = n;
      next_.store(0);
      busy_ = (int)th_.size();
      ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [this] { return busy_ == 0; });
    fn_ = nullptr;
  }

 private:
  void work() {
    for (;;) {
      const int64_t i = next_.fetch_add(1);
      if (i >= n_) return;
      (*fn_)(i);
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (stop_) return;
      }
      work();
      std::lock_guard<std::mutex> lk(m_);
      if (--busy_ == 0) done_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(int64_t)>* fn_ = nullptr;
  int64_t n_ = 0;
  std::atomic<int64_t> next_{0};
  int busy_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

}  // namespace fs

// a host shuffle job: round t, its seeds, and (a subset round) the sampled clients the
// seeds belong to, sel-major (empty: every client)
struct ShuffleJob {
  int t = 0;
  std::vector<int64_t> seeds;
  std::vector<int32_t> sel;
};

struct fs_plan {
  fs_plan_desc d;
  std::vector<int64_t> n, off;         // per pass (j*E + e): rows, offset into the shuffle buffer
  int64_t perm_len = 0;                // E * rows
  int32_t* h_perm[2] = {nullptr, nullptr};   // pinned (host replay)
  int32_t* d_perm[2] = {nullptr, nullptr};
  // device replay: a ring of SEED_SLOTS pinned seed buffers, each freed by its own event, so the
  // host never waits on the shuffle of the previous round before enqueuing the next (with two
  // slots that wait held the host ~330 us per round at config 2 and left the GPU idle between
  // rounds -- r02s2t)
  static constexpr int SEED_SLOTS = 4;
  int64_t* h_seed[SEED_SLOTS] = {};             // pinned, coherent
  int64_t* d_seed[SEED_SLOTS] = {};
  int64_t* h_seed_dev[SEED_SLOTS] = {};         // device view of h_seed (zero-copy seeds)
  hipEvent_t seed_read[SEED_SLOTS] = {};
  bool seed_pending[SEED_SLOTS] = {};
  bool seed_copy = false;                         // FS_SEED_COPY=1: upload the seeds (hipMemcpyAsync)
  int64_t* d_pass = nullptr;                 // [2][P]: rows, offset of every pass (device replay)
  int64_t max_n = 0;
  int64_t max_client_steps = 0;       // E * ceil(max_j n_j / B)
  int fuse_E = 0;                     // evaluation blocks a TRAIN launch can carry (0: none)
  int rp_idle = 0;                    // CUs a TRAIN launch leaves idle for a device replay beside it (0: no cap)
  int eval_pending = -1;              // round whose evaluation rides on the next TRAIN launch
  int fin_pending = -1;               // round whose fused evaluation awaits its finaliser (it rides
                                      // on the next AGGREGATE launch, fs_plan_round)
  // fs_plan_set_nova: AGGREGATE is fs_aggregate_nova in this mode (0: the plain aggregate)
  int nova_mode = 0;
  const float* nova_b = nullptr;
  float nova_te = 1.f, nova_s0 = 1.f;
  // fs_plan_set_scaffold: TRAIN is fs_local_train_scaffold and AGGREGATE fs_aggregate_scaffold while on
  int scaffold = 0;
  float* sc_c = nullptr;              // [C][ld] server variate
  float* sc_ci = nullptr;             // [N][C][ld] client variates
  const float* sc_r = nullptr;        // [N], or [M] of a subset round
  float sc_cs = 0.f;
  // fs_plan_set_server_opt: AGGREGATE is fs_aggregate_opt with this rule (0: none)
  int opt_rule = 0;
  float* opt_m = nullptr;             // [C][ld] first moment
  float* opt_v = nullptr;             // [C][ld] second moment (AVGM: unused)
  float opt_eta = 0.f, opt_beta1 = 0.f, opt_omb1 = 0.f, opt_beta2 = 0.f, opt_omb2 = 0.f, opt_tau = 0.f;
  // fs_plan_set_qffl: AGGREGATE is fs_aggregate_qffl with u = the round's weights
  int qffl = 0;
  const float* qf_g = nullptr;        // [N], or [M] of a subset round
  double qf_L = 0.0;
  float* qf_S = nullptr;              // [C][ld] the folded update
  double* qf_n = nullptr;             // [N] / [M] squared update norms
  double* qf_hc = nullptr;            // [2] H, coef
  double* qf_nws = nullptr;
  int64_t qf_nws_doubles = 0;
  // fs_plan_set_robust: AGGREGATE is fs_aggregate_robust (0 off, FS_ROBUST_*)
  int robust = 0;
  double rb_trim = 0.0;
  // fs_plan_set_krum: AGGREGATE is fs_aggregate_krum
  int krum = 0;
  double kr_f = 0.0;
  int kr_m = 0;                       // 1 Krum, 0 M - f, else a count
  int32_t* kr_pick = nullptr;         // [N]
  double* kr_score = nullptr;         // [N]
  void* kr_ws = nullptr;
  int64_t kr_ws_bytes = 0;
  // fs_plan_set_rfa: AGGREGATE is fs_aggregate_rfa
  int rfa = 0;
  int rf_T = 0, rf_init = 0, rf_uniform = 0;
  double rf_nu = 0.0;
  double* rf_dist = nullptr;          // [N]
  float* rf_b = nullptr;              // [N]
  double* rf_obj = nullptr;           // [T + 2]
  void* rf_ws = nullptr;
  int64_t rf_ws_bytes = 0;
  // fs_plan_set_topk: AGGREGATE is fs_aggregate_topk
  int topk = 0;
  int64_t tk_count = 0;
  float* tk_e = nullptr;              // [N][C][ld] residuals (nullptr: no memory)
  float* tk_tau = nullptr;            // [N]
  int32_t* tk_kept = nullptr;         // [N]
  void* tk_ws = nullptr;
  int64_t tk_ws_bytes = 0;
  // fs_plan_set_dp: AGGREGATE is fs_aggregate_dp
  int dp = 0;
  double dp_S = 0.0, dp_z = 0.0;
  uint64_t dp_seed = 0;
  int dp_uniform = 0, dp_adaptive = 0;
  int64_t dp_cols = 0;                // the model's real columns D <= ld: the padding takes no noise
  double dp_gamma = 0.0, dp_eta = 0.0, dp_sigma_b = 0.0;
  double* dp_clip = nullptr;          // [1] the adaptive clip (nullptr: fixed)
  float* dp_c = nullptr;              // [N]
  double* dp_r = nullptr;             // [N]
  double* dp_state = nullptr;         // [FS_DP_STATE]
  void* dp_ws = nullptr;
  int64_t dp_ws_bytes = 0;
  hipStream_t copy = nullptr;
  hipEvent_t uploaded[2] = {nullptr, nullptr};
  hipEvent_t consumed[2] = {nullptr, nullptr};
  bool up_pending[2] = {false, false};
  bool cons_recorded[2] = {false, false};
  int slot_round[2] = {-1, -1};       // round whose shuffles slot s holds (set by the coordinator)
  int slot_M[2] = {0, 0};             // clients whose passes that round's replay wrote (0: all N)
  // chunked device replay (fs_plan_set_shuffle_chunk, K > 1): slot s holds the shuffles of
  // the K rounds of chunk c (rounds cK .. cK+K-1), generated by ONE launch; the local
  // training waits for the slot once per chunk and records its release once per chunk, so
  // consecutive rounds of a chunk run back to back with no cross-stream wait between them
  int chunk = 1;
  int64_t* d_pass_chunk = nullptr;    // [2][K*P]: rows, offset of every pass of a chunk
  int slot_chunk[2] = {-1, -1};       // chunk whose shuffles slot s holds (launched)
  int slot_nrounds[2] = {0, 0};       // rounds of that chunk generated
  int slot_waited[2] = {-1, -1};      // chunk the compute stream last waited for in slot s
  int fill_chunk = -1, fill_rounds = 0;   // chunk whose seeds are being collected, rounds so far
  int job_status = FS_OK;
  std::string job_error;
  fs::Pool* pool = nullptr;
  // coordinator: shuffle jobs (round, seeds) in order
  std::thread coord;
  std::mutex m;
  std::condition_variable cv, done;
  std::deque<ShuffleJob> jobs;
  bool stop = false;
};

using namespace fs;

static int hip_fail(const char* what, hipError_t e) {
  return fail(FS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define FS_HIP(call, what)                          \
  do {                                              \
    hipError_t e_ = (call);                         \
    if (e_ != hipSuccess) return hip_fail(what, e_); \
  } while (0)

extern "C" int64_t fs_plan_desc_size(void) { return (int64_t)sizeof(fs_plan_desc); }

static int run_shuffle_job(fs_plan* p, const ShuffleJob& job);

static void coordinator(fs_plan* p) {
  for (;;) {
    ShuffleJob job;
    {
      std::unique_lock<std::mutex> lk(p->m);
      p->cv.wait(lk, [p] { return p->stop || !p->jobs.empty(); });
      if (p->jobs.empty()) return;
      job = std::move(p->jobs.front());
    }
    const int rc = run_shuffle_job(p, job);
    std::lock_guard<std::mutex> lk(p->m);
    p->jobs.pop_front();
    if (rc != FS_OK && p->job_status == FS_OK) {
      p->job_status = rc;
      p->job_error = fs_last_error();
    }
    p->done.notify_all();
  }
}

extern "C" int fs_plan_destroy(fs_plan* p) {
  if (!p) return FS_OK;
  if (p->coord.joinable()) {
    {
      std::lock_guard<std::mutex> lk(p->m);
      p->stop = true;
    }
    p->cv.notify_all();
    p->coord.join();
  }
  if (p->copy) (void)hipStreamSynchronize(p->copy);
  for (int s = 0; s < 2; ++s) {
    if (p->h_perm[s]) (void)hipHostFree(p->h_perm[s]);
    if (p->d_perm[s]) (void)hipFree(p->d_perm[s]);
    if (p->uploaded[s]) (void)hipEventDestroy(p->uploaded[s]);
    if (p->consumed[s]) (void)hipEventDestroy(p->consumed[s]);
  }
  for (int s = 0; s < fs_plan::SEED_SLOTS; ++s) {
    if (p->h_seed[s]) (void)hipHostFree(p->h_seed[s]);
    if (p->d_seed[s]) (void)hipFree(p->d_seed[s]);
    if (p->seed_read[s]) (void)hipEventDestroy(p->seed_read[s]);
  }
  if (p->d_pass) (void)hipFree(p->d_pass);
  if (p->d_pass_chunk) (void)hipFree(p->d_pass_chunk);
  if (p->copy) (void)hipStreamDestroy(p->copy);
  delete p->pool;
  delete p;
  return FS_OK;
}

// int64 entries of one pinned seed slot (and of its device copy) for chunks of `rounds` rounds of P
// passes: the chunk's seeds [rounds][P] -- and never fewer than 3 * P, since a subset round lays
// its seeds and its pass table out as [3][P] (device_shuffle_subset) whenever the chunk is 1,
// whatever the chunk was set to before
static int64_t seed_slot_entries(int64_t P, int rounds) {
  return std::max<int64_t>(1, std::max<int64_t>((int64_t)rounds * P, 3 * P));
}

extern "C" int fs_plan_create(const fs_plan_desc* desc, fs_plan** out) {
  FS_REQUIRE(desc && out, "null pointer");
  const fs_plan_desc& d = *desc;
  FS_REQUIRE(d.N >= 1 && d.E >= 0 && d.C >= 1 && d.ld >= 64 && d.ld % 64 == 0, "bad sizes");
  FS_REQUIRE(d.loss == 0 || d.loss == 1, "loss must be 0 (cross-entropy) or 1 (MSE)");
  FS_REQUIRE(d.h_n && d.d_phi && d.d_row_off && (d.loss ? (const void*)d.d_y : (const void*)d.d_labels) && d.d_W_g &&
                 d.d_W_out && d.d_loss_hist,
             "null pointer");
  // MSE (tools.py:183-184): one output column, one workgroup per client, no exchange workspace
  FS_REQUIRE(d.loss == 0 || (d.C == 1 && d.G == 1), "the MSE plan needs C == 1 and G == 1");
  *out = nullptr;
  fs_plan* p = new fs_plan();
  p->d = d;
  int64_t rows = 0;
  for (int j = 0; j < d.N; ++j) {
    if (d.h_n[j] < 0) {
      delete p;
      return fail(FS_EINVAL, "fs_plan_create: negative client size");
    }
    for (int e = 0; e < d.E; ++e) {
      p->n.push_back(d.h_n[j]);
      p->off.push_back((int64_t)d.E * rows + (int64_t)e * d.h_n[j]);
    }
    rows += d.h_n[j];
  }
  p->perm_len = std::max<int64_t>(1, (int64_t)d.E * rows);
  const int64_t P = (int64_t)p->n.size();
  for (int64_t v : p->n) p->max_n = std::max(p->max_n, v);
  {
    int64_t mx = 0;
    for (int j = 0; j < d.N; ++j) mx = std::max(mx, d.h_n[j]);
    p->max_client_steps = std::max<int64_t>(1, (int64_t)d.E * ((mx + d.B - 1) / std::max(1, d.B)));
  }
  // FS_PHASE_EVAL_DEFER: a parallel split launch that leaves CUs idle evaluates the previous
  // round's global model on them (fs_tuning.no_eval_fuse turns this off)
  // (the MSE plan never fuses: G == 1, fuse_E stays 0 and a deferred evaluation runs as a launch of its own)
  if (d.loss == 0 && d.d_phi_t && d.n_t > 0 && d.d_labels_t && d.d_eval_ws && d.C <= 16 && d.G > 1 && !(d.G & FS_G_WIDE) &&
      !d.chained) {   // (the wide form is one workgroup per client: nothing to fuse into, as under loss = 1)
    if (!fs::tuning().no_eval_fuse) {
      const int idle = fs::split_idle_cus(d.N, d.C, d.B, d.ld, d.G, 0);
      p->fuse_E = (int)std::min<int64_t>(idle, (d.n_t + 15) / 16);
    }
  }
  // A device replay that runs beside a parallel exchanging TRAIN launch stays on some of the CUs
  // that launch leaves idle, the same number on every XCD (rp_cap_blocks, randperm_geom.h; DESIGN
  // 4.4): a group needs every partner resident, and a replay wave on a CU a group needs holds the
  // whole launch up for the length of a pass.  Launches that leave fewer than 16 CUs idle, chained
  // launches and FedAMW's replay (shuffle_after_train: beside the Z GEMM) keep the uncapped geometry.
  // (The cap's "at most half of an XCD's idle CUs" is there for the fused evaluation's blocks; it
  // holds whether or not this plan fuses one -- fuse_E == 0 with no_eval_fuse or no test set -- since
  // the replay ends inside its chunk on that share anyway: one rule, not two.)
  if (RP_CAPPED && d.shuffle_device && d.loss == 0 && d.G > 1 && !(d.G & FS_G_WIDE) && !d.chained &&
      !d.shuffle_after_train)
    p->rp_idle = fs::split_idle_cus(d.N, d.C, d.B, d.ld, d.G, 0);
  hipError_t e = hipSuccess;
  for (int s = 0; s < 2 && e == hipSuccess; ++s) {
    if (!d.shuffle_device) {
      e = hipHostMalloc(reinterpret_cast<void**>(&p->h_perm[s]), sizeof(int32_t) * p->perm_len, hipHostMallocDefault);
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_perm[s]), sizeof(int32_t) * p->perm_len);
    // zeroed once: a subset round's replay writes the sampled clients' passes only, and a pass
    // never written must still index inside its client (row 0) should a caller train it
    if (e == hipSuccess) e = hipMemset(p->d_perm[s], 0, sizeof(int32_t) * p->perm_len);
    if (e == hipSuccess && p->h_perm[s]) std::memset(p->h_perm[s], 0, sizeof(int32_t) * p->perm_len);
    // ordering-only events: no timestamps and no system-scope release when they complete (the
    // waits are device-side, and the host only needs the seed upload's completion, not the
    // visibility of device writes)
    const unsigned evf = hipEventDisableTiming | (unsigned)hipEventDisableSystemFence;
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->uploaded[s], evf);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->consumed[s], evf);
  }
  if (d.shuffle_device) {
    // the seeds stay in pinned, coherent host memory that the shuffle kernel reads directly
    // (round 2, r02s2: no slower than a hipMemcpyAsync upload, and no copy on the side stream)
    p->seed_copy = false;
    for (int k = 0; k < fs_plan::SEED_SLOTS && e == hipSuccess; ++k) {
      // [3][P]: the seeds, then a subset round's pass table (rows, offset of each sampled pass)
      e = hipHostMalloc(reinterpret_cast<void**>(&p->h_seed[k]), sizeof(int64_t) * seed_slot_entries(P, 1),
                        p->seed_copy ? hipHostMallocDefault : (hipHostMallocMapped | hipHostMallocCoherent));
      if (e == hipSuccess && !p->seed_copy)
        e = hipHostGetDevicePointer(reinterpret_cast<void**>(&p->h_seed_dev[k]), p->h_seed[k], 0);
      if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_seed[k]), sizeof(int64_t) * std::max<int64_t>(1, P));
      if (e == hipSuccess) e = hipEventCreateWithFlags(&p->seed_read[k], hipEventDisableTiming | hipEventDisableSystemFence);
    }
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->copy, hipStreamNonBlocking);
  if (e == hipSuccess && d.shuffle_device && P > 0) {
    std::vector<int64_t> h(2 * P);
    std::copy(p->n.begin(), p->n.end(), h.begin());
    std::copy(p->off.begin(), p->off.end(), h.begin() + P);
    e = hipMalloc(reinterpret_cast<void**>(&p->d_pass), sizeof(int64_t) * 2 * P);
    if (e == hipSuccess) e = hipMemcpy(p->d_pass, h.data(), sizeof(int64_t) * 2 * P, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    fs_plan_destroy(p);
    return hip_fail("fs_plan_create", e);
  }
  if (!d.shuffle_device) {
    const int nthreads =
        d.host_threads > 0 ? d.host_threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    p->pool = new Pool(nthreads);
    int dev = 0;
    (void)hipGetDevice(&dev);
    p->coord = std::thread([p, dev] {
      (void)hipSetDevice(dev);
      coordinator(p);
    });
  }
  *out = p;
  return FS_OK;
}

// the workgroups a replay of `npasses` passes, the shuffles of `rounds` rounds, may take (0: no cap)
static int plan_rp_cap(const fs_plan* p, int64_t npasses, int rounds) {
  return fs::rp_cap_blocks(p->rp_idle, npasses, p->max_n, rounds);
}

// Device replay: upload the seeds and launch fs_randperm_device on the side stream.
static int device_shuffle(fs_plan* p, const int64_t* h_seeds, int t) {
  const int s = t & 1;
  const int64_t P = (int64_t)p->n.size();
  const int k = t % fs_plan::SEED_SLOTS;
  if (p->seed_pending[k]) FS_HIP(hipEventSynchronize(p->seed_read[k]), "fs_plan_shuffle");   // pinned seeds free
  std::memcpy(p->h_seed[k], h_seeds, sizeof(int64_t) * P);
  if (p->cons_recorded[s]) FS_HIP(hipStreamWaitEvent(p->copy, p->consumed[s], 0), "fs_plan_shuffle");
  // optionally also behind the latest local training (the other slot's consumer)
  if (p->d.shuffle_after_train && p->cons_recorded[s ^ 1])
    FS_HIP(hipStreamWaitEvent(p->copy, p->consumed[s ^ 1], 0), "fs_plan_shuffle");
  if (p->seed_copy)
    FS_HIP(hipMemcpyAsync(p->d_seed[k], p->h_seed[k], sizeof(int64_t) * P, hipMemcpyHostToDevice, p->copy),
           "fs_plan_shuffle");
  const int64_t* seeds = p->seed_copy ? p->d_seed[k] : p->h_seed_dev[k];
  // (no error word: p->max_n is the maximum of the plan's own pass sizes)
  const int rc = fs::randperm_device(seeds, p->d_pass, p->d_pass + P, P, p->max_n, p->d_perm[s], nullptr,
                                     plan_rp_cap(p, P, 1), p->copy);
  if (rc != FS_OK) return rc;
  FS_HIP(hipEventRecord(p->seed_read[k], p->copy), "fs_plan_shuffle");
  p->seed_pending[k] = true;
  FS_HIP(hipEventRecord(p->uploaded[s], p->copy), "fs_plan_shuffle");
  p->up_pending[s] = true;
  p->slot_round[s] = t;
  p->slot_M[s] = 0;
  return FS_OK;
}

// Device replay of a subset round: the M*E sampled passes only.  Their seeds and a per-round pass
// table (rows and offset of each sampled pass, the plan's own offsets E*row_off[j] + e*n_j) go
// side by side into the pinned seed slot, which one fs::randperm_device launch reads.
static int device_shuffle_subset(fs_plan* p, const int64_t* h_seeds, const int32_t* h_sel, int M, int t) {
  const int s = t & 1;
  const int E = p->d.E;
  const int64_t P = (int64_t)p->n.size(), PS = (int64_t)M * E;
  const int k = t % fs_plan::SEED_SLOTS;
  if (p->seed_pending[k]) FS_HIP(hipEventSynchronize(p->seed_read[k]), "fs_plan_shuffle_subset");   // pinned seeds free
  int64_t* hs = p->h_seed[k];
  std::memcpy(hs, h_seeds, sizeof(int64_t) * PS);
  for (int i = 0; i < M; ++i)
    for (int e = 0; e < E; ++e) {
      const int64_t pass = (int64_t)h_sel[i] * E + e;
      hs[P + (int64_t)i * E + e] = p->n[pass];
      hs[2 * P + (int64_t)i * E + e] = p->off[pass];
    }
  if (p->cons_recorded[s]) FS_HIP(hipStreamWaitEvent(p->copy, p->consumed[s], 0), "fs_plan_shuffle_subset");
  if (p->d.shuffle_after_train && p->cons_recorded[s ^ 1])
    FS_HIP(hipStreamWaitEvent(p->copy, p->consumed[s ^ 1], 0), "fs_plan_shuffle_subset");
  const int64_t* dev = p->h_seed_dev[k];
  // (no error word: p->max_n bounds every pass of the plan; the cap is the plan's -- M <= N clients
  // leave no fewer CUs idle than the N the cap was sized for)
  const int rc = fs::randperm_device(dev, dev + P, dev + 2 * P, PS, p->max_n, p->d_perm[s], nullptr,
                                     plan_rp_cap(p, PS, 1), p->copy);
  if (rc != FS_OK) return rc;
  FS_HIP(hipEventRecord(p->seed_read[k], p->copy), "fs_plan_shuffle_subset");
  p->seed_pending[k] = true;
  FS_HIP(hipEventRecord(p->uploaded[s], p->copy), "fs_plan_shuffle_subset");
  p->up_pending[s] = true;
  p->slot_round[s] = t;
  p->slot_M[s] = M;
  return FS_OK;
}

// Chunked device replay: the seeds of rounds cK .. cK+K-1 are collected in one pinned seed
// slot; one fs_randperm_device launch over all K*P passes fills shuffle slot c & 1.
extern "C" int fs_plan_set_shuffle_chunk(fs_plan* p, int rounds) {
  FS_REQUIRE(p && rounds >= 1 && rounds <= 64, "bad arguments");
  FS_REQUIRE(p->d.shuffle_device, "fs_plan_set_shuffle_chunk: device replay only");
  FS_REQUIRE(!p->seed_pending[0] && p->slot_round[0] < 0 && p->slot_round[1] < 0 && p->slot_chunk[0] < 0 &&
                 p->fill_chunk < 0,
             "fs_plan_set_shuffle_chunk: set before the first shuffle");
  if (rounds == p->chunk) return FS_OK;
  const int64_t P = (int64_t)p->n.size();
  const int64_t KP = std::max<int64_t>(1, (int64_t)rounds * P);
  for (int s = 0; s < 2; ++s) {
    FS_HIP(hipFree(p->d_perm[s]), "fs_plan_set_shuffle_chunk");
    p->d_perm[s] = nullptr;
    FS_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_perm[s]), sizeof(int32_t) * p->perm_len * rounds),
           "fs_plan_set_shuffle_chunk");
    // zeroed as at creation (a pass no replay ever wrote indexes row 0 of its client)
    FS_HIP(hipMemset(p->d_perm[s], 0, sizeof(int32_t) * p->perm_len * rounds), "fs_plan_set_shuffle_chunk");
  }
  const int64_t slot = seed_slot_entries(P, rounds);
  for (int k = 0; k < fs_plan::SEED_SLOTS; ++k) {
    FS_HIP(hipHostFree(p->h_seed[k]), "fs_plan_set_shuffle_chunk");
    FS_HIP(hipFree(p->d_seed[k]), "fs_plan_set_shuffle_chunk");
    p->h_seed[k] = nullptr;
    p->d_seed[k] = nullptr;
    FS_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->h_seed[k]), sizeof(int64_t) * slot,
                         p->seed_copy ? hipHostMallocDefault : (hipHostMallocMapped | hipHostMallocCoherent)),
           "fs_plan_set_shuffle_chunk");
    if (!p->seed_copy)
      FS_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&p->h_seed_dev[k]), p->h_seed[k], 0),
             "fs_plan_set_shuffle_chunk");
    FS_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_seed[k]), sizeof(int64_t) * slot), "fs_plan_set_shuffle_chunk");
  }
  if (p->d_pass_chunk) FS_HIP(hipFree(p->d_pass_chunk), "fs_plan_set_shuffle_chunk");
  p->d_pass_chunk = nullptr;
  if (P > 0) {
    std::vector<int64_t> h(2 * KP);
    for (int r = 0; r < rounds; ++r)
      for (int64_t i = 0; i < P; ++i) {
        h[r * P + i] = p->n[i];
        h[KP + r * P + i] = p->off[i] + (int64_t)r * p->perm_len;
      }
    FS_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_pass_chunk), sizeof(int64_t) * 2 * KP),
           "fs_plan_set_shuffle_chunk");
    FS_HIP(hipMemcpy(p->d_pass_chunk, h.data(), sizeof(int64_t) * 2 * KP, hipMemcpyHostToDevice),
           "fs_plan_set_shuffle_chunk");
  }
  p->chunk = rounds;
  return FS_OK;
}

// launch the shuffles of the collected rounds of chunk p->fill_chunk into slot (chunk & 1)
static int launch_chunk(fs_plan* p) {
  const int c = p->fill_chunk, nr = p->fill_rounds, K = p->chunk;
  const int s = c & 1, k = c % fs_plan::SEED_SLOTS;
  const int64_t P = (int64_t)p->n.size(), KP = std::max<int64_t>(1, (int64_t)K * P);
  // the slot's previous chunk (c - 2) released it after its last local training
  if (p->cons_recorded[s]) FS_HIP(hipStreamWaitEvent(p->copy, p->consumed[s], 0), "fs_plan_shuffle");
  if (P > 0) {
    if (p->seed_copy)
      FS_HIP(hipMemcpyAsync(p->d_seed[k], p->h_seed[k], sizeof(int64_t) * nr * P, hipMemcpyHostToDevice, p->copy),
             "fs_plan_shuffle");
    const int64_t* seeds = p->seed_copy ? p->d_seed[k] : p->h_seed_dev[k];
    // (no error word: the plan's max_n is the maximum of its own pass sizes, so no pass exceeds it)
    const int rc = fs::randperm_device(seeds, p->d_pass_chunk, p->d_pass_chunk + KP, nr * P, p->max_n, p->d_perm[s],
                                       nullptr, plan_rp_cap(p, nr * P, nr), p->copy);
    if (rc != FS_OK) return rc;
  }
  FS_HIP(hipEventRecord(p->seed_read[k], p->copy), "fs_plan_shuffle");
  p->seed_pending[k] = true;
  FS_HIP(hipEventRecord(p->uploaded[s], p->copy), "fs_plan_shuffle");
  p->up_pending[s] = true;
  p->slot_chunk[s] = c;
  p->slot_nrounds[s] = nr;
  p->fill_chunk = -1;
  p->fill_rounds = 0;
  return FS_OK;
}

static int chunk_shuffle(fs_plan* p, const int64_t* h_seeds, int t) {
  const int K = p->chunk, c = t / K, r = t % K;
  const int64_t P = (int64_t)p->n.size();
  FS_REQUIRE(r == (p->fill_chunk == c ? p->fill_rounds : 0) && (r > 0 || p->fill_chunk < 0),
             "rounds must be prepared in order");
  if (r == 0) {
    const int k = c % fs_plan::SEED_SLOTS;
    if (p->seed_pending[k]) FS_HIP(hipEventSynchronize(p->seed_read[k]), "fs_plan_shuffle");   // seed slot free
    p->fill_chunk = c;
    p->fill_rounds = 0;
  }
  std::memcpy(p->h_seed[c % fs_plan::SEED_SLOTS] + (int64_t)r * P, h_seeds, sizeof(int64_t) * P);
  ++p->fill_rounds;
  return r == K - 1 ? launch_chunk(p) : FS_OK;
}

// Timing events for measurement (bench.py's per-launch durations): timestamps, but no
// system-scope release when recorded (hipEventDisableSystemFence) -- a default timing event
// between two kernels of a round cost ~3.5 us of GPU idle each at config 2 (r02s2z).
extern "C" int fs_timer_create(void** ev) {
  FS_REQUIRE(ev, "null pointer");
  hipEvent_t e = nullptr;
  FS_HIP(hipEventCreateWithFlags(&e, (unsigned)hipEventDisableSystemFence), "fs_timer_create");
  *ev = e;
  return FS_OK;
}
extern "C" int fs_timer_record(void* ev, void* stream) {
  FS_REQUIRE(ev, "null pointer");
  FS_HIP(hipEventRecord(reinterpret_cast<hipEvent_t>(ev), reinterpret_cast<hipStream_t>(stream)), "fs_timer_record");
  return FS_OK;
}
extern "C" int fs_timer_elapsed_ms(void* start, void* end, float* ms) {
  FS_REQUIRE(start && end && ms, "null pointer");
  FS_HIP(hipEventSynchronize(reinterpret_cast<hipEvent_t>(end)), "fs_timer_elapsed_ms");
  FS_HIP(hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(start), reinterpret_cast<hipEvent_t>(end)),
         "fs_timer_elapsed_ms");
  return FS_OK;
}
extern "C" int fs_timer_destroy(void* ev) {
  if (ev) FS_HIP(hipEventDestroy(reinterpret_cast<hipEvent_t>(ev)), "fs_timer_destroy");
  return FS_OK;
}

extern "C" int fs_plan_eval_blocks(const fs_plan* p) {
  FS_REQUIRE(p, "bad arguments");
  return p->fuse_E;
}

extern "C" int fs_plan_shuffle_flush(fs_plan* p) {
  FS_REQUIRE(p, "bad arguments");
  return (p->chunk > 1 && p->fill_chunk >= 0) ? launch_chunk(p) : FS_OK;
}

// Prepare round t's shuffles: device replay is enqueued here; a host replay job is queued
// for the coordinator thread and this returns at once.
extern "C" int fs_plan_shuffle(fs_plan* p, const int64_t* h_seeds, int t) {
  FS_REQUIRE(p && (h_seeds || p->n.empty()) && t >= 0, "bad arguments");
  if (p->d.shuffle_device) {
    if (p->chunk > 1) return chunk_shuffle(p, h_seeds, t);
    if (p->n.empty()) {
      p->slot_round[t & 1] = t;
      return FS_OK;
    }
    return device_shuffle(p, h_seeds, t);
  }
  {
    std::lock_guard<std::mutex> lk(p->m);
    if (p->job_status != FS_OK) return fail(p->job_status, p->job_error);
    p->jobs.push_back(ShuffleJob{t, std::vector<int64_t>(h_seeds, h_seeds + p->n.size()), {}});
  }
  p->cv.notify_all();
  return FS_OK;
}

// what both subset entry points reject (after their null and range checks)
static int subset_admits(const fs_plan* p, const char* who) {
  if (p->d.chained)
    return fail(FS_EUNSUPPORTED, std::string(who) + ": chained plans walk the clients by position, not through the "
                                                    "order table; subset rounds need parallel clients");
  if (p->chunk > 1)
    return fail(FS_EINVAL, std::string(who) + ": subset rounds use per-round shuffle slots (fs_plan_set_shuffle_chunk(1))");
  return FS_OK;
}

// ABI 22: prepare a subset round's shuffles -- the M*E passes of the sampled clients h_sel
// (strictly ascending client ids), seeds sel-major / epoch-minor -- into slot t % 2.
extern "C" int fs_plan_shuffle_subset(fs_plan* p, const int64_t* h_seeds, const int32_t* h_sel, int M, int t) {
  FS_REQUIRE(p && h_sel && t >= 0, "bad arguments");
  FS_REQUIRE(M >= 1 && M <= p->d.N, "M must be in [1, N]");
  FS_REQUIRE(h_seeds || p->n.empty(), "null pointer");
  if (int rc = subset_admits(p, "fs_plan_shuffle_subset")) return rc;
  for (int i = 0; i < M; ++i)
    FS_REQUIRE(h_sel[i] >= 0 && h_sel[i] < p->d.N && (i == 0 || h_sel[i] > h_sel[i - 1]),
               "sampled client ids must be strictly ascending and in [0, N)");
  if (p->d.shuffle_device) {
    if (p->n.empty()) {
      p->slot_round[t & 1] = t;
      p->slot_M[t & 1] = M;
      return FS_OK;
    }
    return device_shuffle_subset(p, h_seeds, h_sel, M, t);
  }
  {
    std::lock_guard<std::mutex> lk(p->m);
    if (p->job_status != FS_OK) return fail(p->job_status, p->job_error);
    p->jobs.push_back(ShuffleJob{t, std::vector<int64_t>(h_seeds, h_seeds + (int64_t)M * p->d.E),
                                 std::vector<int32_t>(h_sel, h_sel + M)});
  }
  p->cv.notify_all();
  return FS_OK;
}

static int run_shuffle_job(fs_plan* p, const ShuffleJob& job) {
  const int t = job.t;
  const int64_t* h_seeds = job.seeds.data();
  const int s = t & 1;
  if (p->up_pending[s]) FS_HIP(hipEventSynchronize(p->uploaded[s]), "fs_plan_shuffle");   // pinned slot free
  int32_t* out = p->h_perm[s];
  const int E = p->d.E;
  // a subset round: seed i belongs to pass sel[i / E] * E + i % E of the plan's table
  const std::function<void(int64_t)> one = [&](int64_t i) {
    const int64_t pass = job.sel.empty() ? i : (int64_t)job.sel[i / E] * E + i % E;
    replay_randperm((uint64_t)h_seeds[i], p->n[pass], out + p->off[pass]);
  };
  p->pool->run(job.sel.empty() ? (int64_t)p->n.size() : (int64_t)job.sel.size() * E, one);
  // the device slot is rewritten only after the local training that read it has finished
  if (p->cons_recorded[s]) FS_HIP(hipStreamWaitEvent(p->copy, p->consumed[s], 0), "fs_plan_shuffle");
  FS_HIP(hipMemcpyAsync(p->d_perm[s], out, sizeof(int32_t) * p->perm_len, hipMemcpyHostToDevice, p->copy),
         "fs_plan_shuffle");
  FS_HIP(hipEventRecord(p->uploaded[s], p->copy), "fs_plan_shuffle");
  p->up_pending[s] = true;
  std::lock_guard<std::mutex> lk(p->m);
  p->slot_round[s] = t;
  p->slot_M[s] = (int)job.sel.size();
  return FS_OK;
}

// round te's evaluation as a launch of its own, by the plan's loss
static int plan_eval(const fs_plan_desc& d, int te, hipStream_t st) {
  double* out = d.d_eval_hist + 2 * (int64_t)te;
  if (d.loss) return fs::eval_mse(d.d_phi_t, d.ld, d.d_y_t, d.n_t, d.d_W_g, out, d.d_eval_ws, st);
  return fs_eval(d.d_phi_t, d.ld, d.d_labels_t, d.n_t, d.d_W_g, d.C, out, d.d_eval_ws, st);
}

// round t's local training on the shuffles at `perms`, by the plan's loss
// a subset round's sampled clients (fs_plan_round_subset): M ids ascending (the aggregate's fold
// order) and in dispatch order (the training launch's), and their weights; all on the device
struct Subset {
  const int32_t* sel;
  const int32_t* order;
  const float* q;
  int M;
};

// (a subset round: the same launch over the M clients of sub->order -- every form finds its
// client through the order table, so W_out[j] and loss[j] stay indexed by client id)
static int plan_train(fs_plan* p, const int32_t* perms, int t, float lr, const fs::FuseEval* fuse, const Subset* sub,
                      hipStream_t st) {
  const fs_plan_desc& d = p->d;
  double* loss = d.d_loss_hist + (int64_t)t * d.N;
  const int n = sub ? sub->M : d.N;
  const int32_t* order = sub ? sub->order : d.d_order;
  if (p->scaffold)
    return fs::local_train_scaffold(d.d_phi, d.ld, d.d_row_off, d.d_labels, perms, order, n, d.C, d.B, d.E, lr, d.lam,
                                    d.reg, d.d_W_g, p->sc_c, p->sc_ci, d.d_W_out, loss, st);
  if (d.loss)
    return fs::local_train_mse(d.d_phi, d.ld, d.d_row_off, d.d_y, perms, order, n, d.B, d.E, lr, d.mu, d.prox,
                               d.lam, d.reg, d.chained, d.d_W_g, d.d_W_out, loss, st);
  return fs::local_train(d.d_phi, d.ld, d.d_row_off, d.d_labels, perms, order, n, d.C, d.B, d.E, lr, d.mu, d.prox,
                         d.lam, d.reg, d.chained, d.d_W_g, d.d_W_out, loss, d.G, d.d_ws, d.ws_bytes, st,
                         p->max_client_steps, fuse);
}

// the deferred evaluation of round p->eval_pending as a launch of its own
static int flush_eval(fs_plan* p, hipStream_t st) {
  if (p->eval_pending < 0) return FS_OK;
  const int te = p->eval_pending;
  p->eval_pending = -1;
  return plan_eval(p->d, te, st);
}

// ABI 15: complete every evaluation this plan still holds -- a deferred one
// not yet carried by a TRAIN launch (as its own fs_eval launch) and a fused one whose finaliser
// waits for the next AGGREGATE -- so d_eval_hist is final once `stream` reaches this point.
extern "C" int fs_plan_eval_flush(fs_plan* p, void* stream) {
  FS_REQUIRE(p, "bad arguments");
  const fs_plan_desc& d = p->d;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (p->fin_pending >= 0) {
    const fs::EvalFinalize f{d.d_eval_ws, p->fuse_E, (int)d.n_t, d.d_eval_hist + 2 * (int64_t)p->fin_pending};
    p->fin_pending = -1;
    const int rc = fs::eval_finalize_launch(f.part, f.nb, f.n, f.out, st);
    if (rc != FS_OK) return rc;
  }
  return flush_eval(p, st);
}

// one round's launches; sub: the sampled clients of a subset round (nullptr: all N)
static int plan_round(fs_plan* p, int t, float lr, int phases, const float* d_p_override, const Subset* sub,
                      hipStream_t st) {
  const fs_plan_desc& d = p->d;
  const int s = t & 1;
  // a deferred evaluation rides on this TRAIN launch (it reads W_g before the launch
  // rewrites nothing but W_out); anything else that follows it runs it on its own first
  fs::FuseEval fuse{d.d_phi_t, d.d_labels_t, (int)d.n_t, p->fuse_E, d.d_eval_ws};
  auto fin_of = [&](int te) { return fs::EvalFinalize{d.d_eval_ws, p->fuse_E, (int)d.n_t, d.d_eval_hist + 2 * (int64_t)te}; };
  // a finaliser left by an earlier TRAIN call rides on this call's aggregation -- unless this
  // call trains (its fused evaluation rewrites the partials) or does not aggregate: then first
  if (p->fin_pending >= 0 && ((phases & FS_PHASE_TRAIN) || !(phases & FS_PHASE_AGGREGATE))) {
    const fs::EvalFinalize f = fin_of(p->fin_pending);
    p->fin_pending = -1;
    const int rc = fs::eval_finalize_launch(f.part, f.nb, f.n, f.out, st);
    if (rc != FS_OK) return rc;
  }
  // (SCAFFOLD's training launch is one workgroup per client and carries no evaluation: never fused)
  const bool fused = (phases & FS_PHASE_TRAIN) && p->eval_pending >= 0 && p->fuse_E > 0 && !p->scaffold;
  if (p->eval_pending >= 0 && !fused) {
    const int rc = flush_eval(p, st);
    if (rc != FS_OK) return rc;
  }
  const int t_eval = p->eval_pending;
  if ((phases & FS_PHASE_TRAIN) && p->chunk > 1) {
    const int K = p->chunk, c = t / K, r = t % K, sc = c & 1;
    // a partly collected chunk (the last rounds of a run) is launched when first needed
    if (p->slot_chunk[sc] != c && p->fill_chunk == c) {
      const int rc = launch_chunk(p);
      if (rc != FS_OK) return rc;
    }
    if (p->slot_chunk[sc] != c || r >= p->slot_nrounds[sc])
      return fail(FS_EINVAL, "fs_plan_round: shuffles of this round were not prepared");
    if (p->slot_waited[sc] != c) {                 // once per chunk
      FS_HIP(hipStreamWaitEvent(st, p->uploaded[sc], 0), "fs_plan_round");
      p->slot_waited[sc] = c;
    }
    const int rc = plan_train(p, p->d_perm[sc] + (int64_t)r * p->perm_len, t, lr, fused ? &fuse : nullptr, nullptr, st);
    if (rc != FS_OK) return rc;
    if (r == p->slot_nrounds[sc] - 1) {            // the chunk's last round releases the slot
      FS_HIP(hipEventRecord(p->consumed[sc], st), "fs_plan_round");
      p->cons_recorded[sc] = true;
    }
  } else if (phases & FS_PHASE_TRAIN) {
    {
      // wait for this round's shuffle job (normally finished long ago)
      std::unique_lock<std::mutex> lk(p->m);
      p->done.wait(lk, [&] {
        if (p->job_status != FS_OK || p->slot_round[s] == t) return true;
        for (auto& j : p->jobs) if (j.t == t) return false;
        return true;                               // never queued
      });
      if (p->job_status != FS_OK) return fail(p->job_status, p->job_error);
      if (p->slot_round[s] != t) return fail(FS_EINVAL, "fs_plan_round: shuffles of this round were not prepared");
      if (p->slot_M[s] != (sub ? sub->M : 0))
        return fail(FS_EINVAL, "fs_plan_round: this round's shuffles were prepared for another client count");
    }
    FS_HIP(hipStreamWaitEvent(st, p->uploaded[s], 0), "fs_plan_round");
    const int rc = plan_train(p, p->d_perm[s], t, lr, fused ? &fuse : nullptr, sub, st);
    if (rc != FS_OK) return rc;
    FS_HIP(hipEventRecord(p->consumed[s], st), "fs_plan_round");
    p->cons_recorded[s] = true;
  }
  // the fused evaluation's finaliser rides on the next aggregation launch, this call's or a later
  // call's (the two are independent: the partials of round t_eval's W_g vs this round's W_out;
  // the FedAvg driver's TRAIN and AGGREGATE | EVAL calls of a round: one launch fewer per round)
  if (fused) {
    p->eval_pending = -1;
    p->fin_pending = t_eval;
  }
  if (phases & FS_PHASE_AGGREGATE) {
    const float* pw = sub ? sub->q : d_p_override ? d_p_override : d.d_p;
    if (!pw) return fail(FS_EINVAL, "fs_plan_round: no mixture weights");
    const int64_t len = (int64_t)d.C * d.ld;
    const fs::EvalFinalize fin = fin_of(p->fin_pending);
    const bool with_fin = p->fin_pending >= 0;
    p->fin_pending = -1;
    const int32_t* sel = sub ? sub->sel : nullptr;
    const int M = sub ? sub->M : d.N;
    const fs::EvalFinalize* f = with_fin ? &fin : nullptr;
    int rc;
    if (p->scaffold) {
      // (no finaliser rides on the dual fold: none is pending while SCAFFOLD is on, but one left
      // by a call before the setter would be lost -- it runs as a launch of its own)
      rc = with_fin ? fs::eval_finalize_launch(fin.part, fin.nb, fin.n, fin.out, st) : FS_OK;
      if (rc == FS_OK)
        rc = fs::aggregate_scaffold_launch(d.d_W_out, len, sel, pw, p->sc_r, p->sc_cs, M, len, d.d_W_g, p->sc_c,
                                           d.d_agg_ws, d.agg_ws_floats, d.agg_chunks, st);
    } else if (p->opt_rule)
      rc = fs::aggregate_opt_launch(d.d_W_out, len, sel, pw, p->opt_rule, p->opt_eta, p->opt_beta1, p->opt_omb1,
                                    p->opt_beta2, p->opt_omb2, p->opt_tau, M, len, d.d_W_g, p->opt_m, p->opt_v,
                                    d.d_agg_ws, d.agg_ws_floats, d.agg_chunks, f, st);
    else if (p->qffl)
      rc = fs::aggregate_qffl_launch(d.d_W_out, len, sel, pw, p->qf_g, p->qf_L, M, len, d.d_W_g, p->qf_S, p->qf_n,
                                     p->qf_hc, d.d_agg_ws, d.agg_ws_floats, d.agg_chunks, p->qf_nws, p->qf_nws_doubles,
                                     f, st);
    else if (p->robust) {
      // b from the round's own client count, so that 2b < M
      const int b = p->robust == FS_ROBUST_MEDIAN ? (M - 1) / 2 : std::min((int)std::floor(p->rb_trim * (double)M), (M - 1) / 2);
      rc = fs::aggregate_robust_launch(d.d_W_out, len, sel, M, len, b, d.d_W_g, f, st);
    } else if (p->krum) {
      // f and m from the round's own client count (M < 3: refused by the launch)
      const int kf = std::max(0, std::min((int)std::floor(p->kr_f * (double)M), (M - 3) / 2));
      const int km = p->kr_m == 1 ? 1 : p->kr_m == 0 ? M - kf : std::min(p->kr_m, M - kf);
      rc = fs::aggregate_krum_launch(d.d_W_out, len, sel, M, len, d.d_W_g, kf, km, d.d_W_g, p->kr_pick, p->kr_score,
                                     p->kr_ws, p->kr_ws_bytes, d.d_agg_ws, d.agg_ws_floats, d.agg_chunks, f, st);
    } else if (p->rfa) {
      rc = fs::aggregate_rfa_launch(d.d_W_out, len, sel, M, len, d.d_W_g, p->rf_uniform ? nullptr : pw,
                                    (float)(1.0 / (double)M), p->rf_T, p->rf_nu, p->rf_init, d.d_W_g, p->rf_dist,
                                    p->rf_b, p->rf_obj, p->rf_ws, p->rf_ws_bytes, f, st);
    } else if (p->topk) {
      rc = fs::aggregate_topk_launch(d.d_W_out, len, sel, pw, M, len, p->tk_count, d.d_W_g, p->tk_e, p->tk_tau,
                                     p->tk_kept, d.d_agg_ws, d.agg_ws_floats, d.agg_chunks, p->tk_ws, p->tk_ws_bytes, f,
                                     st);
    } else if (p->dp) {
      rc = fs::aggregate_dp_launch(d.d_W_out, len, sel, p->dp_uniform ? nullptr : pw, M, len, p->dp_S, p->dp_z,
                                   p->dp_seed, t, p->dp_adaptive, p->dp_gamma, p->dp_eta, p->dp_sigma_b, p->dp_clip,
                                   d.ld, p->dp_cols, d.d_W_g, p->dp_c, p->dp_r, p->dp_state, d.d_agg_ws, d.agg_ws_floats, d.agg_chunks,
                                   p->dp_ws, p->dp_ws_bytes, f, st);
    } else if (p->nova_mode)
      rc = fs::aggregate_nova_launch(d.d_W_out, len, sel, pw, p->nova_b, p->nova_te, p->nova_s0, p->nova_mode, d.d_W_g,
                                     M, len, d.d_W_g, d.d_agg_ws, d.agg_ws_floats, d.agg_chunks, f, st);
    else if (sub)
      rc = fs::aggregate_sel_launch(d.d_W_out, len, sel, pw, M, len, d.d_W_g, d.d_agg_ws, d.agg_ws_floats,
                                    d.agg_chunks, f, st);
    else
      rc = fs::aggregate_launch(d.d_W_out, len, pw, M, len, d.d_W_g, d.d_agg_ws, d.agg_ws_floats, d.agg_chunks, f, st);
    if (rc != FS_OK) return rc;
  }
  // (a finaliser still pending here is launched by the next fs_plan_round call -- any call that
  // trains or does not aggregate runs it first; results are read after such a call)
  if (phases & FS_PHASE_EVAL) {
    if (!(d.d_phi_t && (d.loss ? (const void*)d.d_y_t : (const void*)d.d_labels_t) && d.d_eval_hist && d.d_eval_ws))
      return fail(FS_EINVAL, "fs_plan_round: no test set");
    if ((phases & FS_PHASE_EVAL_DEFER) && (p->fuse_E > 0 || d.loss)) {
      p->eval_pending = t;                         // evaluated by the next TRAIN launch (MSE: never fused,
      return FS_OK;                                // a launch of its own in the call that would have carried it)
    }
    const int rc = plan_eval(d, t, st);
    if (rc != FS_OK) return rc;
  }
  return FS_OK;
}

// ABI 23: the aggregation rule of the AGGREGATE phases enqueued from now on (host state, read
// when a round call enqueues): 0 the plain aggregate, else fs_aggregate_nova in that mode with
// q = the round's weights, base = d_W_g (mode 2, in place).  d_b is read by those launches.
extern "C" int fs_plan_set_nova(fs_plan* p, int mode, const float* d_b, float te, float s0) {
  FS_REQUIRE(p, "bad arguments");
  FS_REQUIRE(mode == 0 || mode == FS_NOVA_REFERENCE || mode == FS_NOVA_UPDATES, "mode must be 0, 1 or 2");
  FS_REQUIRE(mode != FS_NOVA_REFERENCE || d_b, "mode 1 needs d_b");
  FS_REQUIRE(!(mode == FS_NOVA_UPDATES && p->d.chained),
             "mode 2 needs parallel clients (a chained client's W_j - W_g holds its predecessors' work)");
  FS_REQUIRE(mode == 0 || p->opt_rule == 0,
             "a FedNova aggregate and a server optimizer exclude each other (fs_plan_set_server_opt(0) first)");
  FS_REQUIRE(mode == 0 || !p->qffl, "a FedNova aggregate and q-FedAvg exclude each other (fs_plan_set_qffl(0) first)");
  FS_REQUIRE(mode == 0 || !p->robust, "a FedNova aggregate and a robust aggregate exclude each other (fs_plan_set_robust(0) first)");
  FS_REQUIRE(mode == 0 || !p->krum, "a FedNova aggregate and Krum exclude each other (fs_plan_set_krum(0) first)");
  FS_REQUIRE(mode == 0 || !p->rfa, "a FedNova aggregate and RFA exclude each other (fs_plan_set_rfa(0) first)");
  FS_REQUIRE(mode == 0 || !p->topk, "a FedNova aggregate and FedTopK exclude each other (fs_plan_set_topk(0) first)");
  FS_REQUIRE(mode == 0 || !p->dp, "a FedNova aggregate and DP-FedAvg exclude each other (fs_plan_set_dp(0) first)");
  p->nova_mode = mode;
  p->nova_b = mode == FS_NOVA_REFERENCE ? d_b : nullptr;
  p->nova_te = te;
  p->nova_s0 = s0;
  return FS_OK;
}

// Additive to ABI 23: SCAFFOLD rounds from now on (host state, read when a round call enqueues, as
// fs_plan_set_nova's).  on = 1: TRAIN launches fs_local_train_scaffold with the server variate d_c
// [C][ld] and the client variates d_ci [N][C][ld], AGGREGATE launches fs_aggregate_scaffold with the
// round's weights as q, d_r ([N]; [M] of a subset round) and cs, updating d_W_g and d_c in place.
// d_r and cs change with the round's lr and sample: call again before each round (allowed while
// on, whatever the plan holds).  Turning it on is refused while the plan holds a pending
// evaluation (fs_plan_eval_flush first).  on = 0: the plan as it was.
extern "C" int fs_plan_set_scaffold(fs_plan* p, int on, float* d_c, float* d_ci, const float* d_r, float cs) {
  FS_REQUIRE(p, "bad arguments");
  if (!on) {
    p->scaffold = 0;
    p->sc_c = p->sc_ci = nullptr;
    p->sc_r = nullptr;
    p->sc_cs = 0.f;
    return FS_OK;
  }
  FS_REQUIRE(d_c && d_ci && d_r, "null pointer");
  FS_REQUIRE(!p->d.chained, "SCAFFOLD needs parallel clients");
  FS_REQUIRE(p->d.loss == 0, "SCAFFOLD is implemented for cross-entropy only");
  FS_REQUIRE(p->d.B <= 64, "SCAFFOLD needs batch_size <= 64");
  FS_REQUIRE(!p->d.prox, "the prox term is not supported together with SCAFFOLD");
  FS_REQUIRE(p->nova_mode == 0, "SCAFFOLD and a FedNova aggregate exclude each other (fs_plan_set_nova(0) first)");
  FS_REQUIRE(p->opt_rule == 0, "SCAFFOLD and a server optimizer exclude each other (fs_plan_set_server_opt(0) first)");
  FS_REQUIRE(!p->qffl, "SCAFFOLD and q-FedAvg exclude each other (fs_plan_set_qffl(0) first)");
  FS_REQUIRE(!p->robust, "SCAFFOLD and a robust aggregate exclude each other (fs_plan_set_robust(0) first)");
  FS_REQUIRE(!p->krum, "SCAFFOLD and Krum exclude each other (fs_plan_set_krum(0) first)");
  FS_REQUIRE(!p->rfa, "SCAFFOLD and RFA exclude each other (fs_plan_set_rfa(0) first)");
  FS_REQUIRE(!p->topk, "SCAFFOLD and FedTopK exclude each other (fs_plan_set_topk(0) first)");
  FS_REQUIRE(!p->dp, "SCAFFOLD and DP-FedAvg exclude each other (fs_plan_set_dp(0) first)");
  FS_REQUIRE(p->scaffold || (p->eval_pending < 0 && p->fin_pending < 0),
             "the plan holds a pending evaluation (fs_plan_eval_flush first)");
  p->scaffold = 1;
  p->sc_c = d_c;
  p->sc_ci = d_ci;
  p->sc_r = d_r;
  p->sc_cs = cs;
  return FS_OK;
}

// Additive to ABI 23: a server optimizer on the AGGREGATE phases enqueued from now on (host
// state, read when a round call enqueues, as fs_plan_set_nova's).  rule FS_OPT_*: AGGREGATE launches
// fs_aggregate_opt with q = the round's weights, d_W_g and the moments d_m / d_v [C][ld] in place
// and the pending finaliser; TRAIN is unchanged.  rule 0: the plain aggregate again.
extern "C" int fs_plan_set_server_opt(fs_plan* p, int rule, float* d_m, float* d_v, float eta, float beta1, float omb1,
                                      float beta2, float omb2, float tau) {
  FS_REQUIRE(p, "bad arguments");
  if (rule == 0) {
    p->opt_rule = 0;
    p->opt_m = p->opt_v = nullptr;
    return FS_OK;
  }
  FS_REQUIRE(rule >= FS_OPT_AVGM && rule <= FS_OPT_YOGI, "rule must be 0 or FS_OPT_AVGM .. FS_OPT_YOGI");
  FS_REQUIRE(d_m && (rule == FS_OPT_AVGM || d_v), "null moments");
  FS_REQUIRE(d_m != d_v && d_m != p->d.d_W_g && d_v != p->d.d_W_g, "d_W_g, d_m and d_v must be different buffers");
  FS_REQUIRE(rule == FS_OPT_AVGM || tau > 0.f, "tau must be > 0");
  FS_REQUIRE(!p->d.chained,
             "a server optimizer needs parallel clients (a chained client's W_j - W_g holds its predecessors' work)");
  FS_REQUIRE(p->nova_mode == 0, "a server optimizer and a FedNova aggregate exclude each other (fs_plan_set_nova(0) first)");
  FS_REQUIRE(!p->scaffold, "a server optimizer and SCAFFOLD exclude each other (fs_plan_set_scaffold(0) first)");
  FS_REQUIRE(!p->qffl, "a server optimizer and q-FedAvg exclude each other (fs_plan_set_qffl(0) first)");
  FS_REQUIRE(!p->robust, "a server optimizer and a robust aggregate exclude each other (fs_plan_set_robust(0) first)");
  FS_REQUIRE(!p->krum, "a server optimizer and Krum exclude each other (fs_plan_set_krum(0) first)");
  FS_REQUIRE(!p->rfa, "a server optimizer and RFA exclude each other (fs_plan_set_rfa(0) first)");
  FS_REQUIRE(!p->topk, "a server optimizer and FedTopK exclude each other (fs_plan_set_topk(0) first)");
  FS_REQUIRE(!p->dp, "a server optimizer and DP-FedAvg exclude each other (fs_plan_set_dp(0) first)");
  p->opt_rule = rule;
  p->opt_m = d_m;
  p->opt_v = rule == FS_OPT_AVGM ? nullptr : d_v;
  p->opt_eta = eta;
  p->opt_beta1 = beta1;
  p->opt_omb1 = omb1;
  p->opt_beta2 = beta2;
  p->opt_omb2 = omb2;
  p->opt_tau = tau;
  return FS_OK;
}

// Additive to ABI 23: q-FedAvg on the AGGREGATE phases enqueued from now on (host state, read when a
// round call enqueues, as fs_plan_set_server_opt's).  on = 1: AGGREGATE launches fs_aggregate_qffl
// with u = the round's weights, g = d_g, Lc, d_W_g in place, the outputs d_S / d_n / d_hc, the
// plan's aggregation workspace and chunks, the norm workspace d_nws and the pending finaliser;
// TRAIN is unchanged.  Lc follows the round's lr: call again before each round (allowed while on).
// on = 0: the plain aggregate again.
extern "C" int fs_plan_set_qffl(fs_plan* p, int on, const float* d_g, double Lc, float* d_S, double* d_n, double* d_hc,
                                double* d_nws, int64_t nws_doubles) {
  FS_REQUIRE(p, "bad arguments");
  if (!on) {
    p->qffl = 0;
    p->qf_g = nullptr;
    p->qf_L = 0.0;
    p->qf_S = nullptr;
    p->qf_n = p->qf_hc = p->qf_nws = nullptr;
    p->qf_nws_doubles = 0;
    return FS_OK;
  }
  FS_REQUIRE(d_g && d_S && d_n && d_hc && d_nws, "null pointer");
  FS_REQUIRE(Lc > 0.0 && Lc <= 1.7976931348623157e308, "Lc must be finite and > 0");
  FS_REQUIRE(d_S != p->d.d_W_g, "d_S and d_W_g must be different buffers");
  FS_REQUIRE(nws_doubles >= fs::aggregate_qffl_ws_doubles_upto(p->d.N, (int64_t)p->d.C * p->d.ld),
             "d_nws is too small (the largest fs_aggregate_qffl_ws_doubles(M, C * ld) over M <= N)");
  FS_REQUIRE(!p->d.chained,
             "q-FedAvg needs parallel clients (a chained client's W_j - W_g holds its predecessors' work)");
  FS_REQUIRE(p->nova_mode == 0, "q-FedAvg and a FedNova aggregate exclude each other (fs_plan_set_nova(0) first)");
  FS_REQUIRE(!p->scaffold, "q-FedAvg and SCAFFOLD exclude each other (fs_plan_set_scaffold(0) first)");
  FS_REQUIRE(p->opt_rule == 0, "q-FedAvg and a server optimizer exclude each other (fs_plan_set_server_opt(0) first)");
  FS_REQUIRE(!p->robust, "q-FedAvg and a robust aggregate exclude each other (fs_plan_set_robust(0) first)");
  FS_REQUIRE(!p->krum, "q-FedAvg and Krum exclude each other (fs_plan_set_krum(0) first)");
  FS_REQUIRE(!p->rfa, "q-FedAvg and RFA exclude each other (fs_plan_set_rfa(0) first)");
  FS_REQUIRE(!p->topk, "q-FedAvg and FedTopK exclude each other (fs_plan_set_topk(0) first)");
  FS_REQUIRE(!p->dp, "q-FedAvg and DP-FedAvg exclude each other (fs_plan_set_dp(0) first)");
  p->qffl = 1;
  p->qf_g = d_g;
  p->qf_L = Lc;
  p->qf_S = d_S;
  p->qf_n = d_n;
  p->qf_hc = d_hc;
  p->qf_nws = d_nws;
  p->qf_nws_doubles = nws_doubles;
  return FS_OK;
}

// Additive to ABI 23: robust aggregation on the AGGREGATE phases enqueued from now on (host state,
// read when a round call enqueues).  on = 1: AGGREGATE launches fs_aggregate_robust over the round's
// rows into d_W_g with b from `mode`, `trim` and the round's own client count; the weights are
// ignored, TRAIN is unchanged.  on = 0: the plain aggregate again.
extern "C" int fs_plan_set_robust(fs_plan* p, int on, int mode, double trim) {
  FS_REQUIRE(p, "bad arguments");
  if (!on) {
    p->robust = 0;
    p->rb_trim = 0.0;
    return FS_OK;
  }
  FS_REQUIRE(mode == FS_ROBUST_TRIMMED_MEAN || mode == FS_ROBUST_MEDIAN,
             "mode must be FS_ROBUST_TRIMMED_MEAN or FS_ROBUST_MEDIAN");
  FS_REQUIRE(mode == FS_ROBUST_MEDIAN || (trim >= 0.0 && trim < 0.5), "trim must be in [0, 0.5)");
  FS_REQUIRE(!p->d.chained,
             "a robust aggregate needs parallel clients (a chained client's row holds its predecessors' work)");
  FS_REQUIRE(p->d.N <= fs_aggregate_robust_max_m(), "N is larger than fs_aggregate_robust_max_m()");
  FS_REQUIRE(p->nova_mode == 0, "a robust aggregate and a FedNova aggregate exclude each other (fs_plan_set_nova(0) first)");
  FS_REQUIRE(!p->scaffold, "a robust aggregate and SCAFFOLD exclude each other (fs_plan_set_scaffold(0) first)");
  FS_REQUIRE(p->opt_rule == 0,
             "a robust aggregate and a server optimizer exclude each other (fs_plan_set_server_opt(0) first)");
  FS_REQUIRE(!p->qffl, "a robust aggregate and q-FedAvg exclude each other (fs_plan_set_qffl(0) first)");
  FS_REQUIRE(!p->krum, "a robust aggregate and Krum exclude each other (fs_plan_set_krum(0) first)");
  FS_REQUIRE(!p->rfa, "a robust aggregate and RFA exclude each other (fs_plan_set_rfa(0) first)");
  FS_REQUIRE(!p->topk, "a robust aggregate and FedTopK exclude each other (fs_plan_set_topk(0) first)");
  FS_REQUIRE(!p->dp, "a robust aggregate and DP-FedAvg exclude each other (fs_plan_set_dp(0) first)");
  p->robust = mode;
  p->rb_trim = mode == FS_ROBUST_MEDIAN ? 0.0 : trim;
  return FS_OK;
}

// Additive to ABI 23: Krum / Multi-Krum on the AGGREGATE phases enqueued from now on (host state, read
// when a round call enqueues).  on = 1: AGGREGATE launches fs_aggregate_krum over the round's rows
// with x = d_W_g into d_W_g, f and m from f_frac, m_mode and the round's own client count; the
// weights are ignored, TRAIN is unchanged.  on = 0: the plain aggregate again.
extern "C" int fs_plan_set_krum(fs_plan* p, int on, double f_frac, int m_mode, int32_t* d_pick, double* d_score,
                                void* d_ws, int64_t ws_bytes) {
  FS_REQUIRE(p, "bad arguments");
  if (!on) {
    p->krum = 0;
    p->kr_f = 0.0;
    p->kr_m = 0;
    p->kr_pick = nullptr;
    p->kr_score = nullptr;
    p->kr_ws = nullptr;
    p->kr_ws_bytes = 0;
    return FS_OK;
  }
  FS_REQUIRE(f_frac >= 0.0 && f_frac < 0.5, "f_frac must be in [0, 0.5)");
  FS_REQUIRE(m_mode >= 0, "m_mode must be 1 (Krum), 0 (M - f) or a count");
  FS_REQUIRE(d_pick && d_score && d_ws, "null pointer");
  FS_REQUIRE(!p->d.chained, "Krum needs parallel clients (a chained client's row holds its predecessors' work)");
  FS_REQUIRE(p->d.N >= 3, "Krum needs N >= 3");
  FS_REQUIRE(p->d.N <= fs_aggregate_krum_max_m(), "N is larger than fs_aggregate_krum_max_m()");
  FS_REQUIRE(ws_bytes >= fs::aggregate_krum_ws_bytes(p->d.N, (int64_t)p->d.C * p->d.ld),
             "d_ws is too small (fs_aggregate_krum_ws_bytes(N, C * ld))");
  FS_REQUIRE(p->nova_mode == 0, "Krum and a FedNova aggregate exclude each other (fs_plan_set_nova(0) first)");
  FS_REQUIRE(!p->scaffold, "Krum and SCAFFOLD exclude each other (fs_plan_set_scaffold(0) first)");
  FS_REQUIRE(p->opt_rule == 0, "Krum and a server optimizer exclude each other (fs_plan_set_server_opt(0) first)");
  FS_REQUIRE(!p->qffl, "Krum and q-FedAvg exclude each other (fs_plan_set_qffl(0) first)");
  FS_REQUIRE(!p->robust, "Krum and a robust aggregate exclude each other (fs_plan_set_robust(0) first)");
  FS_REQUIRE(!p->rfa, "Krum and RFA exclude each other (fs_plan_set_rfa(0) first)");
  FS_REQUIRE(!p->topk, "Krum and FedTopK exclude each other (fs_plan_set_topk(0) first)");
  FS_REQUIRE(!p->dp, "Krum and DP-FedAvg exclude each other (fs_plan_set_dp(0) first)");
  p->krum = 1;
  p->kr_f = f_frac;
  p->kr_m = m_mode;
  p->kr_pick = d_pick;
  p->kr_score = d_score;
  p->kr_ws = d_ws;
  p->kr_ws_bytes = ws_bytes;
  return FS_OK;
}

// Additive to ABI 23: RFA on the AGGREGATE phases enqueued from now on (host state, read when a round
// call enqueues).  on = 1: AGGREGATE launches fs_aggregate_rfa over the round's rows with x = d_W_g
// into d_W_g under the round's weights (uniform: f32(1 / M)); TRAIN is unchanged.  on = 0: the plain
// aggregate again.
extern "C" int fs_plan_set_rfa(fs_plan* p, int on, int T, double nu, int init, int uniform, double* d_dist, float* d_b,
                               double* d_obj, void* d_ws, int64_t ws_bytes) {
  FS_REQUIRE(p, "bad arguments");
  if (!on) {
    p->rfa = 0;
    p->rf_T = p->rf_init = p->rf_uniform = 0;
    p->rf_nu = 0.0;
    p->rf_dist = nullptr;
    p->rf_b = nullptr;
    p->rf_obj = nullptr;
    p->rf_ws = nullptr;
    p->rf_ws_bytes = 0;
    return FS_OK;
  }
  FS_REQUIRE(T >= 0 && T <= FS_RFA_MAX_ITERS, "T must be in [0, 32]");
  FS_REQUIRE(nu > 0.0 && std::isfinite(nu), "nu must be positive and finite");
  FS_REQUIRE(init == FS_RFA_INIT_START || init == FS_RFA_INIT_MEAN, "init must be FS_RFA_INIT_START or FS_RFA_INIT_MEAN");
  FS_REQUIRE(d_dist && d_b && d_obj && d_ws, "null pointer");
  FS_REQUIRE(!p->d.chained, "RFA needs parallel clients (a chained client's row holds its predecessors' work)");
  FS_REQUIRE(p->d.N <= fs_aggregate_rfa_max_m(), "N is larger than fs_aggregate_rfa_max_m()");
  FS_REQUIRE(ws_bytes >= fs::aggregate_rfa_ws_bytes(p->d.N, (int64_t)p->d.C * p->d.ld),
             "d_ws is too small (fs_aggregate_rfa_ws_bytes(N, C * ld))");
  FS_REQUIRE(p->nova_mode == 0, "RFA and a FedNova aggregate exclude each other (fs_plan_set_nova(0) first)");
  FS_REQUIRE(!p->scaffold, "RFA and SCAFFOLD exclude each other (fs_plan_set_scaffold(0) first)");
  FS_REQUIRE(p->opt_rule == 0, "RFA and a server optimizer exclude each other (fs_plan_set_server_opt(0) first)");
  FS_REQUIRE(!p->qffl, "RFA and q-FedAvg exclude each other (fs_plan_set_qffl(0) first)");
  FS_REQUIRE(!p->robust, "RFA and a robust aggregate exclude each other (fs_plan_set_robust(0) first)");
  FS_REQUIRE(!p->krum, "RFA and Krum exclude each other (fs_plan_set_krum(0) first)");
  FS_REQUIRE(!p->topk, "RFA and FedTopK exclude each other (fs_plan_set_topk(0) first)");
  FS_REQUIRE(!p->dp, "RFA and DP-FedAvg exclude each other (fs_plan_set_dp(0) first)");
  p->rfa = 1;
  p->rf_T = T;
  p->rf_nu = nu;
  p->rf_init = init;
  p->rf_uniform = uniform ? 1 : 0;
  p->rf_dist = d_dist;
  p->rf_b = d_b;
  p->rf_obj = d_obj;
  p->rf_ws = d_ws;
  p->rf_ws_bytes = ws_bytes;
  return FS_OK;
}

// Additive to ABI 23: FedTopK on the AGGREGATE phases enqueued from now on (host state, read when a
// round call enqueues).  on = 1: AGGREGATE launches fs_aggregate_topk over the round's rows with the
// round's weights as q, d_W_g and the residuals d_e (nullptr: no memory) in place; TRAIN is
// unchanged.  on = 0: the plain aggregate again.
extern "C" int fs_plan_set_topk(fs_plan* p, int on, int64_t kcount, float* d_e, float* d_tau, int32_t* d_kept,
                                void* d_sws, int64_t sws_bytes) {
  FS_REQUIRE(p, "bad arguments");
  if (!on) {
    p->topk = 0;
    p->tk_count = 0;
    p->tk_e = p->tk_tau = nullptr;
    p->tk_kept = nullptr;
    p->tk_ws = nullptr;
    p->tk_ws_bytes = 0;
    return FS_OK;
  }
  FS_REQUIRE(kcount >= 1 && kcount <= (int64_t)p->d.C * p->d.ld, "kcount must be in [1, C * ld]");
  FS_REQUIRE(d_tau && d_kept, "null pointer");
  FS_REQUIRE(!d_e || (d_e != p->d.d_W_g && d_e != p->d.d_W_out), "d_e must not be d_W_g or d_W_out");
  FS_REQUIRE(!p->d.chained, "FedTopK needs parallel clients (a chained client's W_j - W_g holds its predecessors' work)");
  FS_REQUIRE(sws_bytes >= fs::aggregate_topk_ws_bytes(p->d.N, (int64_t)p->d.C * p->d.ld),
             "d_sws is too small (fs_aggregate_topk_ws_bytes(N, C * ld))");
  FS_REQUIRE(p->nova_mode == 0, "FedTopK and a FedNova aggregate exclude each other (fs_plan_set_nova(0) first)");
  FS_REQUIRE(!p->scaffold, "FedTopK and SCAFFOLD exclude each other (fs_plan_set_scaffold(0) first)");
  FS_REQUIRE(p->opt_rule == 0, "FedTopK and a server optimizer exclude each other (fs_plan_set_server_opt(0) first)");
  FS_REQUIRE(!p->qffl, "FedTopK and q-FedAvg exclude each other (fs_plan_set_qffl(0) first)");
  FS_REQUIRE(!p->robust, "FedTopK and a robust aggregate exclude each other (fs_plan_set_robust(0) first)");
  FS_REQUIRE(!p->krum, "FedTopK and Krum exclude each other (fs_plan_set_krum(0) first)");
  FS_REQUIRE(!p->rfa, "FedTopK and RFA exclude each other (fs_plan_set_rfa(0) first)");
  FS_REQUIRE(!p->dp, "FedTopK and DP-FedAvg exclude each other (fs_plan_set_dp(0) first)");
  p->topk = 1;
  p->tk_count = kcount;
  p->tk_e = d_e;
  p->tk_tau = d_tau;
  p->tk_kept = d_kept;
  p->tk_ws = d_sws;
  p->tk_ws_bytes = sws_bytes;
  return FS_OK;
}

// Additive to ABI 23: DP-FedAvg on the AGGREGATE phases enqueued from now on (host state, read when a
// round call enqueues).  on = 1: AGGREGATE launches fs_aggregate_dp over the round's rows with the
// round's weights as q (uniform: 1 / M), the call's t as the noise round, d_W_g in place; TRAIN is
// unchanged.  on = 0: the plain aggregate again.
extern "C" int fs_plan_set_dp(fs_plan* p, int on, double S, double z, uint64_t seed, int uniform, int adaptive,
                              double gamma, double eta, double sigma_b, double* d_clip, int64_t cols, float* d_c,
                              double* d_r, double* d_state, void* d_sws, int64_t sws_bytes) {
  FS_REQUIRE(p, "bad arguments");
  if (!on) {
    p->dp = 0;
    p->dp_clip = p->dp_r = p->dp_state = nullptr;
    p->dp_c = nullptr;
    p->dp_ws = nullptr;
    p->dp_ws_bytes = 0;
    return FS_OK;
  }
  const double dmax = 1.7976931348623157e308;
  FS_REQUIRE(S > 0.0, "the clip S must be > 0 (+Inf: no clipping)");
  FS_REQUIRE(z >= 0.0 && z <= dmax, "the noise multiplier z must be finite and >= 0");
  FS_REQUIRE(z == 0.0 || S <= dmax, "noise (z > 0) needs a finite clip");
  FS_REQUIRE(!adaptive || (d_clip && S <= dmax && gamma >= 0.0 && gamma <= 1.0 && eta >= 0.0 && eta <= dmax &&
                           sigma_b >= 0.0 && sigma_b <= dmax),
             "the adaptive clip needs d_clip, a finite clip, a quantile in [0, 1] and finite lr, count noise >= 0");
  FS_REQUIRE(d_c && d_r && d_state && d_sws, "null pointer");
  FS_REQUIRE(cols >= 1 && cols <= p->d.ld, "cols (the model's real columns) must be in [1, ld]");
  FS_REQUIRE(!p->d.chained, "DP-FedAvg needs parallel clients (a chained client's W_j - W_g holds its predecessors' work)");
  FS_REQUIRE(sws_bytes >= fs::aggregate_dp_ws_bytes(p->d.N, (int64_t)p->d.C * p->d.ld),
             "d_sws is too small (fs_aggregate_dp_ws_bytes(N, C * ld))");
  FS_REQUIRE(p->nova_mode == 0, "DP-FedAvg and a FedNova aggregate exclude each other (fs_plan_set_nova(0) first)");
  FS_REQUIRE(!p->scaffold, "DP-FedAvg and SCAFFOLD exclude each other (fs_plan_set_scaffold(0) first)");
  FS_REQUIRE(p->opt_rule == 0, "DP-FedAvg and a server optimizer exclude each other (fs_plan_set_server_opt(0) first)");
  FS_REQUIRE(!p->qffl, "DP-FedAvg and q-FedAvg exclude each other (fs_plan_set_qffl(0) first)");
  FS_REQUIRE(!p->robust, "DP-FedAvg and a robust aggregate exclude each other (fs_plan_set_robust(0) first)");
  FS_REQUIRE(!p->krum, "DP-FedAvg and Krum exclude each other (fs_plan_set_krum(0) first)");
  FS_REQUIRE(!p->rfa, "DP-FedAvg and RFA exclude each other (fs_plan_set_rfa(0) first)");
  FS_REQUIRE(!p->topk, "DP-FedAvg and FedTopK exclude each other (fs_plan_set_topk(0) first)");
  p->dp = 1;
  p->dp_S = S;
  p->dp_z = z;
  p->dp_seed = seed;
  p->dp_uniform = uniform ? 1 : 0;
  p->dp_adaptive = adaptive ? 1 : 0;
  p->dp_cols = cols;
  p->dp_gamma = gamma;
  p->dp_eta = eta;
  p->dp_sigma_b = sigma_b;
  p->dp_clip = adaptive ? d_clip : nullptr;
  p->dp_c = d_c;
  p->dp_r = d_r;
  p->dp_state = d_state;
  p->dp_ws = d_sws;
  p->dp_ws_bytes = sws_bytes;
  return FS_OK;
}

extern "C" int fs_plan_round(fs_plan* p, int t, float lr, int phases, const float* d_p_override, void* stream) {
  FS_REQUIRE(p && t >= 0, "bad arguments");
  return plan_round(p, t, lr, phases, d_p_override, nullptr, reinterpret_cast<hipStream_t>(stream));
}

// ABI 22: round t over the M sampled clients.  d_sel (ascending: the fold order), d_sel_order (the
// same ids in dispatch order) and d_q are read asynchronously by the launches enqueued here.
extern "C" int fs_plan_round_subset(fs_plan* p, int t, float lr, int phases, const int32_t* d_sel,
                                    const int32_t* d_sel_order, const float* d_q, int M, void* stream) {
  FS_REQUIRE(p && t >= 0 && d_sel && d_sel_order && d_q, "bad arguments");
  FS_REQUIRE(M >= 1 && M <= p->d.N, "M must be in [1, N]");
  if (int rc = subset_admits(p, "fs_plan_round_subset")) return rc;
  const Subset sub{d_sel, d_sel_order, d_q, M};
  return plan_round(p, t, lr, phases, nullptr, &sub, reinterpret_cast<hipStream_t>(stream));
}

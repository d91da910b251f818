/*
 * fedsim.h -- C-ABI of the MI355X (gfx950) federated-round engine.
 *
 * The reference (Bojian-Wei/Non-IID-Distributed-Learning-with-Optimal-Mixture-Weights)
 * is pure Python/PyTorch and has no native interface; every entry point below
 * replaces one Python-level piece of its hot path, cited as
 * /root/reference/<file>:<line>.  The Python drop-ins in
 * non-iid-distributed-learning-with-optimal-mixture-weights_amd/functions/tools.py
 * (FedAvg / FedProx / FedAMW) are the callers; INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Pointers named d_* are DEVICE pointers
 *     (hipMalloc / torch caching allocator); h_* are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     device entry points are asynchronous on that stream, allocate nothing and
 *     never synchronise (safe under hipGraph capture).  Kernels that exchange data
 *     between workgroups take a caller-owned workspace: the launch zeroes its
 *     exchange part itself; its LAST 256 bytes are an error block whose first
 *     uint32 is set (sticky) when a bounded cross-workgroup wait timed out -- the
 *     caller zeroes the workspace once at allocation, reads that word after the
 *     work and clears it.  Test knob: fs_tuning.inject_timeout = 1 makes every
 *     such launch report a timeout (the error path without a real hang).
 *   - Feature rows are fp32, row-major, with a leading dimension `ld` that is a
 *     multiple of 64 floats (D is zero-padded to ld; padded columns stay exactly 0).
 *   - Return value: 0 on success, negative on error; fs_last_error() returns a
 *     thread-local message.  No C++ exception crosses the ABI.
 */
#ifndef FEDSIM_H
#define FEDSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_OK 0
#define FS_EINVAL (-1)
#define FS_EHIP (-2)
#define FS_EUNSUPPORTED (-3)

#define FS_ABI_VERSION 23

/* ABI version and the last error message of the calling thread. */
int fs_abi_version(void);
const char* fs_last_error(void);

/* ------------------------------------------------------------------------- *
 * Tuning (ABI 9).  Every knob that changes HOW (never what) the kernels compute, as
 * explicit fields -- the library reads no environment variable.  All-zero = the defaults
 * (what the planners pick by shape); fs_tuning_size() is for binding-layout checks.
 * Threading contract (ABI 12): a launch reads the tuning in effect for the HOST THREAD
 * that enqueues it, at the moment it is enqueued (fs_local_train*, fs_plan_*, fs_mix_solve,
 * fs_randperm_device ...; a launch already enqueued is never affected).  That is the
 * thread's own override if fs_set_thread_tuning(t) set one, else the process-wide value of
 * fs_set_tuning (mutex-protected; visible to every thread without an override).
 * fs_set_tuning(NULL) restores the process-wide defaults; fs_set_thread_tuning(NULL)
 * drops the calling thread's override; fs_get_tuning reports what the calling thread's
 * next launch would use.  Two host threads that drive two plans with different solver or
 * form choices therefore each set a thread override.
 *   mix_solver         0 = by shape, else force one p-solver (FS_SOLVER_*; a forced solver
 *                      that does not cover the shape falls through to the shape's choice)
 *   mix_prefetch       L2 prefetch helper workgroups beside the p-solve: 0 = by solver
 *                      (4 for the quarter-wave solver when Z outgrows the L2s, 24 for qmc),
 *                      -1 = none, n > 0 = n
 *   mix_prefetch_lead  steps the helpers run ahead (0 = by solver: 16 quad; qmc 8 at K >= 12
 *                      workgroups, else 6)
 *   mix_exact_softmax  quarter-wave solvers: 1 = torch's exp(o - m - log sum) form with libm
 *                      expf / logf (default: e * rcp(sum e) on v_exp_f32 / v_rcp_f32; both
 *                      within the fp32 tolerance of the reference)
 *   no_eval_fuse       fs_plan_create: 1 = never carry a deferred evaluation inside a
 *                      training launch (fs_plan_eval_blocks() is then 0)
 *   spin_limit         bound of every cross-workgroup spin, in polls (0 = the default)
 *   inject_timeout     test knob: 1 = every exchanging launch reports a timeout at its first
 *                      hand-off (the error path without a real hang)
 *   train_form         (ABI 10) fs_local_train_plan's choice for parallel clients: 0 = by shape
 *                      (the pair form where it fits, else the split form), 1 = never the pair
 *                      form, 2 = the pair form wherever it fits (else as 0)
 *   split_early        (ABI 11) split form without a prox anchor on full slices: 0 = issue the
 *                      first SP_E1 (local_train_split.hip: 4 at G = 2, 6 at G >= 4) of each
 *                      wave's 16 next-step row loads right after the hand-off (they stream
 *                      through the softmax), -1 = all of them inside the backward; since
 *                      round 5 it covers the prox term (anchor slice first, 2 early rows) and
 *                      the narrow chained instances (one tile per wave at 4 or 8 tiles per
 *                      slice: every row load early); -1 turns both off (bitwise the same W)
 *   mix_qmc_lane_clients (ABI 13) qmc p-solver: clients per lane, 0 = by shape (4 where
 *                      K = ceil(N / 64) <= 16 workgroups, else 8 for C <= 10), 4 = force 4,
 *                      8 = force 8 where C <= 10 (K = ceil(N / 128)); same p to fp32 rounding
 *                      of the K-partial sums (a different client-to-workgroup split)
 *   mix_quad_loaders   (ABI 13) quad p-solver at 64 < N <= 128, C <= 10 (config 2): 0 = with
 *                      4 loader waves that stream the late classes' Z rows into LDS (default),
 *                      -1 = without (each compute wave issues all of its loads); bitwise the
 *                      same p
 *   split_teams        (ABI 13) fs_local_train_plan's choice of the team form for parallel
 *                      clients: 0 = by shape (not chosen: measured slower), 1 = wherever it
 *                      fits, -1 = never
 *   mix_poll_delay     (ABI 13) qmc p-solver: s_sleep(1) units (~64 cycles each) between a
 *                      step's publish and its first poll: 0 = by shape (10 at K >= 12 with
 *                      C >= 8, else 8), -1 = none, n > 0 = n; bitwise the same p
 *   split_poll_delay   (ABI 13) split form: s_sleep(1) units between a step's publish and its
 *                      first poll: 0 = by width (16 at G >= 8 with parallel clients, else
 *                      none), -1 = none, n > 0 = n; bitwise the same results
 *   split_pipe         (ABI 14) fs_local_train_plan's choice of the pipe form (FS_G_PIPE):
 *                      0 = by shape, 1 = wherever it fits (G = ld / 1024), -1 = never
 *   split_dbuf         (ABI 15) split form on full slices (8 waves x 2 tiles, or the narrow
 *                      chained 4 x 1) with 16 < B <= 32: the double-buffered instance
 *                      (local_train_dbuf.hip: the rows streamed ahead of the hand-off);
 *                      1 = wherever it covers; 0 = by shape (not chosen: measured a tie at
 *                      configs 2 and 5, slower at config 1); -1 = never; bitwise the same results
 *   split_mb           (ABI 16) split form with 16 < B <= 32: the classes on the 16-block
 *                      v_mfma_f32_4x4x1_16b_f32 in ceil(C / 4) blocks of 4 (the "mb" instances,
 *                      local_train_split.hip) instead of v_mfma_f32_16x16x4_f32 padded to 16;
 *                      0 = by shape, 1 = wherever it fits, -1 = never.  Same steps and hand-off,
 *                      the products summed in another order (within the oracle's fp32 tolerance)
 * ------------------------------------------------------------------------- */
#define FS_SOLVER_AUTO 0
#define FS_SOLVER_REG 1
#define FS_SOLVER_MC 2
#define FS_SOLVER_STAGED 3
#define FS_SOLVER_GLOBAL 4
#define FS_SOLVER_REG2 5
#define FS_SOLVER_WAVE 6
#define FS_SOLVER_QUAD 8
#define FS_SOLVER_QMC 9
#define FS_SOLVER_BIN 10

typedef struct fs_tuning {
  int mix_solver;
  int mix_prefetch;
  int mix_prefetch_lead;
  int mix_exact_softmax;
  int no_eval_fuse;
  unsigned spin_limit;
  int inject_timeout;
  int train_form;
  int split_early;
  int mix_qmc_lane_clients;
  int mix_quad_loaders;
  int split_teams;
  int mix_poll_delay;
  int split_poll_delay;
  int split_pipe;
  int split_dbuf;
  int split_mb;
} fs_tuning;

int64_t fs_tuning_size(void);
int fs_set_tuning(const fs_tuning* t);
int fs_set_thread_tuning(const fs_tuning* t);
int fs_get_tuning(fs_tuning* t);
/* (ABI 14) the process-wide value alone (what fs_set_tuning last set), whatever the calling
 * thread's override; and the calling thread's override: returns 1 and fills *t if one is
 * set, 0 (and *t = all-zero) if not.  A binding that changes one field for a block of code
 * reads the value it will restore from the layer it writes (the ADVICE round-4 fix: a
 * process-wide set from a thread with an override neither copies that override into the
 * process value nor is shadowed silently). */
int fs_get_process_tuning(fs_tuning* t);
int fs_get_thread_tuning(fs_tuning* t);

/* ------------------------------------------------------------------------- *
 * Host: DataLoader shuffle replay.
 * Replaces the RandomSampler permutation of every shuffled pass
 * (torch.utils.data.DataLoader(shuffle=True) at tools.py:179, 220; exp.py:99):
 * for pass i, out[off[i] .. off[i]+n[i]) = torch.randperm(n[i], generator=g)
 * with g.manual_seed(seed[i]) -- MT19937 seeded with (uint32)seed, forward
 * Fisher-Yates with z = mt() % (n-k).  Bit-exact with torch 2.10 CPU.
 * nthreads <= 0 picks the hardware concurrency.
 * ------------------------------------------------------------------------- */
int fs_randperm_batch(const int64_t* h_seeds, const int64_t* h_n, const int64_t* h_off,
                      int64_t npasses, int32_t* h_out, int nthreads);

/* ------------------------------------------------------------------------- *
 * Host: LIBSVM / svmlight reader.  Replaces the parse of svmlight_data
 * (utils.py:36-38, sklearn load_svmlight_file) for the dense float32 rows
 * load_full_data feeds the feature map (utils.py:56): `label [qid:q] idx:val ...`
 * per line, `#` comments, blank lines skipped; values parsed as doubles and rounded
 * once to float32 (= csr.toarray().astype(float32)).  fs_libsvm_scan reports the
 * sample count and the smallest / largest feature index (-1: no features).
 * fs_libsvm_read fills X [n_rows][n_features] (zeroed first) and y [n_rows];
 * zero_based: 1 indices start at 0, 0 at 1, -1 auto (zero-based iff the smallest
 * index is 0, as sklearn's 'auto'); an index outside n_features is an error.
 * Parallel over line-aligned chunks (nthreads <= 0: min(16, hardware)).
 * ------------------------------------------------------------------------- */
int fs_libsvm_scan(const char* path, int64_t* n_rows, int64_t* min_index, int64_t* max_index);
int fs_libsvm_read(const char* path, int64_t n_rows, int64_t n_features, int zero_based, float* X, double* y,
                   int nthreads);

/* ------------------------------------------------------------------------- *
 * Device: the same shuffle replay as fs_randperm_batch, on the GPU; d_seeds/d_n/d_off
 * are device arrays of npasses int64.  max_n MUST bound every n[i] (the host chooses the
 * form from it before the device sees n): max_n <= 64 runs one pass per LANE (64 passes per
 * wave, the MT state and the shuffle in registers / the lane's LDS row); larger max_n runs
 * one wave per pass with an LDS-resident (max_n <= ~38K) or in-place global-memory
 * permutation.  Bit-identical to fs_randperm_batch.  Asynchronous on `stream`.
 * (ABI 14) d_err (device, may be NULL): a pass with n[i] > max_n -- a caller breaking the
 * contract -- is written as the identity permutation (memory-safe: no LDS row or buffer is
 * overrun) and sets *d_err to 1 (sticky; the caller zeroes it once, reads it after the work
 * and raises -- Shuffler.check_errors in engine.py).
 * ------------------------------------------------------------------------- */
int fs_randperm_device(const int64_t* d_seeds, const int64_t* d_n, const int64_t* d_off, int64_t npasses,
                       int64_t max_n, int32_t* d_out, uint32_t* d_err, void* stream);

/* ------------------------------------------------------------------------- *
 * Local training of N clients.  Replaces train_loop (tools.py:177-215) called
 * once per client by FedAvg/FedProx/FedAMW (tools.py:340-343, 367-370, 430-433).
 *
 *   d_phi      [rows][ld]      client features, client j = rows d_row_off[j] .. d_row_off[j+1]-1
 *   d_row_off  [N+1]  int64    CSR row offsets
 *   d_labels   [rows] int32    class index per row
 *   d_perms    [E*rows] int32  client j, epoch e: local indices at E*row_off[j] + e*n_j
 *   d_order    [N] int32       block -> client schedule (parallel mode; NULL = identity)
 *   d_W_start  [C][ld]         round-start weights (client 0's start when chained)
 *   d_W_out    [N][C][ld]      each client's trained weights (the clients x params buffer)
 *   d_loss     [N] double      last-epoch |b|-weighted mean loss (incl. prox/ridge terms)
 *   B, E       batch size (>= 1; above 64: the wide form, G = 1 | FS_G_WIDE), local epochs.  The
 *              effective batch of client j is min(B, n_j).
 *   lr, mu, lam, prox, reg     SGD lr; prox weight (used iff prox); ridge weight (iff reg)
 *   chained    1: client j starts from client j-1's result and its prox anchor is
 *              that start (reference semantics);  0: every client starts
 *              from d_W_start (parallel clients).
 *   G, d_ws    workgroups per client and their workspace, from fs_local_train_plan:
 *              G = 1: one workgroup walks each client (any shape, chained or not);
 *              G = 2/4/8/16: "split clients" -- a group of G co-resident workgroups
 *              shares one client's feature tiles and exchanges partial logits every
 *              step (C <= 16, B <= 32).  Parallel clients: min(N, CUs/G) groups walk
 *              the clients (LPT order, snake over the groups); chained clients: one
 *              group walks the chain with the weights kept in registers.  The error
 *              word (last 256 bytes of d_ws) is nonzero after the kernel if a partner
 *              never arrived (results invalid).
 *              G | FS_G_PAIR (ABI 10, parallel clients, ld == 512 G): the "pair" form --
 *              min(ceil(N/2), CUs/G) groups of G workgroups, each training TWO clients at a
 *              time interleaved, so one client's hand-off overlaps the other's compute and
 *              the feature rows stream through every phase; the same arithmetic as the split
 *              form at width G (bitwise the same results).
 *              G | FS_G_TEAMS (ABI 13, parallel clients, G = 4 or 8): the "team" form --
 *              min(ceil(N/2), CUs/G) groups of G workgroups, each workgroup's 8 waves two
 *              teams of 4 that train two clients at once with team-local barriers, so one
 *              team's hand-off and softmax run beside the other team's MFMAs (the split
 *              arithmetic with 4 waves per slice: within the fp32 tolerance of the split form).
 *              G | FS_G_PIPE (ABI 14, ld == 1024 G with G = 2, 4, 8 or 16, 16 < B <= 32, C <= 16;
 *              parallel or chained clients, ridge and prox terms): the "pipe" form -- the split form with
 *              each step's hand-off pipelined by 16-row tile (one tile's partner round trip under
 *              the other tile's forward or backward MFMAs, the softmax per wave in registers, two
 *              barriers per step); the same arithmetic in the same order as the split form at
 *              width G (bitwise the same results).
 *              fs_local_train_plan: *G_out on entry is a request (0 = planner's choice, 1 =
 *              one workgroup per client, 2..16 = that split width if the shape allows it,
 *              G | FS_G_PAIR = the pair form, G | FS_G_TEAMS = the team form at that width
 *              if the shape allows it); prox says whether the FedProx term is on.
 *              1 | FS_G_WIDE (ABI 21, any B >= 1, C <= 32, parallel or chained clients): the
 *              "wide" form -- one workgroup per client with the batch walked in 64-row blocks:
 *              every block's forward on the step's unchanged weights, g = (softmax - onehot) /
 *              |b| over the whole batch, the gradient accumulated over all blocks and one
 *              fused update per batch.  min(N, 512) workgroups walk d_order (chained: one), each
 *              with a slot of d_ws for its batch's g: [ceil64(min(B, max_j n_j))][16 or 32]
 *              floats; the last 256 bytes stay the error block, which this form never writes.
 *              fs_local_train_plan answers 1 | FS_G_WIDE for B > 64, and for a request of
 *              1 | FS_G_WIDE at any B; its ws_bytes comes from max_en / E (the largest client)
 *              and the workgroups launched -- host arithmetic only, the same on every device.
 *              A client whose batch outgrows the slot (a workspace planned for other clients)
 *              is not trained: its start comes back with a NaN loss.
 * Requires 1 <= C <= 32, B >= 1 (B <= 64 without FS_G_WIDE), ld % 64 == 0, D <= ld.
 * ------------------------------------------------------------------------- */
#define FS_G_PAIR 256
#define FS_G_TEAMS 512
#define FS_G_PIPE 1024
#define FS_G_WIDE 2048
int fs_local_train_plan(int N, int C, int B, int E, int64_t ld, int64_t max_en, int chained, int prox,
                        int* G_out, int64_t* ws_bytes_out);
int fs_local_train(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int32_t* d_labels,
                   const int32_t* d_perms, const int32_t* d_order, int N, int C, int B, int E,
                   float lr, float mu, int prox, float lam, int reg, int chained,
                   const float* d_W_start, float* d_W_out, double* d_loss, int G, void* d_ws,
                   int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * (ABI 17) Local training under nn.MSELoss at ONE output column: train_loop with
 * type != 'classification' (tools.py:177-215, the criterion of tools.py:183-184) and
 * num_classes = 1 (utils.py:121, 167).  Arguments as fs_local_train without C, G and the
 * workspace:
 *   d_y        [rows] float    target per row (the [n, 1] targets of utils.py:81-82, flattened)
 *   d_W_start  [ld]            round-start weights;  d_W_out [N][ld]
 * Per batch b: o_i = phi_i . w;  L = (1/|b|) sum_i (o_i - y_i)^2 [+ mu ||w - w_a||] [+ lam ||w||];
 * dL/do_i = (2/|b|) (o_i - y_i);  w -= lr (sum_i dL/do_i phi_i + mu (w - w_a)/||w - w_a|| +
 * lam w/||w||) (tools.py:190-211; a zero norm contributes a zero gradient).  d_loss as
 * fs_local_train.  One workgroup per client (parallel clients: a grid of N in d_order) or one
 * workgroup walking the chain; w lives in registers; no cross-workgroup exchange, no spin, no
 * workspace.  Requires 1 <= B <= 64, ld % 64 == 0, ld <= 16384, E >= 0: anything else returns
 * FS_EUNSUPPORTED before launching.
 * ------------------------------------------------------------------------- */
int fs_local_train_mse(const float* d_phi, int64_t ld, const int64_t* d_row_off, const float* d_y,
                       const int32_t* d_perms, const int32_t* d_order, int N, int B, int E, float lr, float mu,
                       int prox, float lam, int reg, int chained, const float* d_W_start, float* d_W_out,
                       double* d_loss, void* stream);

/* ------------------------------------------------------------------------- *
 * Weighted aggregation: d_W_bar = p0*W0 + p1*W1 + ... + p_{N-1}*W_{N-1}, every
 * product and sum rounded separately in that left-to-right order
 * (tools.py:345-350, 372-377, 455-460).  W_j = d_W_all + j*stride, len floats.
 * chunks == 1 gives the reference's exact fold; chunks > 1 folds `chunks`
 * consecutive client ranges in parallel and then folds the partials in order
 * (needs d_ws of chunks*len floats).  chunks <= 0 picks a value from the shape.
 * ------------------------------------------------------------------------- */
int fs_aggregate(const float* d_W_all, int64_t stride, const float* d_p, int N, int64_t len,
                 float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks, void* stream);

/* ------------------------------------------------------------------------- *
 * (ABI 22) The gathered fold of a round with partial client participation:
 * d_W_bar = q_0*W[sel_0] + q_1*W[sel_1] + ... + q_{M-1}*W[sel_{M-1}] in k order, every product
 * and sum rounded separately (tools.py:345-350 over the sampled clients, ascending client id).
 * W[j] = d_W_all + j*stride, len floats; d_sel [M] int32 row indices (each a valid row of
 * d_W_all: the caller's contract, nothing on the device checks it), d_q [M] weights.
 * Contract: bitwise what fs_aggregate returns on the compacted copy W[sel] with the same
 * `chunks`, d_ws and ws_floats -- the same regimes chosen by M instead of N, so for M < 16 (or
 * chunks == 1) the reference's exact left fold.  Rows outside d_sel are never read: the traffic
 * is M*len floats plus the output, not N*len.  No atomics, no cross-workgroup wait.
 * ------------------------------------------------------------------------- */
int fs_aggregate_sel(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                     int64_t len, float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks, void* stream);

/* ------------------------------------------------------------------------- *
 * (ABI 23) FedNova's scaled fold (tools.py:383-410) over M rows of the clients x params buffer,
 * in k order, every operation rounded separately.  W[j] = d_W_all + j*stride, len floats; d_sel
 * [M] int32 row ids (valid rows: the caller's contract), or NULL for rows 0..M-1; d_q [M].
 *   mode FS_NOVA_REFERENCE  the reference's lines (tools.py:401-405), which scale the WEIGHTS:
 *       d_W_bar = fl(W[sel_0]*s0) + sum_{k>=1} fl( fl( fl(q_k*W[sel_k]) * te ) / d_b[k] )
 *     with the correctly rounded IEEE quotient.  Bitwise the reference's fold for
 *     s0 = f32(f64(p_0)*Tau_eff/Tau_0), te = f32(Tau_eff), d_b[k] = f32(Tau_k), q = p.  s0 belongs
 *     to the fold's first row only (not to a chunk's first row); d_b[0] is not read.  For unequal
 *     client sizes these coefficients sum to N * sum_j p_j^2 > 1, not to 1.
 *   mode FS_NOVA_UPDATES    normalised averaging of the UPDATES (Wang et al. 2020):
 *       d_W_bar = fl( base + sum_k fl( q_k * fl(W[sel_k] - base) ) ),  base = d_W_base [len].
 *     d_W_base may be d_W_bar itself: every position's base is read before that position is
 *     written, by the same workgroup.  d_b, te and s0 are not read.
 * The first term of any range is the term itself, not 0 + term.  Regimes are fs_aggregate's,
 * chosen by M with the same `chunks`, d_ws and ws_floats: for M < 16 or chunks == 1 the exact
 * left fold, else the same sub-ranges / chunks and stage-2 tree.  Mode 1 with te = 1, d_b == 1,
 * s0 = q_0 is bitwise fs_aggregate / fs_aggregate_sel.  Rows outside d_sel are never read.  No
 * atomics, no cross-workgroup wait, no allocation; asynchronous on `stream`.
 * FS_EINVAL for M < 1, len / stride not multiples of 4, a null pointer the mode needs, or a mode
 * other than 1 or 2.
 * ------------------------------------------------------------------------- */
#define FS_NOVA_REFERENCE 1
#define FS_NOVA_UPDATES   2
int fs_aggregate_nova(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                      const float* d_b, float te, float s0, int mode, const float* d_W_base, int M, int64_t len,
                      float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks, void* stream);

/* ------------------------------------------------------------------------- *
 * SCAFFOLD (Karimireddy et al., ICML 2020; option II).  Additive to ABI 23: three new entry
 * points, no new field in fs_tuning or fs_plan_desc, FS_ABI_VERSION unchanged.
 *
 * fs_local_train_scaffold: local training with control variates, parallel clients,
 * cross-entropy.  One 512-thread workgroup per client of d_order (NULL: clients 0..N-1); grid N.
 * Under a subset launch N is the sample size and d_order holds the ids; d_W_out [clients][C][ld],
 * d_ci [clients][C][ld] and d_loss [clients] stay indexed by client id and entries of clients
 * outside d_order are not touched.  Client i starts from y = d_W_start and takes fs_local_train's
 * K_i = E*ceil(n_i/B) steps (single form: same tiling, sums and ownership) with one more gradient
 * term: d = fl(c - c_i), fixed for the whole client, grad = fl(grad_CE + d), then the ridge term
 * (reg), then y -= lr*grad.  The reported loss is fs_local_train's (the correction is no part of
 * it).  After the last step, in place:
 *     c_i <- fl(fl(c_i - c) + fl(fl(x - y) * inv)),   inv = 1.0f / fl((float)K_i * lr)
 * with x = d_W_start, every operation rounded separately, and d_W_out[i] = y.  With c = c_i = 0
 * d_W_out and d_loss are bitwise fs_local_train's at G = 1.  A client without steps (E = 0)
 * returns x, loss 0 and an unchanged c_i.  d_c [C][ld] is only read; d_W_start must not alias
 * d_W_out.  There is no prox term and no chained, wide, split or MSE form.
 * Requirements: 1 <= C <= 32, 1 <= B, ld % 64 == 0, lr > 0, non-null pointers (d_order may be
 * NULL): FS_EINVAL otherwise, and FS_EUNSUPPORTED for B > 64 -- before any launch, outputs
 * untouched.
 *
 * fs_aggregate_scaffold: the server step, both folds from one pass over the M rows d_sel (NULL:
 * rows 0..M-1) of d_W_all, in place, with x = d_W_g on entry:
 *     d_W_g <- fl(x + sum_k fl(q_k * fl(W_k - x)))
 *     d_c   <- fl(fl(cs * c) + sum_k fl(r_k * fl(x - W_k)))
 * k ascending, every operation rounded separately.  With q_k = eta_g p_k / sum_S p,
 * r_k = p_k / (K_k lr) and cs = 1 - sum_S p_k (0 when S is every client) d_c stays
 * sum_j p_j c_j over ALL clients to rounding, since option II's c_i+ - c_i = -c + (x - W_i)/(K_i lr)
 * does not need the old c_i.  Regimes are fs_aggregate's, chosen by M and chunks: the exact left
 * fold for M < 16 or chunks == 1, else the same sub-ranges, chunks and stage-2 tree; the two-stage
 * form keeps two partials per chunk in d_ws, so its chunk clamp uses ws_floats / 2.  d_W_g is
 * bitwise what fs_aggregate_nova returns in mode FS_NOVA_UPDATES with base d_W_g, the same q and
 * chunks and a workspace of ws_floats / 2; d_c has the same fold structure over its own terms
 * (the first term of a range is the term itself, fl(cs * c) is added last).  A position's x and c
 * are read by the workgroup that writes them, before it writes.  (M + 2)*len floats read, 2*len
 * written.  FS_EINVAL for M < 1, len or stride no multiple of 4, a null pointer (d_sel and d_ws
 * may be NULL) or d_W_g == d_c; nothing is written then.
 * ------------------------------------------------------------------------- */
int fs_local_train_scaffold(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int32_t* d_labels,
                            const int32_t* d_perms, const int32_t* d_order, int N, int C, int B, int E,
                            float lr, float lam, int reg, const float* d_W_start, const float* d_c,
                            float* d_ci, float* d_W_out, double* d_loss, void* stream);
int fs_aggregate_scaffold(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                          const float* d_r, float cs, int M, int64_t len, float* d_W_g, float* d_c,
                          float* d_ws, int64_t ws_floats, int chunks, void* stream);

/* ------------------------------------------------------------------------- *
 * FedOpt server optimizers (Reddi et al., ICLR 2021, Algorithm 2: FedAdagrad / FedAdam / FedYogi;
 * server momentum FedAvgM, Hsu et al. 2019).  Additive to ABI 23: two new entry points, no new
 * field in fs_tuning or fs_plan_desc, FS_ABI_VERSION unchanged.
 *
 * fs_aggregate_opt: the fold of the updates of the M rows d_sel (NULL: rows 0..M-1) of d_W_all
 * with the optimizer step fused onto its end, d_W_g, d_m and d_v [len] updated in place.  With
 * x = d_W_g, m = d_m, v = d_v on entry, k ascending, every operation rounded separately:
 *     delta = sum_k fl(q_k * fl(W_k - x)),     d2 = fl(delta*delta)
 *   FS_OPT_AVGM     m' = fl(fl(beta1*m) + delta),   x' = fl(x + fl(eta*m'));  d_v is not read and
 *                   may be NULL
 *   the others      m' = fl(fl(beta1*m) + fl(omb1*delta))
 *   FS_OPT_ADAGRAD  v' = fl(v + d2)
 *   FS_OPT_ADAM     v' = fl(fl(beta2*v) + fl(omb2*d2))
 *   FS_OPT_YOGI     v' = fl(v - fl(fl(omb2*d2) * s)),  s = sgn(fl(v - d2)) in {-1, 0, +1}
 *                   x' = fl(x + fl(fl(eta*m') / fl(sqrtf(v') + tau)))
 * with the correctly rounded IEEE quotient and square root and no bias correction (as the paper).
 * omb1 and omb2 are the caller's f32(1 - beta), computed in float64: the host decides their
 * rounding once.  delta is folded exactly as fs_aggregate_nova folds mode FS_NOVA_UPDATES before
 * it adds its base -- the first term of a range is the term itself; regimes are fs_aggregate's,
 * chosen by M with the same `chunks`, d_ws and ws_floats (one partial per chunk): the exact left
 * fold for M < 16 or chunks == 1, else the same sub-ranges / chunks and stage-2 tree -- so
 * FS_OPT_AVGM with beta1 = 0, eta = 1 leaves in d_W_g bitwise what mode FS_NOVA_UPDATES returns
 * with base d_W_g.  The step runs once per element, in the thread that writes the position; a
 * position's x, m and v are read by the workgroup that writes them, before it writes.  Rows
 * outside d_sel are never read.  (M + 3)*len floats read and 3*len written (FS_OPT_AVGM: M + 2
 * and 2).  No atomics, no cross-workgroup wait, no allocation; asynchronous on `stream`.
 * FS_EINVAL for M < 1, len or stride no multiple of 4, stride < len, a rule outside 1..4, a null
 * pointer the rule needs (d_sel and d_ws may be NULL), tau <= 0 for rules 2..4 (a padding column
 * has delta = 0 and its step must be 0 / positive) or any two of d_W_g, d_m, d_v equal; nothing
 * is written then.
 * ------------------------------------------------------------------------- */
#define FS_OPT_AVGM    1
#define FS_OPT_ADAGRAD 2
#define FS_OPT_ADAM    3
#define FS_OPT_YOGI    4
int fs_aggregate_opt(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int rule,
                     float eta, float beta1, float omb1, float beta2, float omb2, float tau, int M, int64_t len,
                     float* d_W_g, float* d_m, float* d_v, float* d_ws, int64_t ws_floats, int chunks, void* stream);

/* ------------------------------------------------------------------------- *
 * q-FedAvg (q-FFL; Li, Sanjabi, Beirami, Smith, ICLR 2020).  Additive to ABI 23: four new entry
 * points, no new field in fs_tuning or fs_plan_desc, FS_ABI_VERSION unchanged.
 *
 * fs_aggregate_qffl: the q-FFL server step from ONE pass over the M rows d_sel (NULL: rows
 * 0..M-1) of d_W_all: the weighted fold of the updates and every update's squared norm from the
 * same loads.  With x = d_W_g on entry, k ascending, every float operation rounded separately:
 *     d_S    = sum_k fl(u_k * fl(W_k - x))           folded exactly as fs_aggregate_opt folds its
 *              delta (the regimes of fs_aggregate at M rows, the same `chunks`, d_ws, ws_floats;
 *              the first term of a range is the term itself): bitwise the d_m that
 *              FS_OPT_AVGM with beta1 = 0 leaves with q = u
 *     d_n[k] = sum_i fl(W_k[i] - x[i])^2             the same differences, from the same load; in
 *              float only inside one wave's share of a row (the square, the thread's 4 elements,
 *              at most 6 levels across the wave: at most 10 roundings), in double in a fixed order
 *              above that: within 16 * 2^-24 relative of the exact sum of the float differences'
 *              squares whatever len, and the same bits on every call
 *     U = sum_k (double)u_k,  G = sum_k (double)g_k * d_n[k],  H = Lc * U + G     (double, IEEE)
 *     coef   = (float)(Lc / H);  0 when H is not finite or <= 0, and d_W_g is then left as it is
 *     d_W_g  = fl(x + fl(coef * d_S));               d_hc = {H, (double)coef}
 * (M + 1)*len floats read by the pass; the two small launches after it touch len- and M-sized data
 * and the partial table only.  d_nws: fs_aggregate_qffl_ws_doubles(M, len) doubles of workspace
 * (the table of the waves' float shares; it holds nothing between calls).  Rows outside d_sel are
 * never read.  No atomics, no cross-workgroup wait, no allocation, no host synchronisation;
 * asynchronous on `stream`.
 * FS_EINVAL for M < 1, len or stride no multiple of 4, stride < len, a null pointer (d_sel and
 * d_ws may be NULL), Lc <= 0 or not finite, nws_doubles too small or d_S == d_W_g; nothing is
 * written then.
 *
 * fs_qffl_coef: the coefficients of a round from the losses fs_eval_clients left on the device
 * (d_F2 [N][2], the loss at [k][0]), one small launch: with Ft = d_F2[2 * row_k] + 1e-10,
 * row_k = d_sel[k] (NULL: k), in double and rounded once to float
 *     d_u[k] = d_p[k] * Ft^q            d_g[k] = d_p[k] * q * Ft^(q-1) * L^2
 * and q = 0 gives d_u = d_p, d_g = 0 exactly.  FS_EINVAL for q < 0, L <= 0, M < 1 or a null
 * pointer (d_sel may be NULL).
 * ------------------------------------------------------------------------- */
int64_t fs_aggregate_qffl_ws_doubles(int M, int64_t len);
int fs_aggregate_qffl(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_u, const float* d_g,
                      double Lc, int M, int64_t len, float* d_W_g, float* d_S, double* d_n, double* d_hc, float* d_ws,
                      int64_t ws_floats, int chunks, double* d_nws, int64_t nws_doubles, void* stream);
int fs_qffl_coef(const double* d_F2, const int32_t* d_sel, const float* d_p, double q, double L, int M, float* d_u,
                 float* d_g, void* stream);

/* ------------------------------------------------------------------------- *
 * Robust aggregation: the coordinate-wise beta-trimmed mean and median (Yin, Chen, Ramchandran,
 * Bartlett, ICML 2018).  Additive to ABI 23: three new entry points, FS_ABI_VERSION unchanged.
 *
 * fs_aggregate_robust: over the M rows d_sel (NULL: rows 0..M-1) of d_W_all, each of len floats,
 * with the trim count b, 0 <= 2b < M, for every coordinate i on its own:
 *   Order.  The M values are ordered by the monotone 32-bit key of a float's bits,
 *     key = bits ^ 0xFFFFFFFF when the sign bit is set, bits | 0x80000000 otherwise:
 *     a total order with -0 < +0, +Inf and sign-clear NaNs at the top, -Inf and sign-set NaNs at
 *     the bottom.
 *   Kept.   The ranks b+1 .. M-b of that order (n = M - 2b values, a multiset).  Values that tie
 *     at a threshold have equal keys, hence equal bits: which of them are kept cannot matter.
 *   Output. d_out[i] = (float)(S / (double)n), S the sum of the kept values as doubles.
 *   b = 0 is the uniform mean, b = (M-1)/2 the median (odd M: the middle value itself, even M:
 *   the mean of the two middle values).  Up to b rows of arbitrary bits per side are discarded
 *   per coordinate (Inf and NaN included); a NaN that survives the trim makes that coordinate
 *   NaN (with whatever payload: callers compare NaN as NaN).
 *   Summation order of S (IEEE double, no fused multiply-add), with lo and hi the values at ranks
 *   b+1 and M-b, clo and chi the number of kept copies of each (lo == hi as keys: clo = n,
 *   chi = 0), T = 256 / width slices and width = 32 columns for M <= 1261, 16 for M <= 2523,
 *   8 above:
 *     n <= 2:  S = clo * lo, then + chi * hi when chi > 0;
 *     else     slice s (0 <= s < T) = 0.0 + the values strictly between lo and hi (by key) at
 *              k = s, s + T, s + 2T, ... in ascending k (k the position in d_sel);
 *              the slices joined by the pairwise tree p[j] += p[j + h] for j = 0, 2h, 4h, ...,
 *              h = 1, 2, 4, ... < T;   S = (tree + clo * lo), then + chi * hi when chi > 0.
 *   tests/robust_restatement.py restates this in numpy; the kernel equals it bit for bit, and it
 *   is within 2^-24 |ref| + n 2^-52 mean|kept| + 2^-149 of the sorted float64 mean ref.
 * Every selected row element is loaded once, rows outside d_sel are never read, d_W_all is the
 * only input: d_out may be any buffer that is not part of the selected rows (the global model).
 * One launch; no global atomics, no cross-workgroup wait, no allocation, no host synchronisation;
 * the same bits on every call and for the same rows gathered from a larger buffer.
 * FS_EINVAL for M < 1, M > fs_aggregate_robust_max_m(), 2b >= M or b < 0, len or stride no
 * multiple of 4, stride < len or a null pointer (d_sel may be NULL); nothing is launched then.
 * fs_aggregate_robust_max_m: the largest M the kernel accepts (5047: the M rows of a stripe of 8
 * columns in one CU's LDS).
 * ------------------------------------------------------------------------- */
int fs_aggregate_robust(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len, int b,
                        float* d_out, void* stream);
int fs_aggregate_robust_max_m(void);

/* ------------------------------------------------------------------------- *
 * Krum and Multi-Krum (Blanchard, El Mhamdi, Guerraoui, Stainer, NeurIPS 2017): robust aggregation
 * by the pairwise distances of the rows.  Additive to ABI 23: the entry points below,
 * FS_ABI_VERSION unchanged.
 *
 * The rule, over the round's M rows W_k (k the position in d_sel, NULL: rows 0..M-1) of d_W_all,
 * each of len floats, the round-start model x = d_x [len], a Byzantine bound f and a pick count m:
 *   Centring.  U_k = fl(W_k - x), elementwise in float as fs_aggregate_qffl forms it.
 *   Distances. G_ab = U_a . U_b;  D_ab = max(0, fl(fl(G_aa + G_bb) - 2 G_ab)) for a != b, D_aa = 0;
 *     a D_ab that comes out NaN or +-Inf (NaN or Inf rows, overflow) is stored as +Inf.  One
 *     triangle is computed and mirrored: D_ab == D_ba bitwise.
 *   Score.    s_a = the sum, in double, of the n = M - f - 2 smallest of {D_ab : b != a}; a itself is
 *     left out by index, not by value.  Values that tie at the threshold are equal floats: which
 *     copies are kept cannot matter.
 *   Pick.     The m rows with the smallest (s_a, a), lexicographic (a score's bits order it: it is
 *     >= 0).  m = 1 is Krum, m = M - f the one-shot Multi-Krum.  d_pick [m] holds their row ids of
 *     d_W_all (d_sel[a], not a), in ascending position a -- ascending id when d_sel ascends.
 *   Output.   d_out = bitwise what fs_aggregate_sel(d_W_all, d_pick, q == f32(1 / m), m, ...) returns
 *     with the same chunks, d_agg_ws and agg_ws_floats; for m = 1 the picked row's bits.
 *   With at most f bad rows of arbitrary bits every good row has M - 1 - f >= n finite distances,
 *   hence a finite score; a row holding NaN or Inf scores +Inf and is never picked while m rows
 *   with finite scores exist.
 *
 * fs_krum_distances: D [M][ldD], ldD = (M + 3) & ~3 (the padding columns are not written), from
 * the gathered rows and x.  Summation order of G_ab (float, v_mfma_f32_32x32x2_f32, no other
 * precision): the len axis is cut into S slices of kc * 32 consecutive elements (S, kc from
 * fs_krum_split: a function of M and len only; the last slice may be shorter, and is padded with
 * exact zeros to a multiple of 32).  Inside a slice one accumulator starts at 0 and takes, K-step
 * by K-step of 32 elements in ascending order, 16 instructions (kq = 0..3 outer, j = 0..3 inner),
 * each adding the two products at the K-step's offsets 8 kq + j and 8 kq + 4 + j; then
 * G_ab = ((p_0 + p_1) + p_2) + ... over the slices' partials in ascending order.  A product
 * therefore passes through at most  min(len, 32 kc) + (S - 1)  additions on its way into G_ab and
 * two more into D_ab:  n_chain = min(len, 32 kc) + S + 1 <= len + 2,  and with
 * g = n_chain 2^-24 / (1 - n_chain 2^-24)
 *     | D_ab - ||U_a - U_b||^2 |  <=  2 g (||U_a||^2 + ||U_b||^2) + 2^-24 ||U_a - U_b||^2
 * (a-priori; tests/test_gpu_krum_kernels.py holds the kernel to it).  Two launches: the partial
 * Gram tiles into d_ws (fs_krum_distances_ws_bytes(M, len) bytes; enough for every M' <= M too),
 * then their fixed-order reduction and D.  No centred copy of the rows is written; rows outside
 * d_sel are never read.
 *
 * fs_krum_select: d_score [M] (double) and d_pick [m] from D [M][ldD] alone (d_sel, NULL: the
 * identity, only maps positions to ids; d_q, may be NULL: [m] floats set to f32(1 / m); d_rank: M
 * ints of scratch, left holding every row's rank under (score, position)).  The n-th
 * smallest t of row a's D_ab, b != a, by a radix select over the raw bits (D >= 0 or +Inf: the
 * bits are ordered); c = n - #{b != a : D_ab < t} copies of it are kept.  Summation order of s_a
 * (IEEE double): slice s (0 <= s < 256) = 0.0 + the D_ab < t, b != a, at b = s, s + 256, ... in
 * ascending b; the slices joined by the pairwise tree p[j] += p[j + h] for j = 0, 2h, 4h, ...,
 * h = 1, 2, 4, ... < 256;  s_a = tree + (double)c * (double)t.  tests/krum_restatement.py restates
 * it in numpy; the kernels equal it bit for bit.  Three launches (scores; ranks; pick).
 *
 * fs_aggregate_krum: the two stages and the gathered fold on `stream`, six or seven launches.
 * d_ws: fs_aggregate_krum_ws_bytes(M, len) bytes (enough for every M' <= M too); D stands at its
 * start ([M][ldD] floats) once the call has run.  d_agg_ws / agg_ws_floats / chunks are
 * fs_aggregate_sel's.  d_x may be d_out: it is read by the first launch only.  No global atomics,
 * no cross-workgroup wait, no allocation, no host synchronisation; the same bits on every call
 * and for the same rows gathered from a larger buffer.
 * FS_EINVAL, with nothing launched, for M < 3, f < 0, M - f - 2 < 1, m < 1 or m > M - f,
 * M > fs_aggregate_krum_max_m(), len or stride no multiple of 4, stride < len, a workspace that
 * is too small or a null pointer (d_sel, d_agg_ws and fs_krum_select's d_q may be NULL).
 * fs_aggregate_krum_max_m: 5120 (>= fs_aggregate_robust_max_m(): a row of D in one CU's LDS).
 * ------------------------------------------------------------------------- */
int fs_aggregate_krum_max_m(void);
int fs_krum_split(int M, int64_t len, int* splits, int* ksteps);
int64_t fs_krum_distances_ws_bytes(int M, int64_t len);
int64_t fs_aggregate_krum_ws_bytes(int M, int64_t len);
int fs_krum_distances(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                      const float* d_x, float* d_D, void* d_ws, int64_t ws_bytes, void* stream);
int fs_krum_select(const float* d_D, int M, int f, int m, const int32_t* d_sel, double* d_score, int32_t* d_pick,
                   float* d_q, int32_t* d_rank, void* stream);
int fs_aggregate_krum(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                      const float* d_x, int f, int m, float* d_out, int32_t* d_pick, double* d_score, void* d_ws,
                      int64_t ws_bytes, float* d_agg_ws, int64_t agg_ws_floats, int chunks, void* stream);

/* ------------------------------------------------------------------------- *
 * RFA (Pillutla, Kakade, Harchaoui, IEEE TSP 2022): the geometric median of the rows by T
 * smoothed Weiszfeld iterations.  Additive to ABI 23: the entry points below, FS_ABI_VERSION
 * unchanged.
 *
 * The rule, over the round's M rows W_k (k the position in d_sel, NULL: rows 0..M-1) of d_W_all,
 * each of len floats, the round-start model x = d_x [len], weights alpha_k >= 0 (d_alpha [M]
 * floats), a smoothing nu > 0, an iteration count 0 <= T <= FS_RFA_MAX_ITERS fixed by the caller and
 * init = FS_RFA_INIT_START (v0 = x) or FS_RFA_INIT_MEAN.  W = fs_rfa_width(M) (32, 16 or 8: a
 * function of M only) cuts the len axis into stripes of W consecutive columns, the last one
 * possibly shorter; all arithmetic is IEEE, nothing is contracted.
 *   Distance.  d_k(v) = sqrt(d2_k), d2_k = sum_i (double)e_i * (double)e_i with e_i = fl(W_k[i] - v[i])
 *     in float, as fs_aggregate_qffl forms it.  Order: a stripe's partial = 0.0 + its terms in
 *     ascending i; slice s (0 <= s < 32) = 0.0 + the partials of the stripes s, s + 32, ... in
 *     ascending order; the slices joined by the pairwise tree p[j] += p[j + h] for j = 0, 2h, 4h,
 *     ..., h = 1, 2, 4, ... < 32.  The sum cannot overflow in double; d_k is NaN or +Inf exactly
 *     when the row holds NaN or Inf or a float difference overflows.  Such a row is "not finite".
 *   Weights.   beta_k = (double)alpha_k / max(nu, d_k) when d_k is finite, else 0 (the weighted-mean
 *     step of INIT_MEAN: beta_k = (double)alpha_k when d_k is finite, else 0).  B = sum_k beta_k:
 *     slice s (0 <= s < 256) = 0.0 + beta_k at k = s, s + 256, ... ascending, the 256 slices joined by
 *     the same tree (h < 256).  b_k = (float)(beta_k / B); every b_k = 0 when B is 0 or not finite
 *     ("no finite row").  Stateless: a row is judged again at every iteration.
 *   Fold.      v'[i] = (float)(sum_{k : b_k != 0} (double)b_k * (double)W_k[i]) (the products are
 *     exact).  Order: slice s (0 <= s < 256 / W) = 0.0 + the terms at k = s, s + 256 / W, ... ascending,
 *     the slices joined by the same tree (h < 256 / W).  A row with b_k == 0 is skipped by index,
 *     never multiplied (0 * NaN).  After "no finite row" v' = v bit for bit.
 *   Objective. g(v) = sum_{k finite} (double)alpha_k * h(d_k), h(d) = d for d > nu, else
 *     d * d / (2.0 * nu) + nu / 2.0, in B's order; NaN when no row is finite.
 *   Chain.     Pass 0 takes the distances to x and folds nothing.  INIT_MEAN: one fused step with
 *     the weighted-mean weights over the rows pass 0 found finite gives v0.  Then T fused steps,
 *     each with the weights from the distances to the iterate before it.  d_out = v_T (T = 0: x, or
 *     v0).  d_dist [M] (double): the distances to d_out.  d_b [M]: the weights of the last fold (no
 *     fold at all, T = 0 from INIT_START: the weights pass 0 gave).  d_obj [T + 2] (double): g at
 *     x, at v0 (INIT_MEAN only), at v_1 .. v_T, in this order; the slots the chain does not reach
 *     hold NaN.
 *
 * fs_rfa_step: one iteration from one read of the rows.  d_b == NULL (then d_flag == NULL): pass 0,
 * d_v_out = d_v and the distances to it.  Else d_v_out = the fold with d_b (d_flag[0] != 0: d_v
 * instead), and the distances to d_v_out.  d_part [stripes][M] doubles takes the stripes' partials
 * (stripes = ceil(len / W)).  d_v_out may be d_v.
 * fs_rfa_weights: d_part reduced into d_d2 [M] (d_part == NULL: d_d2 as given), then d_dist, d_b,
 * d_obj[0] and d_flag[0] (1: no finite row) as above; mean = 1 for the weighted-mean weights.  Two
 * launches (the reduction over the stripes: 8 rows to a workgroup; the weights: one workgroup).
 * fs_aggregate_rfa: the chain on `stream`, 3 (T + 1) launches, 3 (T + 2) with INIT_MEAN (a step, the
 * reduction and the weights per stage).  d_ws: fs_aggregate_rfa_ws_bytes(M, len) bytes (enough for
 * every M' <= M too): the partial table, d2, two iterates, the flag.  d_out may be d_x: x is read
 * by pass 0 only, which copies it.  No global atomics, no cross-workgroup wait, no allocation, no
 * host synchronisation; the same bits on every call and for the same rows gathered from a larger
 * buffer.  tests/rfa_restatement.py restates the rule in numpy; the kernels equal it bit for bit.
 * FS_EINVAL, with nothing launched, for M < 1, M > fs_aggregate_rfa_max_m(), T outside [0, 32],
 * nu <= 0 or not finite, an unknown init, len or stride no multiple of 4, stride < len, a workspace
 * that is too small or a null pointer (d_sel may be NULL).
 * fs_aggregate_rfa_max_m: 5047 (= fs_aggregate_robust_max_m(): 8 columns of every row in one CU's
 * LDS); W = 32 up to M = 1261, 16 up to 2523.
 * ------------------------------------------------------------------------- */
#define FS_RFA_INIT_START 0
#define FS_RFA_INIT_MEAN 1
#define FS_RFA_MAX_ITERS 32
int fs_aggregate_rfa_max_m(void);
int fs_rfa_width(int M);
int64_t fs_aggregate_rfa_ws_bytes(int M, int64_t len);
int fs_rfa_step(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len, const float* d_v,
                const float* d_b, const int32_t* d_flag, float* d_v_out, double* d_part, void* stream);
int fs_rfa_weights(const double* d_part, int M, int64_t len, const float* d_alpha, double nu, int mean, double* d_d2,
                   double* d_dist, float* d_b, double* d_obj, int32_t* d_flag, void* stream);
int fs_aggregate_rfa(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                     const float* d_x, const float* d_alpha, int T, double nu, int init, float* d_out, double* d_dist,
                     float* d_b, double* d_obj, void* d_ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * FedTopK: top-k sparsified uploads with error feedback (Aji & Heafield, EMNLP 2017; Stich,
 * Cordonnier & Jaggi, NeurIPS 2018; Sattler et al. 2019).  Additive to ABI 23: the entry points
 * below, FS_ABI_VERSION unchanged.
 *
 * The rule, over the round's M rows W_k (k the position in d_sel, NULL: rows 0..M-1) of d_W_all,
 * each of len floats, x = d_W_g [len] on entry, the residual rows e_k of d_e ([clients][stride]
 * floats, indexed by client id as d_W_all; NULL: no memory), the weights q_k (d_q [M]) and a count
 * 1 <= kcount <= len; all arithmetic is IEEE, every operation rounded separately, nothing contracted.
 *   Update.    a_k[i] = fl(fl(W_k[i] - x[i]) + e_k[i]); without memory a_k[i] = fl(W_k[i] - x[i]).
 *   Threshold. key(v) = bits(v) & 0x7fffffff as uint32: magnitude order, the sign ignored, Inf above
 *     every finite value and NaN above Inf.  tau_k = the kcount-th largest of the row's len keys.
 *     Position i is kept iff key(a_k[i]) >= tau_k: ties at the threshold are all kept, so the kept
 *     count n_k >= kcount, and an all-zero row keeps everything.  Integer selection: exact,
 *     order-independent, the same bits on every run.  A NaN or an Inf is therefore always
 *     transmitted: the rule carries no robustness claim.
 *   Residual.  e_k[i] <- kept ? +0.0f : a_k[i], in place.  Rows of clients outside d_sel are neither
 *     read nor written; without memory nothing is stored.
 *   Fold.      s_k[i] = kept ? a_k[i] : +0.0f, d_W_g[i] <- fl(x[i] + sum_k fl(q_k * s_k[i])), k
 *     ascending, folded exactly as fs_aggregate_nova folds FS_NOVA_UPDATES before it adds its base:
 *     the first term of a range the term itself; regimes, sub-ranges, chunks and the stage-2 tree
 *     fs_aggregate's, chosen by M and `chunks`, d_ws / ws_floats one partial per chunk.
 *   Outputs.   d_tau[k]: a float whose bits are the key tau_k.  d_kept[k] = n_k (int32).
 * Dense identity: with kcount == len -- or any kcount at which every nonzero is kept -- and e == 0
 * on entry, d_W_g is bitwise what fs_aggregate_opt(FS_OPT_AVGM, beta1 = 0, eta = 1) leaves with the
 * same q, chunks and workspace, and e stays all +0 -- for rows without negative-zero differences
 * (fl(W_k[i] - x[i]) = -0 becomes +0 when e_k[i] = +0 is added; the identity needs a memory-free call,
 * d_e == NULL, to hold there as well).
 *
 * fs_topk_threshold: stage A, one workgroup per row.  With memory it LEAVES a_k IN e_k (the residual
 * is completed by the fold) and writes d_tau and d_kept; without, d_tau and d_kept only.  Reads
 * 2 M len floats (W_k, e_k; x from cache) and writes M len, then reads a_k back three times (a row
 * just written: cache hits); without memory 4 reads of W_k.  A radix select on the keys, most
 * significant digit first (8, 8, 8, 7 bits), the counts in LDS integer atomics.  d_ws / ws_bytes:
 * fs_aggregate_topk_ws_bytes(M, len) bytes, which is 0 (d_ws may be NULL).
 * fs_aggregate_topk: stage A, then the thresholded fold (1 or 2 launches, as fs_aggregate_nova),
 * which reads M len floats (a_k from d_e; without memory W_k, and x per sub-range), stores zeros
 * over the float4s of e_k that hold a kept position, and writes len floats of d_W_g.  d_sws /
 * sws_bytes as d_ws / ws_bytes above.  d_W_g is updated in place.
 * No float atomics, no global atomics, no cross-workgroup wait, no allocation, no host
 * synchronisation; the same bits on every call and for the same rows gathered from a larger buffer.
 * tests/topk_restatement.py restates the rule in numpy; the kernels equal it bit for bit.
 * FS_EINVAL, and nothing is written then, for M < 1, kcount < 1 or kcount > len, len or stride no
 * multiple of 4, stride < len, len >= 2^31, a null pointer (d_sel, d_e, d_ws and d_sws may be NULL),
 * a workspace that is too small, or d_e equal to d_W_all or d_W_g.
 * ------------------------------------------------------------------------- */
int64_t fs_aggregate_topk_ws_bytes(int M, int64_t len);
int fs_topk_threshold(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                      const float* d_W_g, float* d_e, int64_t kcount, float* d_tau, int32_t* d_kept, void* d_ws,
                      int64_t ws_bytes, void* stream);
int fs_aggregate_topk(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                      int64_t len, int64_t kcount, float* d_W_g, float* d_e, float* d_tau, int32_t* d_kept,
                      float* d_ws, int64_t ws_floats, int chunks, void* d_sws, int64_t sws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * DP-FedAvg: per-client norm clipping and Gaussian noise on the aggregate (McMahan, Ramage, Talwar
 * & Zhang, ICLR 2018; Geyer, Klein & Nabi 2017; adaptive clip: Andrew, Thakkar, McMahan & Ramaswamy,
 * NeurIPS 2021).  Additive to ABI 23: the entry points below, FS_ABI_VERSION unchanged.
 *
 * The rule, over the round's M rows W_k (k the position in d_sel, NULL: rows 0..M-1) of d_W_all,
 * each of len floats, x = d_W_g [len] on entry, the weights q_k (d_q [M]; NULL: every q_k =
 * (float)(1.0 / M)), the clip S > 0 (+Inf: none), the noise multiplier z >= 0, the seed and the
 * round t >= 0; all arithmetic is IEEE, every operation rounded separately, nothing contracted.
 *   Norms.  d_k = fl(W_k - x);  n_k = sum_i d_k[i]^2, float squares summed in a fixed,
 *     timing-independent order (float inside a wavefront's share of a row, at most 10 float
 *     roundings on a square's path, double above it): within 10 x 2^-24 relative of the exact sum.
 *   Coefficients (double).  r_k = sqrt(n_k);  s_k = 1 if r_k <= S, else S / r_k;
 *     c_k = (float)(q_k * s_k), rounded once.  A row whose n_k is NaN or +Inf -- it holds a NaN, an
 *     Inf, or squares that overflow float -- is DROPPED: c_k = 0, and it counts in `dropped`.
 *   Fold.  Delta = sum_k (c_k == 0 ? +0 : fl(c_k * d_k)), a select (0 * NaN would poison the sum),
 *     k ascending, folded exactly as fs_aggregate_opt folds its delta: the first term of a range the
 *     term itself; regimes, sub-ranges, chunks and the stage-2 tree fs_aggregate's, chosen by M and
 *     `chunks`, d_ws / ws_floats one partial per chunk.
 *   Noise.  sigma = (z * S) * max_k q_k in double (max over all M rows; uniform q: z S / M, the
 *     fixed-denominator estimator); z == 0: sigma = 0 and no noise term is formed.  Else
 *     d_W_g[i] <- fl(fl(x[i] + Delta[i]) + fl((float)sigma * g[i])); z == 0: fl(x[i] + Delta[i]).
 *   The field g depends on (seed, t, stream, i) alone, not on the launch geometry: the float4
 *     position j = i / 4 takes the outputs w0..w3 of Philox4x32-10 at counter (j, t, stream, 0) and key
 *     (seed mod 2^32, seed >> 32); u_m = (w_m + 0.5) * 2^-32; (g[4j], g[4j+1]) = sqrt(-2 ln u_0) *
 *     (cos, sin)(2 pi u_1) and (g[4j+2], g[4j+3]) likewise from u_2, u_3, evaluated in double, each
 *     rounded once to float; |g| <= sqrt(66 ln 2) < 6.77.  The model noise is stream 0.  cols_ld != 0:
 *     the len floats are rows of cols_ld floats (a multiple of 4 that divides len) of which the first
 *     cols_d are parameters; the others (a model's zero padding) take no noise term.  This is a
 *     simulator's noise (floating-point Gaussian samples, a truncated tail), not a deployed
 *     mechanism's, and no privacy accountant is provided.
 *   Adaptive clip (adaptive != 0): the clip of the round is read from d_clip[0] on the device (S is
 *     then only checked) and, after every c_k has been formed from it, d_clip[0] <- S_next =
 *     S * exp(-eta * ((b + sigma_b * g_b) / M - gamma)) in double, b = #{k not dropped : r_k <= S} and
 *     g_b the first normal of the block at counter (0, t, 1, 0) (stream 1).  Else S_next = S.
 *   State.  d_state [FS_DP_STATE] doubles: {S used, sigma, b, dropped, S_next}; d_r[k] = r_k (NaN or
 *     +Inf for a dropped row); d_c[k] = c_k.
 * fs_dp_norms: the norm pass alone, n_k into d_n [M] doubles; reads the M rows once, coalesced.
 * fs_dp_coef: the coefficient kernel alone from d_n (one workgroup): d_c, d_r, d_state, d_clip.
 * fs_dp_noise: writes g [len] for (seed, t, stream).
 * fs_aggregate_dp: the three stages (4 to 5 launches): reads the rows twice, writes len floats of
 * d_W_g in place.  d_sws of sws_bytes >= fs_aggregate_dp_ws_bytes(M, len) bytes holds the norms and
 * their partial table.  No atomics, no cross-workgroup wait, no allocation, no host
 * synchronisation; the same bits on every call and for the same rows gathered from a larger buffer.
 * With S = +Inf, z = 0 and every q_k > 0, d_W_g is bitwise what fs_aggregate_opt(FS_OPT_AVGM,
 * beta1 = 0, eta = 1) leaves with the same q, chunks and workspace.  tests/dp_restatement.py restates
 * the rule in numpy.
 * FS_EINVAL, and nothing is written then, for M < 1, S <= 0 or NaN, z < 0 or not finite, z > 0 with
 * S = +Inf, t < 0, len or stride no multiple of 4, stride < len, a null pointer (d_sel and d_q may be
 * NULL; d_clip unless adaptive), a workspace that is too small, or adaptive with S = +Inf, gamma
 * outside [0, 1], or eta or sigma_b negative or not finite.
 * ------------------------------------------------------------------------- */
#define FS_DP_STATE 5
int64_t fs_aggregate_dp_ws_bytes(int M, int64_t len);
int fs_dp_norms(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len, const float* d_W_g,
                double* d_n, void* d_sws, int64_t sws_bytes, void* stream);
int fs_dp_coef(const double* d_n, const float* d_q, int M, double S, double z, uint64_t seed, int t, int adaptive,
               double gamma, double eta, double sigma_b, double* d_clip, float* d_c, double* d_r, double* d_state,
               void* stream);
int fs_dp_noise(uint64_t seed, int t, int noise_stream, int64_t len, float* d_g, void* stream);
int fs_aggregate_dp(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M, int64_t len,
                    double S, double z, uint64_t seed, int t, int adaptive, double gamma, double eta, double sigma_b,
                    double* d_clip, int64_t cols_ld, int64_t cols_d, float* d_W_g, float* d_c, double* d_r,
                    double* d_state, float* d_ws, int64_t ws_floats, int chunks, void* d_sws, int64_t sws_bytes,
                    void* stream);

/* ------------------------------------------------------------------------- *
 * Test evaluation. Replaces test_loop + comp_accuracy + Meter (tools.py:218-237,
 * 82-96, 99-148): d_out[0] = mean cross-entropy over n rows, d_out[1] = top-1
 * accuracy in percent.  Ties in the arg-max go to the lowest class index.
 * d_ws needs fs_eval_ws_doubles(n) doubles.
 * ------------------------------------------------------------------------- */
int64_t fs_eval_ws_doubles(int n);
int fs_eval(const float* d_phi, int64_t ld, const int32_t* d_labels, int n, const float* d_W, int C,
            double* d_out, double* d_ws, void* stream);

/* ------------------------------------------------------------------------- *
 * (ABI 17) Test evaluation under nn.MSELoss at one output column (tools.py:218-237 with the
 * criterion of tools.py:223-224): d_out[0] = mean squared error over n rows (per-block fp64
 * partials, folded in a fixed order as fs_eval's), d_out[1] = 100 * #{y == 0} / n -- the
 * reference's comp_accuracy (tools.py:82-96) takes the top-1 index of a one-column output,
 * always 0, and compares it with the float target; that value is reproduced, not improved.
 * d_y [n] float, d_W [ld]; d_ws needs fs_eval_ws_doubles(n) doubles.
 * ------------------------------------------------------------------------- */
int fs_eval_mse(const float* d_phi, int64_t ld, const float* d_y, int n, const float* d_W, double* d_out,
                double* d_ws, void* stream);

/* ------------------------------------------------------------------------- *
 * (ABI 18) Per-client evaluation: the test_loop metrics (tools.py:218-237) of EVERY client
 * model -- the reference's local_weights[j] (tools.py:340-343, 367-370, 430-433), which it
 * never scores -- from their logits on a row set: d_Z in fs_mix_z's layout below, row v = C
 * segments of ldN = (N + 3) & ~3 floats, client j at d_Z[v][c*ldN + j]; the padding columns
 * N..ldN-1 are read and ignored (they may hold anything).  For every client j < N
 *   d_out[2j]   = mean over the n rows of the cross-entropy of (Z[v][0*ldN+j], ...,
 *                 Z[v][(C-1)*ldN+j]) against d_labels[v]
 *   d_out[2j+1] = 100 * correct / n, top-1, ties to the lowest class index
 * -- fs_eval's definitions.  Z is streamed once (16-byte loads along the client axis, the C
 * logits of a client in registers); per-row losses are summed in fp64 per client over row
 * blocks of fs_z_eval_block_rows() rows with fixed boundaries in absolute row numbers, one
 * partial pair per (row block, client) in the caller-owned workspace d_ws
 * ([row blocks][ldN][2] doubles: fs_z_eval_ws_doubles(n, N)); fs_z_eval_finish folds the row
 * blocks per client in a fixed order.  No atomics, no cross-workgroup wait.  Two contracts:
 *   column independence  a client's two numbers depend on its own column of Z and the labels
 *                        alone -- not on N, its position or its neighbours (bitwise)
 *   chunk independence   the rows may be added in chunks (a bounded scratch Z): the result is
 *                        bitwise the same whatever the chunking
 * fs_z_eval_add adds the partials of rows [row0, row0 + rows) of the n-row set: d_Z points at
 * row row0 (the chunk's first row), d_labels at row 0; row0 must be a multiple of the row
 * block, and only the set's last chunk may end inside a row block.  Every row must be added
 * exactly once before fs_z_eval_finish (which serves both losses).  1 <= C <= 32.
 * fs_z_eval_add_mse: nn.MSELoss at one output column (C = 1, d_Z [n][ldN], d_y [n] float):
 * d_out[2j] = mean (Z[v][j] - y[v])^2, d_out[2j+1] = 100 * #{y == 0} / n -- fs_eval_mse's
 * degenerate accuracy, the same for every client.
 * ------------------------------------------------------------------------- */
int fs_z_eval_block_rows(void);
int64_t fs_z_eval_ws_doubles(int n, int N);
int fs_z_eval_add(const float* d_Z, const int32_t* d_labels, int n, int row0, int rows, int N, int C,
                  double* d_ws, int64_t ws_doubles, void* stream);
int fs_z_eval_add_mse(const float* d_Z, const float* d_y, int n, int row0, int rows, int N, double* d_ws,
                      int64_t ws_doubles, void* stream);
int fs_z_eval_finish(const double* d_ws, int64_t ws_doubles, int n, int N, double* d_out, void* stream);

/* ------------------------------------------------------------------------- *
 * (ABI 19) Local evaluation: the test_loop metrics (tools.py:218-237) of a model on EVERY
 * client's OWN training rows, in one pass over the resident features d_phi (CSR by client:
 * client j owns rows [d_row_off[j], d_row_off[j+1]), int64 [N + 1] on the device).  The
 * reference never reports them: its train_loop keeps a running train_acc.avg (tools.py:213-215)
 * while the weights move, and every caller drops it.  For every client j < N, with
 * n_j = d_row_off[j+1] - d_row_off[j] and the model W_j = d_W + j * w_stride (C rows of ld floats):
 *   d_out[2j]   = mean cross-entropy of W_j over the client's n_j rows
 *   d_out[2j+1] = 100 * correct / n_j, top-1, ties to the lowest class index
 * -- fs_eval's definitions.  w_stride = 0 scores ONE model (the global one) on every client: the
 * per-client distribution of the aggregated model, and sum_j (n_j / n) d_out[2j] is the true
 * objective F(W_g).  w_stride = C * ld scores the clients x params buffer: W_out[j] on client j,
 * the local model on local data.  w_stride must be a multiple of 4 floats.
 *   contract A (bitwise)  d_out[2j..2j+1] equals what fs_eval returns for (d_phi +
 *                         d_row_off[j] * ld, d_labels + d_row_off[j], n_j, W_j) -- so a client's
 *                         result does not depend on N, on its position or on its neighbours
 * One 8-wave workgroup per 16-row group counted from the client's first row (client j owns
 * ceil(n_j / 16) groups) runs fs_eval's group body and writes its fp64 partial pair to the
 * workspace; one 256-thread workgroup per client then folds that client's partials with fs_eval's
 * finaliser arithmetic and divides by n_j.  A workgroup finds its client by binary search in the
 * prefix of group counts, which a one-workgroup pre-kernel writes into the head of the workspace
 * from d_row_off.  Three launches on `stream`; the call is asynchronous, allocates nothing, copies
 * nothing from the host and never synchronises; no atomics, no cross-workgroup wait.
 * h_n [N] (HOST, int64; the n_j above, each >= 1) sizes the grid and is read during the call
 * only.  1 <= C <= 32, ld % 64 == 0; any N whose group count fits 31 bits.
 * d_ws: fs_eval_clients_ws_doubles(total_rows, N) doubles, total_rows = sum_j n_j:
 *   (N + 2) / 2  +  2 * (total_rows / 16 + N)      (integer divisions)
 * -- N + 1 int32 prefix entries, then one pair per group, of which there are at most
 * total_rows / 16 + N.  The workspace holds nothing between calls.
 * fs_eval_clients_mse: the same under nn.MSELoss at one output column (C = 1, d_y float targets
 * by row, W_j = d_W + j * w_stride of ld floats): fs_eval_mse's definitions and row body, held to
 * fs_eval_mse on the slices bit for bit.
 * ------------------------------------------------------------------------- */
int64_t fs_eval_clients_ws_doubles(int64_t total_rows, int N);
int fs_eval_clients(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int64_t* h_n,
                    const int32_t* d_labels, int N, const float* d_W, int64_t w_stride, int C, double* d_out,
                    double* d_ws, int64_t ws_doubles, void* stream);
int fs_eval_clients_mse(const float* d_phi, int64_t ld, const int64_t* d_row_off, const int64_t* h_n,
                        const float* d_y, int N, const float* d_W, int64_t w_stride, double* d_out, double* d_ws,
                        int64_t ws_doubles, void* stream);

/* ------------------------------------------------------------------------- *
 * FedAMW mixture step 1: Z[v][c*ldN + n] = sum_d X_val[v][d] * W_n[c][d], where
 * ldN = (N + 3) & ~3 (d_Z holds n_val * C * ldN floats; padding columns are 0)
 * (the inner matmul of tools.py:448, hoisted out of the p-SGD loop because the
 * stacked W of tools.py:435-440 is fixed during it).  fp32 MFMA GEMM.
 * ------------------------------------------------------------------------- */
int fs_mix_z(const float* d_W_all, const float* d_X_val, int64_t ld, int N, int C, int n_val,
             float* d_Z, void* stream);

/* ------------------------------------------------------------------------- *
 * FedAMW mixture step 2: `epochs` passes of SGD(momentum) on p over the pooled
 * validation set (tools.py:441-453): per batch of <= Bv rows (order from d_perms,
 * [epochs][n_val]): out[b,c] = sum_n p_n Z[v_b][c*ldN+n]; CE mean; grad_p;
 * buf = first ? grad : momentum*buf + grad; p -= lr_p*buf.  d_p, d_buf [N] are
 * updated in place; *d_first (int) is read and cleared (the momentum buffer of
 * torch.optim.SGD starts empty, tools.py:423).  A single persistent workgroup
 * where a register-resident instance covers (N, C, Bv) -- for N <= 16 with C <= 2 one wave
 * ("bin", no LDS, no barrier); for N <= 128 the quarter-wave
 * solver (4 batch rows per wave), with 4 L2 prefetch helper workgroups on its XCD that
 * only load (fs_tuning.mix_prefetch sets their number, -1 = none; their progress word is
 * byte 128 of the error block); for N > 256 the multi-CU quarter-wave solver "qmc"
 * (K <= 16 workgroups of 128 clients on one XCD, one exchange hop per step, 16 helper
 * workgroups); otherwise (Bv <= 16, C <= 16, N <= 2048) K <= 32 workgroups that split the
 * clients and exchange partial logits every step (slices of S >= 16 clients: reduce-scatter
 * to owner workgroups, then an all-gather of the totals); otherwise one LDS-staged /
 * global workgroup.
 * d_ws: fs_mix_solve_ws_bytes(N, C, Bv) bytes, zeroed once at allocation (the multi-CU
 * exchange granules + the error block; a timed-out exchange also writes NaN into d_p).
 * Concurrent solves need separate workspaces.  fs_tuning.mix_solver (FS_SOLVER_*) forces a
 * solver (tests, diagnostics; one that does not cover the shape falls through).
 * ------------------------------------------------------------------------- */
int64_t fs_mix_solve_ws_bytes(int N, int C, int Bv);
int fs_mix_solve(const float* d_Z, const int32_t* d_labels, const int32_t* d_perms, int N, int C,
                 int n_val, int epochs, int Bv, float lr_p, float momentum, float* d_p, float* d_buf,
                 int* d_first, void* d_ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * (ABI 17) FedAMW mixture step 2 under nn.MSELoss at one output column (tools.py:441-453
 * with the criterion of tools.py:421-422; FedAMW_OneShot tools.py:304-316, momentum 0):
 * d_Z is what fs_mix_z writes at C = 1, [n_val][ldN]; d_y [n_val] float targets.  Per batch:
 * out_b = sum_n p_n Z[v_b][n];  L = mean_b (out_b - y_b)^2;  grad_n = (2/|b|) sum_b (out_b -
 * y_b) Z[v_b][n];  buf = first ? grad : momentum * buf + grad;  p -= lr_p * buf.  d_p, d_buf,
 * d_first, d_perms, the workspace (fs_mix_solve_ws_bytes(N, 1, Bv); its error block stays
 * clear: one workgroup, no exchange) and the return codes as fs_mix_solve.  One persistent
 * workgroup with p and buf in registers.  Requires 1 <= Bv <= 64 and N <= 4096, else
 * FS_EUNSUPPORTED (there is no multi-CU form and no rank-blocked layout under MSE).
 * ------------------------------------------------------------------------- */
int fs_mix_solve_mse(const float* d_Z, const float* d_y, const int32_t* d_perms, int N, int n_val, int epochs,
                     int Bv, float lr_p, float momentum, float* d_p, float* d_buf, int* d_first, void* d_ws,
                     int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * (ABI 12) fs_mix_solve on the rank-blocked Z that one all-gather of the per-rank
 * Z blocks produces (the sharded FedAMW round, dist.py): d_Z is
 * [blocks][n_val][C][L], L = N / blocks (a multiple of 4), client n = block n / L,
 * column n % L -- no layout copy into [n_val][C][N] first.  Read by the qmc solver
 * only (N > 256, C <= 16, Bv <= 16; fs_tuning.mix_solver AUTO or QMC); any other
 * shape or forced solver returns FS_EUNSUPPORTED (use fs_mix_solve on the standard
 * layout).  Same arithmetic in the same order as fs_mix_solve on the standard layout:
 * bitwise the same p and momentum buffer.  Arguments otherwise as fs_mix_solve.
 * fs_mix_solve_blocked_covers tells, before the all-gather, which layout to assemble.
 * ------------------------------------------------------------------------- */
int fs_mix_solve_blocked(const float* d_Z, int blocks, const int32_t* d_labels, const int32_t* d_perms, int N,
                         int C, int n_val, int epochs, int Bv, float lr_p, float momentum, float* d_p, float* d_buf,
                         int* d_first, void* d_ws, int64_t ws_bytes, void* stream);
/* host-only: 1 if fs_mix_solve_blocked covers this shape under the calling thread's tuning */
int fs_mix_solve_blocked_covers(int N, int C, int n_val, int epochs, int Bv);

/* Diagnostic (host state only): the solver the calling thread's last fs_mix_solve
 * launched -- FS_SOLVER_REG (1, register-resident, one row per wave), _MC (2, multi-CU),
 * _STAGED (3), _GLOBAL (4), _REG2 (5, two rows per wave, Bv <= 16, C <= 10), _WAVE (6, one
 * wave: N <= 16, C <= 4, Bv <= 16), _QUAD (8, quarter-wave: N <= 64 with C <= 16, or N <= 128
 * with C <= 10; Bv <= 16), _QMC (9, multi-CU quarter-wave), _BIN (10, one wave, two classes:
 * N <= 16, C <= 2, Bv <= 16); 0 = none yet. */
int fs_mix_solve_last_mode(void);
/* (ABI 14) Diagnostic: the layout of the calling thread's last fs_mix_solve /
 * fs_mix_solve_blocked launch when it ran the qmc solver -- its workgroups K and clients per
 * lane (4 or 8; K = ceil(ldN / (16 * lane_clients))) -- else 0 and 0. */
int fs_mix_solve_last_layout(int* workgroups, int* lane_clients);
/* (ABI 20) host-only, no device state: what fs_mix_solve (blocks = 1) or fs_mix_solve_blocked
 * (blocks > 1; its N % (4 blocks) check is not repeated here, and it launches only where the
 * answer is qmc) would launch for this shape under the calling thread's tuning.
 *   solver        FS_SOLVER_* as fs_mix_solve_last_mode reports it after the launch
 *   workgroups, lane_clients   as fs_mix_solve_last_layout: qmc's K and clients per lane, else 0, 0
 *   helpers       L2 prefetch helper workgroups, after the solver's own bound (given a workspace)
 *   lead          steps they run ahead (0 without helpers)
 *   poll_delay    qmc: s_sleep(1) units before a step's first poll, else 0
 *   ws_bytes      workspace bytes the launch uses (<= fs_mix_solve_ws_bytes(N, C, Bv)) */
typedef struct fs_mix_plan {
  int solver, workgroups, lane_clients, helpers, lead, poll_delay;
  int64_t ws_bytes;
} fs_mix_plan;
int fs_mix_solve_plan(int N, int C, int n_val, int epochs, int Bv, int blocks, fs_mix_plan* out);
/* (ABI 15) Diagnostic (host state only): the kernel the calling thread's last fs_local_train
 * launched -- FS_LT_SINGLE (1, one workgroup per client), FS_LT_SPLIT (2), FS_LT_DBUF (3, the
 * split form's double-buffered instance: the rows streamed ahead of the hand-off),
 * FS_LT_PAIR (4), FS_LT_PIPE (5), FS_LT_TEAMS (6), FS_LT_MB (7, ABI 16: the split form's
 * 4x4x1 multi-block instances, fs_tuning.split_mb), FS_LT_WIDE (8, ABI 21: the batch-tiled
 * form, G = 1 | FS_G_WIDE); 0 = none yet. */
#define FS_LT_SINGLE 1
#define FS_LT_SPLIT 2
#define FS_LT_DBUF 3
#define FS_LT_PAIR 4
#define FS_LT_PIPE 5
#define FS_LT_TEAMS 6
#define FS_LT_MB 7
#define FS_LT_WIDE 8
int fs_local_train_last_kernel(void);

/* ------------------------------------------------------------------------- *
 * Random Fourier feature map.  Replaces RFF's use in feature_mapping
 * (tools.py:22-31: `1 / np.sqrt(D) * torch.cos(torch.matmul(X, W) + b)`, called at
 * exp.py:63 for the training and the test set with one draw of W, b):
 *   d_out[i][k] = scale * cos(sum_j d_X[i][j] * d_W[j][k] + d_b[k])   (k < D)
 *   d_out[i][k] = 0                                                   (D <= k < ldo)
 * d_X [n][ldx] raw features (d used), d_W [d][D] row-major, d_b [D]; scale = 1/sqrt(D).
 * The draw of W and b stays on the host generator (tools.py:15-19).  fp32 MFMA GEMM
 * with the +b / cos / scale epilogue fused; phi written once, in the engine's padded
 * layout when ldo > D.
 * ------------------------------------------------------------------------- */
int fs_feature_map(const float* d_X, int64_t ldx, const float* d_W, const float* d_b, int n, int d, int D,
                   float scale, float* d_out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------- *
 * Data heterogeneity of a partition (exp.py:67-74):
 *   fs_gram:   d_G[a][b] = sum_r phi[r][a] * phi[r][b] over rows [0, rows)   (D x D, row
 *              stride ldg; exactly symmetric).  `torch.matmul(X.T, X)` of exp.py:67
 *              before the division by len.
 *   fs_hetero: d_S[j] = sum_{a,b} (G[a][b] / n_total - G_j[a][b] / n_j)^2 with G_j the
 *              Gram of client j's rows [row_off[j], row_off[j+1]) (never materialised);
 *              the caller forms sum_j n_j / n_total * sqrt(d_S[j]) (exp.py:73).
 * phi [rows][ld] fp32 packed by client, ld % 64 == 0, columns >= D ignored.  MFMA SYRK.
 * ------------------------------------------------------------------------- */
int fs_gram(const float* d_phi, int64_t ld, int64_t rows, int D, float* d_G, int64_t ldg, void* stream);
int fs_hetero(const float* d_phi, int64_t ld, const int64_t* d_row_off, int N, int D, const float* d_G,
              int64_t ldg, int64_t n_total, double* d_S, void* stream);


/* ------------------------------------------------------------------------- *
 * Round plan: the native round driver.  One fs_plan_round call enqueues the
 * launches of one round of the reference's loop (tools.py:337-352 FedAvg,
 * 364-379 FedProx; the train / aggregate / evaluate phases of FedAMW, 427-462):
 *   FS_PHASE_TRAIN      fs_local_train over all N clients with the shuffles of
 *                       round t; losses to d_loss_hist[t*N .. t*N+N)
 *   FS_PHASE_AGGREGATE  fs_aggregate(W_out, p) -> d_W_g  (p = d_p, or the override)
 *   FS_PHASE_EVAL       fs_eval(d_W_g) -> d_eval_hist[2t], [2t+1]
 *   FS_PHASE_EVAL_DEFER (with FS_PHASE_EVAL) round t's evaluation may ride on the
 *                       next call's TRAIN launch, on the CUs its client groups
 *                       leave idle (parallel split launches, C <= 16; the same
 *                       per-row arithmetic as fs_eval).  d_eval_hist[2t..] is then
 *                       written by that call if it aggregates, else (round 5) by the
 *                       call after it: the fused evaluation's finaliser rides on the
 *                       next AGGREGATE launch, and any call that trains or does not
 *                       aggregate runs a pending one first -- make one more
 *                       fs_plan_round call (phases 0 will do) or, since ABI 15,
 *                       fs_plan_eval_flush before reading d_eval_hist after a
 *                       TRAIN-only call.  The pending evaluation reads d_W_g
 *                       as it is when that next call's launches run: the caller
 *                       must NOT write d_W_g (its own aggregate, an all-reduce into
 *                       it, a copy) between the deferring call and the next
 *                       fs_plan_round.  Which launch carries it: a next call whose
 *                       phases include TRAIN fuses it into the training launch, which
 *                       runs before that call's own AGGREGATE rewrites d_W_g; a next
 *                       call without TRAIN runs it as an fs_eval launch of its own
 *                       before anything else.  The fp64 sum of the per-block partials
 *                       then follows the launch's evaluation-block count (CUs left
 *                       idle), so deferred and standalone losses agree to ~1e-12
 *                       relative, not bitwise.  Do not defer the last round's
 *                       evaluation.
 * fs_plan_shuffle(plan, seeds, t) replays round t's N*E training shuffles
 * (DataLoader passes of tools.py:179, client-major / epoch-minor seeds) into slot
 * t % 2 on the plan's side stream -- on the GPU (fs_randperm_device, default) or on
 * the plan's host thread pool plus an async upload; call it for round t+1 after
 * enqueueing round t so it overlaps the GPU.
 * The plan owns its shuffle buffers, copy stream and events; every other pointer
 * is borrowed and must outlive the plan.
 * ------------------------------------------------------------------------- */
#define FS_PHASE_TRAIN 1
#define FS_PHASE_AGGREGATE 2
#define FS_PHASE_EVAL 4
#define FS_PHASE_EVAL_DEFER 8

typedef struct fs_plan fs_plan;

typedef struct fs_plan_desc {
  /* local training (see fs_local_train) */
  const float* d_phi;
  int64_t ld;
  const int64_t* d_row_off;
  const int32_t* d_labels;
  const int32_t* d_order;
  const int64_t* h_n;          /* [N] rows per client (host) */
  int N, C, B, E;
  int G;                       /* from fs_local_train_plan (1 when chained) */
  void* d_ws;
  int64_t ws_bytes;
  int chained, prox, reg;
  float mu, lam;
  float* d_W_g;                /* [C][ld] round-start model; the aggregate is written here */
  float* d_W_out;              /* [N][C][ld] */
  double* d_loss_hist;         /* [R][N] */
  /* aggregation (see fs_aggregate) */
  const float* d_p;            /* [N] default mixture weights (may be NULL) */
  float* d_agg_ws;
  int64_t agg_ws_floats;
  int agg_chunks;
  /* evaluation (see fs_eval; may be NULL when FS_PHASE_EVAL is never used) */
  const float* d_phi_t;
  const int32_t* d_labels_t;
  int n_t;
  double* d_eval_ws;
  double* d_eval_hist;         /* [R][2] */
  int shuffle_device;          /* 1: replay shuffles with fs_randperm_device on the plan's side
                                  stream; 0: on the plan's host thread pool + async upload */
  int host_threads;            /* host replay threads; <= 0: min(16, hardware) */
  int shuffle_after_train;     /* 1 (device replay): round t+1's shuffles also wait for round t's
                                  local training, so they run beside what follows it (FedAMW: the
                                  p-solve, which leaves most CUs idle) instead of holding CUs a
                                  group of the split kernel is waiting for */
  /* (ABI 17) the task's loss: 0 = cross-entropy (everything above), 1 = MSE at one output column
     (tools.py:183-184, 223-224): TRAIN launches fs_local_train_mse on d_y, EVAL launches
     fs_eval_mse on d_y_t; C and G must both be 1 (else FS_EINVAL); d_labels / d_labels_t are not
     read.  FS_PHASE_EVAL_DEFER is accepted but never fused: fs_plan_eval_blocks is 0 and the
     evaluation runs as a launch of its own in the call that would have carried it. */
  int loss;
  const float* d_y;            /* [rows] float targets (loss == 1) */
  const float* d_y_t;          /* [n_t] float test targets (loss == 1) */
} fs_plan_desc;

int64_t fs_plan_desc_size(void);   /* sizeof(fs_plan_desc), for binding-layout checks */
int fs_plan_create(const fs_plan_desc* desc, fs_plan** out);
int fs_plan_destroy(fs_plan* plan);
int fs_plan_shuffle(fs_plan* plan, const int64_t* h_seeds, int t);
int fs_plan_round(fs_plan* plan, int t, float lr, int phases, const float* d_p_override, void* stream);
/* ABI 15: complete on `stream` every evaluation the plan still holds (a deferred one not yet
 * carried by a TRAIN launch, a fused one whose finaliser waits for the next AGGREGATE), so
 * d_eval_hist is final once the stream reaches this point.  Replaces the "one more
 * fs_plan_round call with phases 0" of ABI 14 (which still works). */
int fs_plan_eval_flush(fs_plan* plan, void* stream);
/* ABI 7 (device replay only; call before the first fs_plan_shuffle): generate the shuffles of
 * `rounds` consecutive rounds (a chunk: rounds cK .. cK+K-1) with ONE fs_randperm_device launch
 * into one of two chunk slots.  fs_plan_shuffle then only collects round t's seeds and launches
 * when the chunk's last round arrives (a partly collected chunk is launched by the first
 * fs_plan_round that needs it); the local training waits for its slot, and releases it, once
 * per chunk instead of once per round -- no cross-stream wait between the rounds of a chunk.
 * Rounds must be prepared in order; prepare chunk c+1 while chunk c runs. */
int fs_plan_set_shuffle_chunk(fs_plan* plan, int rounds);
/* ABI 7: launch a partly collected chunk now (after preparing a run's last round). */
int fs_plan_shuffle_flush(fs_plan* plan);
/* ABI 8: evaluation workgroups a TRAIN launch of this plan carries for FS_PHASE_EVAL_DEFER
 * (0: the plan evaluates with launches of its own; fs_tuning.no_eval_fuse = 1 at creation
 * forces 0). */
int fs_plan_eval_blocks(const fs_plan* plan);

/* ------------------------------------------------------------------------- *
 * (ABI 22) Partial client participation: a round in which only M <= N sampled clients train
 * and are aggregated (McMahan's C; parallel clients, each from the round's d_W_g).
 *   fs_plan_shuffle_subset  replays only the M*E passes of the sampled clients h_sel (host,
 *                       strictly ascending ids in [0, N)) into slot t % 2, at the plan's usual
 *                       offsets E*row_off[j] + e*n_j; h_seeds [M*E] sel-major / epoch-minor.
 *                       Device replay: seeds and a per-round pass table in the pinned seed slot,
 *                       one fs_randperm_device launch; host replay: the pool over the M*E passes.
 *   fs_plan_round_subset    fs_plan_round over the sample: TRAIN launches the plan's training
 *                       form over the M clients of d_sel_order (the ids of d_sel in dispatch
 *                       order, longest first) on the unchanged d_W_out and
 *                       d_loss_hist[t*N ..]: rows and entries of clients outside the sample are
 *                       not written.  AGGREGATE is fs_aggregate_sel(d_W_out, d_sel, d_q, M) into
 *                       d_W_g (d_sel ascending: the fold order).  EVAL / EVAL_DEFER as
 *                       fs_plan_round: a deferred evaluation fuses into the subset TRAIN launch
 *                       with the plan's block count (M <= N leaves no fewer CUs idle) and its
 *                       finaliser rides on the gathered aggregate.
 * d_sel, d_sel_order and d_q are device arrays read asynchronously: keep them alive (and
 * unchanged) until the round's launches have run.  Rounds of both kinds may alternate on one
 * plan; TRAIN returns FS_EINVAL when the slot was prepared for another client count.  Only the
 * count is checked (the ids of the round call live on the device): passing the ids the shuffle
 * call was given is the caller's contract -- a client of another sample would train on whatever
 * shuffles its passes last received (zeros before the first: row 0 of the client every step).
 * Returns FS_EUNSUPPORTED for a chained plan (the chain walkers index clients by position),
 * FS_EINVAL for M < 1, M > N, a null pointer, ids not strictly ascending in range, or after
 * fs_plan_set_shuffle_chunk(K > 1) (subset rounds use per-round slots).
 * ------------------------------------------------------------------------- */
int fs_plan_shuffle_subset(fs_plan* plan, const int64_t* h_seeds, const int32_t* h_sel, int M, int t);
int fs_plan_round_subset(fs_plan* plan, int t, float lr, int phases, const int32_t* d_sel,
                         const int32_t* d_sel_order, const float* d_q, int M, void* stream);

/* (ABI 23) The aggregation rule of this plan's AGGREGATE phase.  mode 0 (the default) is the plain
 * aggregate; FS_NOVA_REFERENCE / FS_NOVA_UPDATES make AGGREGATE launch fs_aggregate_nova in that
 * mode instead of fs_aggregate / fs_aggregate_sel, with d_q = the round's weights (d_p, the
 * override, or the subset call's d_q), d_sel = the subset's ids or NULL, d_W_base = d_W_g (mode 2
 * updates the round-start model in place) and the same finaliser handling.  Host state: the next
 * fs_plan_round / fs_plan_round_subset whose phases include FS_PHASE_AGGREGATE reads it when it
 * enqueues, so it may change between rounds (a sampled round's d_b / te / s0).  d_b [N, or M of a
 * subset round] is a device array read asynchronously by those launches (mode 1 only).  Nothing
 * else about the plan changes.  FS_EINVAL for mode 2 on a chained plan (a chained client's
 * W_j - W_g contains its predecessors' work), mode 1 with a null d_b, or another mode. */
int fs_plan_set_nova(fs_plan* plan, int mode, const float* d_b, float te, float s0);

/* (additive to ABI 23) SCAFFOLD rounds.  Host state read when the next round call enqueues, as
 * fs_plan_set_nova's.  on = 1: TRAIN launches fs_local_train_scaffold (the plan's G and workspace
 * are ignored) with d_c [C][ld] and d_ci [N][C][ld]; AGGREGATE launches fs_aggregate_scaffold with
 * the round's d_q (d_p, the override, or the subset call's d_q), d_r ([N]; [M] of a subset round)
 * and cs, updating d_W_g and d_c in place.  d_r and cs change with the round's lr and sample: call
 * again before each round, which is allowed whatever the plan holds while it is on.  Subset
 * rounds, chunked shuffles and the device replay work unchanged.  A deferred evaluation is never
 * fused while it is on: it runs as an fs_eval launch of its own before the next TRAIN, as on
 * loss = 1 plans.  d_c, d_ci and d_r are read (d_c, d_ci also written) asynchronously by the
 * launches: keep them alive.  on = 0 restores the plan as it was (the pointers are ignored).
 * FS_EINVAL for a chained plan, loss = 1, B > 64, a plan with prox on, a nova mode other than 0,
 * a null pointer with on = 1, or turning it on while the plan holds a pending evaluation
 * (fs_plan_eval_flush first). */
int fs_plan_set_scaffold(fs_plan* plan, int on, float* d_c, float* d_ci, const float* d_r, float cs);

/* (additive to ABI 23) A server optimizer on this plan's AGGREGATE phase.  Host state read when
 * the next round call enqueues, as fs_plan_set_nova's.  rule FS_OPT_AVGM .. FS_OPT_YOGI: AGGREGATE
 * launches fs_aggregate_opt with d_q = the round's weights (d_p, the override, or the subset
 * call's d_q, already p_k / sum_S p), d_sel = the subset's ids or NULL, d_W_g in place, the
 * moments d_m and d_v [C][ld] in place, the plan's aggregation workspace and chunks, and the
 * pending finaliser of a deferred evaluation.  TRAIN is unchanged: every training form, the prox
 * term, loss = 1, B > 64, subset rounds, chunked shuffles and the fused deferred evaluation work
 * as without it.  d_m and d_v are read and written asynchronously by those launches: keep them
 * alive (d_v may be NULL for FS_OPT_AVGM).  rule 0 restores the plain aggregate (the other
 * arguments are ignored).  FS_EINVAL for a chained plan (a chained client's W_j - W_g holds its
 * predecessors' work), a nova mode other than 0, SCAFFOLD on, null moments, tau <= 0 for rules
 * 2..4, or another rule; fs_plan_set_nova and fs_plan_set_scaffold refuse in turn while a rule is
 * set. */
int fs_plan_set_server_opt(fs_plan* plan, int rule, float* d_m, float* d_v, float eta, float beta1, float omb1,
                           float beta2, float omb2, float tau);

/* (additive to ABI 23) q-FedAvg on this plan's AGGREGATE phase.  Host state read when the next
 * round call enqueues, as fs_plan_set_server_opt's.  on = 1: AGGREGATE launches fs_aggregate_qffl
 * with d_u = the round's weights (d_p, the override, or the subset call's d_q: the caller puts
 * fs_qffl_coef's u there), d_g ([N]; [M] of a subset round), Lc, d_sel = the subset's ids or NULL,
 * d_W_g in place, the outputs d_S [C][ld], d_n ([N] / [M]) and d_hc [2], the plan's aggregation
 * workspace and chunks, d_nws (the largest fs_aggregate_qffl_ws_doubles(M, C * ld) over 1 <= M <= N
 * doubles: the table is largest at the last M of a regime of the fold, not always at N) and the
 * pending finaliser of a deferred evaluation.  TRAIN is unchanged: every training form, the prox term,
 * loss = 1, B > 64, subset rounds, chunked shuffles and the fused deferred evaluation work as
 * without it.  Lc follows the round's lr: call again before each round (allowed while on).  The
 * buffers are read and written asynchronously by those launches: keep them alive.  on = 0 restores
 * the plain aggregate (the other arguments are ignored).  FS_EINVAL for a chained plan, a nova mode
 * other than 0, SCAFFOLD on, a server-optimizer rule set, a null pointer, Lc <= 0 or not finite,
 * d_S == d_W_g or a d_nws too small; fs_plan_set_nova, fs_plan_set_scaffold and
 * fs_plan_set_server_opt refuse in turn while it is on. */
int fs_plan_set_qffl(fs_plan* plan, int on, const float* d_g, double Lc, float* d_S, double* d_n, double* d_hc,
                     double* d_nws, int64_t nws_doubles);

/* (additive to ABI 23) robust aggregation on this plan's AGGREGATE phase.  Host state read when the
 * next round call enqueues, as fs_plan_set_server_opt's.  on = 1: AGGREGATE launches
 * fs_aggregate_robust over the round's rows of d_W_out (all N, or the subset call's M ids) into
 * d_W_g, with the pending finaliser of a deferred evaluation.  mode FS_ROBUST_TRIMMED_MEAN (1):
 * b = floor(trim * M) in double, M the round's own client count, clamped to (M-1)/2;
 * mode FS_ROBUST_MEDIAN (2): b = (M-1)/2 (trim is ignored).  The rule is unweighted: the round's
 * weights are not read.  TRAIN and EVAL are unchanged: every training form, the prox term, loss = 1,
 * B > 64 and subset rounds work as without it.  on = 0 restores the plain aggregate.  FS_EINVAL for
 * a chained plan, N > fs_aggregate_robust_max_m(), an unknown mode, trim outside [0, 0.5), a nova
 * mode other than 0, SCAFFOLD on, a server-optimizer rule set or q-FedAvg on; fs_plan_set_nova,
 * fs_plan_set_scaffold, fs_plan_set_server_opt and fs_plan_set_qffl refuse in turn while it is on. */
#define FS_ROBUST_TRIMMED_MEAN 1
#define FS_ROBUST_MEDIAN 2
int fs_plan_set_robust(fs_plan* plan, int on, int mode, double trim);

/* (additive to ABI 23) Krum / Multi-Krum on this plan's AGGREGATE phase.  Host state read when the
 * next round call enqueues, as fs_plan_set_robust's.  on = 1: AGGREGATE launches fs_aggregate_krum
 * over the round's rows of d_W_out (all N, or the subset call's M ids) with x = d_W_g into d_W_g,
 * with the pending finaliser of a deferred evaluation on its fold.  f = min(floor(f_frac * M),
 * (M - 3) / 2) in double from the round's own client count M; m_mode 1: m = 1 (Krum), 0: m = M - f
 * (Multi-Krum), any other count: min(m_mode, M - f).  d_pick [N] int32 and d_score [N] double take
 * the round's picked ids (the first m entries) and scores (by position); d_ws of ws_bytes >=
 * fs_aggregate_krum_ws_bytes(N, C * ld) bytes, D at its start.  The round's weights are not read.
 * TRAIN and EVAL are unchanged: every training form, the prox term, loss = 1, B > 64 and subset
 * rounds work as without it; a subset round of M < 3 clients fails with FS_EINVAL when it
 * enqueues.  on = 0 restores the plain aggregate.  FS_EINVAL for a chained plan, N < 3,
 * N > fs_aggregate_krum_max_m(), f_frac outside [0, 0.5), m_mode < 0, a null buffer, a workspace
 * that is too small, a nova mode other than 0, SCAFFOLD on, a server-optimizer rule set, q-FedAvg
 * on or a robust aggregate on; fs_plan_set_nova, fs_plan_set_scaffold, fs_plan_set_server_opt,
 * fs_plan_set_qffl and fs_plan_set_robust refuse in turn while it is on. */
int fs_plan_set_krum(fs_plan* plan, int on, double f_frac, int m_mode, int32_t* d_pick, double* d_score, void* d_ws,
                     int64_t ws_bytes);

/* (additive to ABI 23) RFA on this plan's AGGREGATE phase.  Host state read when the next round
 * call enqueues, as fs_plan_set_krum's.  on = 1: AGGREGATE launches fs_aggregate_rfa over the
 * round's rows of d_W_out (all N, or the subset call's M ids) with x = d_W_g into d_W_g, T, nu and
 * init as given, with the pending finaliser of a deferred evaluation on its last step.  alpha is
 * the round's weights (d_p_override or the plan's p, the subset call's q: as q-FedAvg takes
 * them), or f32(1 / M) for every row when uniform is set.  d_dist [N] double, d_b [N] float and
 * d_obj [T + 2] double take the round's recorded values (by position); d_ws of ws_bytes >=
 * fs_aggregate_rfa_ws_bytes(N, C * ld) bytes.  TRAIN and EVAL are unchanged: every training form,
 * the prox term, loss = 1, B > 64 and subset rounds work as without it.  on = 0 restores the plain
 * aggregate.  FS_EINVAL for a chained plan, N > fs_aggregate_rfa_max_m(), T outside [0, 32],
 * nu <= 0 or not finite, an unknown init, a null buffer, a workspace that is too small, a nova
 * mode other than 0, SCAFFOLD on, a server-optimizer rule set, q-FedAvg on, a robust aggregate
 * on or Krum on; fs_plan_set_nova, fs_plan_set_scaffold, fs_plan_set_server_opt,
 * fs_plan_set_qffl, fs_plan_set_robust and fs_plan_set_krum refuse in turn while it is on. */
int fs_plan_set_rfa(fs_plan* plan, int on, int T, double nu, int init, int uniform, double* d_dist, float* d_b,
                    double* d_obj, void* d_ws, int64_t ws_bytes);

/* (additive to ABI 23) FedTopK on this plan's AGGREGATE phase.  Host state read when the next round
 * call enqueues, as fs_plan_set_rfa's.  on = 1: AGGREGATE launches fs_aggregate_topk over the
 * round's rows of d_W_out (all N, or the subset call's M ids) with the round's normalised weights
 * as q (d_p_override or the plan's p, the subset call's q), kcount as given, d_W_g in place, the
 * plan's aggregation workspace and chunks, and the pending finaliser of a deferred evaluation on
 * the fold.  d_e [N][C * ld] floats is the clients' residual memory, updated in place by client id
 * (a client outside the round keeps its row); NULL: top-k without memory.  d_tau [N] float and
 * d_kept [N] int32 take the round's thresholds and kept counts (by position); d_sws of sws_bytes >=
 * fs_aggregate_topk_ws_bytes(N, C * ld) bytes (0: may be NULL).  TRAIN and EVAL are unchanged: every
 * training form, the prox term, loss = 1, B > 64 and subset rounds work as without it.  on = 0
 * restores the plain aggregate.  FS_EINVAL for a chained plan, kcount outside [1, C * ld], a null
 * d_tau or d_kept, d_e equal to d_W_g or d_W_out, a workspace that is too small, a nova mode other
 * than 0, SCAFFOLD on, a server-optimizer rule set, q-FedAvg on, a robust aggregate on, Krum on or
 * RFA on; fs_plan_set_nova, fs_plan_set_scaffold, fs_plan_set_server_opt, fs_plan_set_qffl,
 * fs_plan_set_robust, fs_plan_set_krum and fs_plan_set_rfa refuse in turn while it is on. */
int fs_plan_set_topk(fs_plan* plan, int on, int64_t kcount, float* d_e, float* d_tau, int32_t* d_kept, void* d_sws,
                     int64_t sws_bytes);

/* (additive to ABI 23) DP-FedAvg on this plan's AGGREGATE phase.  Host state read when the next round
 * call enqueues, as fs_plan_set_topk's.  on = 1: AGGREGATE launches fs_aggregate_dp over the round's
 * rows of d_W_out (all N, or the subset call's M ids) with the round's normalised weights as q
 * (uniform != 0: 1 / M), the round call's t as the noise round, d_W_g in place, the plan's
 * aggregation workspace and chunks, and the pending finaliser of a deferred evaluation on the fold.
 * d_c [N] float, d_r [N] double and d_state [FS_DP_STATE] double take the round's coefficients, norms
 * (by position) and state; d_clip [1] double is the adaptive clip (adaptive != 0: set to S before
 * the first round by the caller, updated on the device every round; else ignored); cols = D, the
 * model's real columns of its ld (the padding takes no noise: it stays exactly 0); d_sws of
 * sws_bytes >= fs_aggregate_dp_ws_bytes(N, C * ld) bytes.  TRAIN and EVAL are unchanged.  on = 0
 * restores the plain aggregate.  FS_EINVAL for a chained plan, the rule's refusals of
 * fs_aggregate_dp, a null d_c, d_r, d_state or d_sws, a workspace that is too small, a nova mode
 * other than 0, SCAFFOLD on, a server-optimizer rule set, q-FedAvg on, a robust aggregate on, Krum
 * on, RFA on or FedTopK on; their setters refuse in turn while it is on. */
int fs_plan_set_dp(fs_plan* plan, int on, double S, double z, uint64_t seed, int uniform, int adaptive, double gamma,
                   double eta, double sigma_b, double* d_clip, int64_t cols, float* d_c, double* d_r, double* d_state,
                   void* d_sws, int64_t sws_bytes);

/* ABI 7, measurement: timing events recorded without a system-scope release (so timing a
 * launch inside a round does not stall the next one); elapsed_ms synchronises on `end`. */
int fs_timer_create(void** ev);
int fs_timer_record(void* ev, void* stream);
int fs_timer_elapsed_ms(void* start, void* end, float* ms);
int fs_timer_destroy(void* ev);

#ifdef __cplusplus
}
#endif

#endif /* FEDSIM_H */

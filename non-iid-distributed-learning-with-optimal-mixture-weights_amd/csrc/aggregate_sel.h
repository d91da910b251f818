// The aggregation rules' launchers, as the round plan (round.hip) and each other call them.  The
// regime threshold and the sub-range and chunk rules they share are aggregate_geom.h's, the kernels
// and the dispatch of the weighted folds aggregate_fold.h's.
#pragma once
#include "aggregate_geom.h"
#include "finalize.h"

namespace fs {

// stage 2 of a plain sum (aggregate.hip): K partials of 4 * len4 floats at d_part folded by the fixed
// tree into d_out
void fold_partials_launch(const float* d_part, int K, int64_t len4, float* d_out, hipStream_t st);

// fs_aggregate_sel with an optional finaliser (nullptr: none), as aggregate_launch
int aggregate_sel_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                         int64_t len, float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks,
                         const EvalFinalize* fin, hipStream_t st);

// fs_aggregate_nova (aggregate_nova.hip) with an optional finaliser, as the two above
int aggregate_nova_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                          const float* d_b, float te, float s0, int mode, const float* d_W_base, int M, int64_t len,
                          float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks, const EvalFinalize* fin,
                          hipStream_t st);

// fs_aggregate_opt (aggregate_opt.hip) with an optional finaliser, as the three above
int aggregate_opt_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int rule,
                         float eta, float beta1, float omb1, float beta2, float omb2, float tau, int M, int64_t len,
                         float* d_W_g, float* d_m, float* d_v, float* d_ws, int64_t ws_floats, int chunks,
                         const EvalFinalize* fin, hipStream_t st);

// fs_aggregate_qffl (aggregate_qffl.hip) with an optional finaliser, as the four above
int aggregate_qffl_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_u,
                          const float* d_g, double Lc, int M, int64_t len, float* d_W_g, float* d_S, double* d_n,
                          double* d_hc, float* d_ws, int64_t ws_floats, int chunks, double* d_nws, int64_t nws_doubles,
                          const EvalFinalize* fin, hipStream_t st);
// the largest fs_aggregate_qffl_ws_doubles(M, len) over 1 <= M <= N
int64_t aggregate_qffl_ws_doubles_upto(int N, int64_t len);

// fs_aggregate_robust (aggregate_robust.hip) with an optional finaliser, as the five above (one launch
// at every M: the finaliser always rides)
int aggregate_robust_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len, int b,
                            float* d_out, const EvalFinalize* fin, hipStream_t st);

// fs_aggregate_krum (aggregate_krum.hip) with an optional finaliser, which rides on its gathered fold
int aggregate_krum_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                          const float* d_x, int f, int m, float* d_out, int32_t* d_pick, double* d_score, void* d_ws,
                          int64_t ws_bytes, float* d_agg_ws, int64_t agg_ws_floats, int chunks,
                          const EvalFinalize* fin, hipStream_t st);
int64_t aggregate_krum_ws_bytes(int M, int64_t len);

// fs_aggregate_rfa (aggregate_rfa.hip) with an optional finaliser, which rides on the chain's last
// step (d_alpha == nullptr: every row weighs ualpha)
int aggregate_rfa_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, int M, int64_t len,
                         const float* d_x, const float* d_alpha, float ualpha, int T, double nu, int init, float* d_out,
                         double* d_dist, float* d_b, double* d_obj, void* d_ws, int64_t ws_bytes,
                         const EvalFinalize* fin, hipStream_t st);
int64_t aggregate_rfa_ws_bytes(int M, int64_t len);

// fs_aggregate_topk (aggregate_topk.hip) with an optional finaliser, which rides on the thresholded fold
int aggregate_topk_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                          int64_t len, int64_t kcount, float* d_W_g, float* d_e, float* d_tau, int32_t* d_kept,
                          float* d_ws, int64_t ws_floats, int chunks, void* d_sws, int64_t sws_bytes,
                          const EvalFinalize* fin, hipStream_t st);
int64_t aggregate_topk_ws_bytes(int M, int64_t len);

// fs_aggregate_dp (aggregate_dp.hip) with an optional finaliser, which rides on the clipped fold
int aggregate_dp_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                        int64_t len, double S, double z, uint64_t seed, int t, int adaptive, double gamma, double eta,
                        double sigma_b, double* d_clip, int64_t cols_ld, int64_t cols_d, float* d_W_g, float* d_c,
                        double* d_r, double* d_state, float* d_ws, int64_t ws_floats, int chunks, void* d_sws,
                        int64_t sws_bytes, const EvalFinalize* fin, hipStream_t st);
int64_t aggregate_dp_ws_bytes(int M, int64_t len);

}  // namespace fs

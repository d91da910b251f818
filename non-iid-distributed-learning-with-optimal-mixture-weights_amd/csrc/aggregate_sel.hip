// fs_aggregate_sel -- the gathered fold: W_bar = q_0 * W[sel_0] + q_1 * W[sel_1] + ... over M
// sampled rows of the clients x params buffer, in k order, every product and every sum rounded
// separately (a round with partial client participation: the tools.py:345-350 left fold over
// the sampled clients in ascending client id).
//
// Contract: bitwise what fs_aggregate (aggregate.hip) returns on the compacted copy W[sel] with
// the same `chunks` -- both are rules of aggregate_fold.h, so the regimes, sub-ranges, chunks and
// stage-2 tree are the same code, and for M < 16 the reference's exact left fold.
//
// HBM-bound: M * len floats read plus the output written; rows outside sel are never touched
// (fs_aggregate with zero weights on them would read N * len and multiply stale rows by 0).
#include "aggregate_fold.h"
#include "aggregate_sel.h"

namespace fs {

// the term is q_k * W[sel_k] in fold_range_cond's groups of 8, nothing is read per position, the
// total is stored
struct SelRule {
  using Finish = StoreFinish;
  Finish f;
  const int32_t* sel;   // [M] row ids
  const float* q;       // [M]
  __device__ __forceinline__ Acc<1> fold(const float* __restrict__ base, int64_t stride, const Finish::Ctx&, int k0,
                                         int k1, bool) const {
    return {{fold_range_cond<true>(base, stride, sel, q, k0, k1)}};
  }
};

int aggregate_sel_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                         int64_t len, float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks,
                         const EvalFinalize* fin, hipStream_t st) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_sel && d_q && d_W_bar, "null pointer");
  return fold_dispatch(d_W_all, stride, SelRule{{d_W_bar}, d_sel, d_q}, M, len, d_ws, ws_floats, chunks, fin, st);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_sel(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int M,
                                int64_t len, float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks,
                                void* stream) {
  return aggregate_sel_launch(d_W_all, stride, d_sel, d_q, M, len, d_W_bar, d_ws, ws_floats, chunks, nullptr,
                              reinterpret_cast<hipStream_t>(stream));
}

// fs_aggregate_scaffold -- SCAFFOLD's server step: two folds over the M sampled rows of the
// clients x params buffer from ONE pass over those rows, both in place:
//
//   W_g <- fl(x + sum_k fl(q_k * fl(W[sel_k] - x)))                x = W_g before the call
//   c   <- fl(fl(cs * c) + sum_k fl(r_k * fl(x - W[sel_k])))
//
// in k order, every operation rounded separately.  A rule of aggregate_fold.h with two accumulators:
// the W_g fold is fs_aggregate_nova's mode 2 (aggregate_nova.hip) term for term, in the same load
// schedule, sub-ranges, chunks and stage-2 tree, the chunk clamp taken on half the workspace since
// every chunk keeps two partials -- so W_g is bitwise what mode 2 returns; the c fold has the same
// structure over its own terms: the first term of a range is the term itself, fl(cs * c) is added
// last.
//
// The identity behind the second fold: option II's c_i+ - c_i = -c + (x - W_i) / (K_i lr) needs no
// c_i, so with r_k = p_k / (K_k lr) and cs = 1 - sum_S p_k the server variate stays
// c = sum_j p_j c_j over ALL clients without reading the N x len variate buffer.
//
// Each row load feeds both accumulators.  (M + 2) * len floats read (+ len of x per further chunk
// or sub-range, cache hits) and 2 * len written, where two mode-2 launches read 2 (M + 1) * len.  No
// allocation.  Both outputs are updated in place: aggregate_fold.h's aliasing note.
#include "aggregate_fold.h"
#include "scaffold.h"

namespace fs {

#pragma clang fp contract(off)

// both terms of a row, from q_k and r_k
struct ScafTerm {
  static constexpr int NC = 2, SETS = 2;
  const float* coef[2];   // q [M], r [M]
  float4 x;
  __device__ __forceinline__ Acc<2> term(bool, const float (&cf)[2], float4 w) const {
    return {{scaled4(cf[0], sub4(w, x)), scaled4(cf[1], sub4(x, w))}};
  }
};

// every thread of a position reads x, the one that finishes also c, and stores x + delta and
// fl(cs * c) + delta.  No finaliser rides (aggregate_scaffold_launch takes none).
struct ScafFinish {
  static constexpr int SETS = 2;
  static constexpr bool RIDES = false;
  float cs;
  float *W_g, *c_g;
  struct Ctx {
    float4 x = zero4(), cv = zero4();
  };
  __device__ __forceinline__ Ctx load(int64_t i, bool fin) const {
    Ctx s;
    s.x = ld4(W_g + 4 * i);
    if (fin) s.cv = ld4(c_g + 4 * i);
    return s;
  }
  __device__ __forceinline__ void finish(int64_t i, const Ctx& s, const Acc<2>& t) const {
    st4(W_g + 4 * i, add4(s.x, t.a[0]));
    st4(c_g + 4 * i, add4(scaled4(cs, s.cv), t.a[1]));
  }
};

template <bool SEL>
struct ScafRule {
  using Finish = ScafFinish;
  Finish f;
  const int32_t* sel;   // [M] row ids (SEL), else rows 0..M-1
  const float *q, *r;   // [M]
  __device__ __forceinline__ Acc<2> fold(const float* __restrict__ W, int64_t stride, const Finish::Ctx& cx, int k0,
                                         int k1, bool) const {
    return fold_range_clamped<SEL>(W, stride, sel, ScafTerm{{q, r}, cx.x}, k0, k1);
  }
};

int aggregate_scaffold_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                              const float* d_r, float cs, int M, int64_t len, float* d_W_g, float* d_c, float* d_ws,
                              int64_t ws_floats, int chunks, hipStream_t st) {
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_q && d_r && d_W_g && d_c, "null pointer");
  FS_REQUIRE(d_W_g != d_c, "d_W_g and d_c must be different buffers");
  const ScafFinish f{cs, d_W_g, d_c};
  if (d_sel)
    return fold_dispatch(d_W_all, stride, ScafRule<true>{f, d_sel, d_q, d_r}, M, len, d_ws, ws_floats, chunks, nullptr, st);
  return fold_dispatch(d_W_all, stride, ScafRule<false>{f, d_sel, d_q, d_r}, M, len, d_ws, ws_floats, chunks, nullptr, st);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_scaffold(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                                     const float* d_r, float cs, int M, int64_t len, float* d_W_g, float* d_c,
                                     float* d_ws, int64_t ws_floats, int chunks, void* stream) {
  return aggregate_scaffold_launch(d_W_all, stride, d_sel, d_q, d_r, cs, M, len, d_W_g, d_c, d_ws, ws_floats, chunks,
                                   reinterpret_cast<hipStream_t>(stream));
}

// fs_aggregate_nova -- FedNova's scaled fold over M rows of the clients x params buffer, in k
// order, every operation rounded separately.  The one aggregation rule of the reference that is
// not a plain sum_k q_k W_k (tools.py:383-410), in two forms:
//
//   mode 1 (FS_NOVA_REFERENCE)  the reference's own lines (tools.py:401-405), which scale the
//       clients' WEIGHTS:  W_bar = fl(W[sel_0] * s0) + sum_{k>=1} fl(fl(fl(q_k * W[sel_k]) * te) / b_k)
//       -- s0 belongs to the fold's global first row only; the division is the correctly rounded
//       IEEE quotient (hipcc's default float `/`; a multiplication by 1/b differs in the last bit).
//   mode 2 (FS_NOVA_UPDATES)    Wang et al.'s normalised averaging of the clients' UPDATES:
//       W_bar = fl(base + sum_k fl(q_k * fl(W[sel_k] - base))).
//
// Two rules of aggregate_fold.h, on its clamped groups of 8: the first term of any range of k is the
// term itself, not 0 + term; regimes, sub-ranges, chunks and the stage-2 tree are fs_aggregate's,
// chosen by M: for M < 16 or chunks == 1 the exact left fold.  M * len floats read (+ len of base in
// mode 2, per chunk or sub-range) and len written; rows outside sel never touched.  No allocation.
// In mode 2 base may be W_bar (the round plan's d_W_g): aggregate_fold.h's aliasing note.
#include "aggregate_fold.h"
#include "aggregate_sel.h"

namespace fs {

#pragma clang fp contract(off)

// mode 1's term, from q_k and b_k: fl(W * s0) for the fold's global first row, else
// fl(fl(fl(q_k * W) * te) / b_k)
struct NovaRefTerm {
  static constexpr int NC = 2, SETS = 1;
  const float* coef[2];   // q [M], b [M]
  float te, s0;
  __device__ __forceinline__ Acc<1> term(bool first, const float (&cf)[2], float4 w) const {
    const float q = cf[0], b = cf[1];
    if (first) return {{make_float4(w.x * s0, w.y * s0, w.z * s0, w.w * s0)}};
    return {{make_float4(((q * w.x) * te) / b, ((q * w.y) * te) / b, ((q * w.z) * te) / b, ((q * w.w) * te) / b)}};
  }
};

template <bool SEL>
struct NovaRefRule {
  using Finish = StoreFinish;
  Finish f;
  const int32_t* sel;   // [M] row ids (SEL), else rows 0..M-1
  NovaRefTerm t;
  __device__ __forceinline__ Acc<1> fold(const float* __restrict__ W, int64_t stride, const Finish::Ctx&, int k0, int k1,
                                         bool) const {
    return fold_range_clamped<SEL>(W, stride, sel, t, k0, k1);
  }
};

// mode 2: every thread of a position reads its base, the one that finishes stores base + delta
struct BaseFinish {
  static constexpr int SETS = 1;
  static constexpr bool RIDES = true;
  const float* base;
  float* out;
  struct Ctx {
    float4 bs = zero4();
  };
  __device__ __forceinline__ Ctx load(int64_t i, bool) const { return {ld4(base + 4 * i)}; }
  __device__ __forceinline__ void finish(int64_t i, const Ctx& cx, const Acc<1>& t) const {
    st4(out + 4 * i, add4(cx.bs, t.a[0]));
  }
};

template <bool SEL>
struct NovaUpdRule {
  using Finish = BaseFinish;
  Finish f;
  const int32_t* sel;
  const float* q;       // [M]
  __device__ __forceinline__ Acc<1> fold(const float* __restrict__ W, int64_t stride, const Finish::Ctx& cx, int k0,
                                         int k1, bool) const {
    return fold_range_clamped<SEL>(W, stride, sel, UpdateTerm{{q}, cx.bs}, k0, k1);
  }
};

int aggregate_nova_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                          const float* d_b, float te, float s0, int mode, const float* d_W_base, int M, int64_t len,
                          float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks, const EvalFinalize* fin,
                          hipStream_t st) {
  FS_REQUIRE(mode == FS_NOVA_REFERENCE || mode == FS_NOVA_UPDATES, "mode must be FS_NOVA_REFERENCE or FS_NOVA_UPDATES");
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_q && d_W_bar, "null pointer");
  FS_REQUIRE(mode != FS_NOVA_REFERENCE || d_b, "mode 1 needs d_b");
  FS_REQUIRE(mode != FS_NOVA_UPDATES || d_W_base, "mode 2 needs d_W_base");
#define FS_NOVA_GO(...) return fold_dispatch(d_W_all, stride, __VA_ARGS__, M, len, d_ws, ws_floats, chunks, fin, st)
  if (mode == FS_NOVA_REFERENCE) {
    const NovaRefTerm t{{d_q, d_b}, te, s0};
    if (d_sel) FS_NOVA_GO(NovaRefRule<true>{{d_W_bar}, d_sel, t});
    FS_NOVA_GO(NovaRefRule<false>{{d_W_bar}, d_sel, t});
  }
  if (d_sel) FS_NOVA_GO(NovaUpdRule<true>{{d_W_base, d_W_bar}, d_sel, d_q});
  FS_NOVA_GO(NovaUpdRule<false>{{d_W_base, d_W_bar}, d_sel, d_q});
#undef FS_NOVA_GO
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_nova(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q,
                                 const float* d_b, float te, float s0, int mode, const float* d_W_base, int M,
                                 int64_t len, float* d_W_bar, float* d_ws, int64_t ws_floats, int chunks,
                                 void* stream) {
  return aggregate_nova_launch(d_W_all, stride, d_sel, d_q, d_b, te, s0, mode, d_W_base, M, len, d_W_bar, d_ws,
                               ws_floats, chunks, nullptr, reinterpret_cast<hipStream_t>(stream));
}

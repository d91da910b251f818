// fs_aggregate_opt -- the FedOpt server step (Reddi et al., ICLR 2021, Algorithm 2; FedAvgM, Hsu et
// al. 2019): the fold of the M sampled clients' updates with an element-wise optimizer step fused
// onto its end, all three state buffers in place.  With x = W_g, m, v on entry:
//
//   delta = sum_k fl(q_k * fl(W[sel_k] - x))                     (k ascending)
//   AVGM     m' = fl(fl(beta1*m) + delta)                         x' = fl(x + fl(eta*m'))
//   others   m' = fl(fl(beta1*m) + fl(omb1*delta)),  d2 = fl(delta*delta)
//     ADAGRAD  v' = fl(v + d2)
//     ADAM     v' = fl(fl(beta2*v) + fl(omb2*d2))
//     YOGI     v' = fl(v - fl(fl(omb2*d2) * s)),  s = sgn(fl(v - d2))
//            x' = fl(x + fl(fl(eta*m') / fl(sqrtf(v') + tau)))
//
// every operation rounded separately, the quotient and the square root the correctly rounded IEEE
// ones, no bias correction (as the paper).  A rule of aggregate_fold.h: the fold is
// fs_aggregate_nova's mode 2 (aggregate_nova.hip) before it adds its base -- the same term, load
// schedule, sub-ranges, chunks (one partial per chunk: the clamp sees the whole workspace) and
// stage-2 tree -- so AVGM with beta1 = 0, eta = 1 is bitwise mode 2.
//
// The finish runs once per element, in the thread that writes the position -- some 30 VALU
// operations per element against M row loads, off the stream's critical path.  (M + 3) * len floats
// read and 3 * len written (AVGM: M + 2 and 2; + len of x per further chunk or sub-range, cache
// hits).  No allocation.  All three buffers are updated in place: aggregate_fold.h's aliasing note.
#include "aggregate_fold.h"
#include "aggregate_sel.h"

namespace fs {

#pragma clang fp contract(off)

// the server step's scalars; the rule is uniform over the launch
struct OptStep {
  int rule;
  float eta, beta1, omb1, beta2, omb2, tau;
};

// the server step at one element.  YOGI's sign is a select (a NaN difference selects 0).
__device__ __forceinline__ void opt_step1(const OptStep& p, float d, float& x, float& m, float& v) {
  if (p.rule == FS_OPT_AVGM) {
    m = p.beta1 * m + d;
    x = x + p.eta * m;
    return;
  }
  const float d2 = d * d;
  m = p.beta1 * m + p.omb1 * d;
  if (p.rule == FS_OPT_ADAGRAD) {
    v = v + d2;
  } else if (p.rule == FS_OPT_ADAM) {
    v = p.beta2 * v + p.omb2 * d2;
  } else {
    const float t = v - d2;
    const float s = t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f);
    v = v - (p.omb2 * d2) * s;
  }
  x = x + (p.eta * m) / (sqrtf(v) + p.tau);
}

// every thread of a position reads x, the one that finishes also m and v (v only where the rule has
// one: AVGM's d_v may be NULL), steps and stores all three
struct OptFinish {
  static constexpr int SETS = 1;
  static constexpr bool RIDES = true;
  OptStep p;
  float *W_g, *m_g, *v_g;
  struct Ctx {
    float4 x = zero4(), m = zero4(), v = zero4();
  };
  __device__ __forceinline__ Ctx load(int64_t i, bool fin) const {
    Ctx s;
    s.x = ld4(W_g + 4 * i);
    if (fin) {
      s.m = ld4(m_g + 4 * i);
      if (p.rule != FS_OPT_AVGM) s.v = ld4(v_g + 4 * i);
    }
    return s;
  }
  __device__ __forceinline__ void finish(int64_t i, Ctx s, const Acc<1>& t) const {
    const float4 d = t.a[0];
    opt_step1(p, d.x, s.x.x, s.m.x, s.v.x);
    opt_step1(p, d.y, s.x.y, s.m.y, s.v.y);
    opt_step1(p, d.z, s.x.z, s.m.z, s.v.z);
    opt_step1(p, d.w, s.x.w, s.m.w, s.v.w);
    st4(W_g + 4 * i, s.x);
    st4(m_g + 4 * i, s.m);
    if (p.rule != FS_OPT_AVGM) st4(v_g + 4 * i, s.v);
  }
};

template <bool SEL>
struct OptRule {
  using Finish = OptFinish;
  Finish f;
  const int32_t* sel;   // [M] row ids (SEL), else rows 0..M-1
  const float* q;       // [M]
  __device__ __forceinline__ Acc<1> fold(const float* __restrict__ W, int64_t stride, const Finish::Ctx& cx, int k0,
                                         int k1, bool) const {
    return fold_range_clamped<SEL>(W, stride, sel, UpdateTerm{{q}, cx.x}, k0, k1);
  }
};

int aggregate_opt_launch(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int rule,
                         float eta, float beta1, float omb1, float beta2, float omb2, float tau, int M, int64_t len,
                         float* d_W_g, float* d_m, float* d_v, float* d_ws, int64_t ws_floats, int chunks,
                         const EvalFinalize* fin, hipStream_t st) {
  FS_REQUIRE(rule >= FS_OPT_AVGM && rule <= FS_OPT_YOGI, "rule must be FS_OPT_AVGM, _ADAGRAD, _ADAM or _YOGI");
  FS_REQUIRE(M >= 1, "M must be >= 1");
  FS_REQUIRE(len >= 4 && len % 4 == 0 && stride % 4 == 0 && stride >= len, "len/stride must be multiples of 4");
  FS_REQUIRE(d_W_all && d_q && d_W_g && d_m, "null pointer");
  FS_REQUIRE(rule == FS_OPT_AVGM || d_v, "the rule needs d_v");
  FS_REQUIRE(rule == FS_OPT_AVGM || tau > 0.f, "tau must be > 0");
  FS_REQUIRE(d_W_g != d_m && (!d_v || (d_v != d_W_g && d_v != d_m)), "d_W_g, d_m and d_v must be different buffers");
  const OptFinish f{{rule, eta, beta1, omb1, beta2, omb2, tau}, d_W_g, d_m, d_v};
  if (d_sel) return fold_dispatch(d_W_all, stride, OptRule<true>{f, d_sel, d_q}, M, len, d_ws, ws_floats, chunks, fin, st);
  return fold_dispatch(d_W_all, stride, OptRule<false>{f, d_sel, d_q}, M, len, d_ws, ws_floats, chunks, fin, st);
}

}  // namespace fs

using namespace fs;

extern "C" int fs_aggregate_opt(const float* d_W_all, int64_t stride, const int32_t* d_sel, const float* d_q, int rule,
                                float eta, float beta1, float omb1, float beta2, float omb2, float tau, int M,
                                int64_t len, float* d_W_g, float* d_m, float* d_v, float* d_ws, int64_t ws_floats,
                                int chunks, void* stream) {
  return aggregate_opt_launch(d_W_all, stride, d_sel, d_q, rule, eta, beta1, omb1, beta2, omb2, tau, M, len, d_W_g, d_m,
                              d_v, d_ws, ws_floats, chunks, nullptr, reinterpret_cast<hipStream_t>(stream));
}

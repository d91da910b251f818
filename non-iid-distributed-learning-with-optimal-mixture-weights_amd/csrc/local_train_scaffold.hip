// fs_local_train_scaffold -- SCAFFOLD's local training (Karimireddy et al., ICML 2020, option II):
// per-client local SGD for the whole round, fused in one launch, with the control-variate
// correction in every step and the client's new variate left behind.
//
// The single form of local_train.hip (one 512-thread workgroup per client, the same tiling
// RT in {1, 2, 4} x CT in {1, 2}, the same W-in-LDS rule, the same fixed-order sums and the same
// lane <-> element ownership), parallel clients and cross-entropy only, without the prox term.
// What it adds:
//   update    grad = fl(grad_CE + d), d = fl(c - c_i) fixed for the whole client, then the ridge
//             term and W -= lr * grad as in local_train.hip.  d is not kept: the lane re-reads its
//             own elements of c and c_i (L2-resident: 2 * C * ld * 4 bytes per step beside the
//             B * ld * 4 of the batch) -- two 16-byte loads per class row and quarter tile.
//   epilogue  in the pass that copies W out of LDS (or, W in L2, a pass of its own):
//             c_i <- fl(fl(c_i - c) + fl(fl(x - y) * inv)),  inv = 1.0f / fl((float)K_i * lr),
//             x = W_start, y = the trained weights, K_i = E * ceil(n_i / B) -- every operation
//             rounded separately.  The lane that owns W[c][d] owns c_i[c][d]: in place, no hand-off.
// With c = c_i = 0 the steps are bitwise local_train.hip's single form (grad + 0).
// A client with no steps returns W_start, loss 0 and leaves c_i alone.
#include "common.h"
#include "scaffold.h"

namespace fs {

constexpr int SC_WAVES = 8;
constexpr int SC_THREADS = SC_WAVES * kWave;

constexpr int SC_CHUNK = 2048;   // batch rows whose (row, label) are staged in LDS at once

template <int RT, int CT>
struct SCShared {
  int erow[SC_CHUNK];                 // global feature row of each staged batch position
  int elab[SC_CHUNK];                 // its label
  float zpart[SC_WAVES][RT * 16][CT * 16];
  float g[RT * 16][CT * 16];
  float red[2][SC_WAVES][2];
  float cep[2][SC_WAVES];
  float pro[SC_WAVES];
  float pad_[2];                      // keep sizeof a multiple of 16 B: the dynamic W image follows
};

__device__ __forceinline__ float4 sc_mask4(float4 v, bool keep) {
  return keep ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int W>
__device__ __forceinline__ float sc_group_max(float v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

template <int W>
__device__ __forceinline__ float sc_group_sum(float v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// option II's new variate of four elements, every operation rounded separately (no fma)
__device__ __forceinline__ float4 sc_variate(float4 ci, float4 c, float4 x, float4 y, float inv) {
#pragma clang fp contract(off)
  return make_float4((ci.x - c.x) + ((x.x - y.x) * inv), (ci.y - c.y) + ((x.y - y.y) * inv),
                     (ci.z - c.z) + ((x.z - y.z) * inv), (ci.w - c.w) + ((x.w - y.w) * inv));
}

// WLDS: the client's weights live in LDS for the whole local training (row stride ld + 4
// floats), as in local_train.hip; otherwise they stay in the (L2-resident) output buffer.
template <int RT, int CT, bool WLDS>
__global__ __launch_bounds__(SC_THREADS) void local_train_scaffold_kernel(LTSParams P) {
  __shared__ SCShared<RT, CT> sh;
  extern __shared__ __attribute__((aligned(16))) float sW[];   // [C][ld + 4] when WLDS
  constexpr int NC = CT * 16;           // padded classes
  constexpr int NZ = RT * 16 * NC;      // padded logits per step
  constexpr int UF = (RT * CT >= 4) ? 1 : 2;   // forward tiles per batch of loads (register budget)
  constexpr int UB = (RT >= 4) ? 1 : 2;        // backward tiles per batch of loads
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int l16 = lane & 15;
  const int lg = lane >> 4;
  const int64_t ld = P.ld;
  const int NT = (int)(ld >> 6);
  const int C = P.C;
  const int B = P.B;
  const int E = P.E;
  const int CH = (SC_CHUNK / B) * B;
  const int64_t LDW = ld + 4;
  int it = 0;  // step counter (parity of the double-buffered LDS slots)

  const int j = P.order ? P.order[blockIdx.x] : (int)blockIdx.x;
  const int64_t row0 = P.row_off[j];
  const int n = (int)(P.row_off[j + 1] - row0);
  const float* start = P.W_start;
  const float* cg = P.c;
  float* cij = P.ci + (int64_t)j * C * ld;
  float* Wj = P.W_out + (int64_t)j * C * ld;
  const int nb = (n + B - 1) / B;
  const int steps = E * nb;

  if (steps == 0) {
    for (int T = w; T < NT; T += SC_WAVES)
      for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 16 + l16;
        if (c < C)
          for (int q = 0; q < 4; ++q) {
            const int64_t off = c * ld + 64 * T + 16 * lg + 4 * q;
            st4(Wj + off, ld4(start + off));
          }
      }
    if (tid == 0) P.loss[j] = 0.0;
    return;
  }

  // ||W_start||^2 for the ridge term of the first step
  float wn2 = 0.f;
  if (P.reg) {
    float acc = 0.f;
    for (int T = w; T < NT; T += SC_WAVES)
      for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 16 + l16;
        if (c < C)
          for (int q = 0; q < 4; ++q) {
            const float4 v = ld4(start + c * ld + 64 * T + 16 * lg + 4 * q);
            acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
          }
      }
    acc = wave_sum(acc);
    if (lane == 0) sh.pro[w] = acc;
    __syncthreads();
    for (int i = 0; i < SC_WAVES; ++i) wn2 += sh.pro[i];
  }

  const float* src = start;
  if (WLDS) {
    // lane-owned copy: every lane later reads and writes exactly these elements
    for (int T = w; T < NT; T += SC_WAVES)
      for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 16 + l16;
        if (c < C)
          for (int q = 0; q < 4; ++q) {
            const int64_t off = 64 * T + 16 * lg + 4 * q;
            st4(sW + c * LDW + off, ld4(start + c * ld + off));
          }
      }
  }
  double lsum = 0.0;
  for (int e = 0; e < E; ++e) {
    for (int s = 0; s < nb; ++s, ++it) {
      const int par = it & 1;
      const int b0 = s * B;
      const int bc = min(B, n - b0);
      const int cb = b0 % CH;           // position of this batch inside the staged chunk
      if (cb == 0) {
        // stage the next CH shuffled rows of this epoch: (global row, label) into LDS
        __syncthreads();                // every wave is done with the previous chunk
        const int cn = min(CH, n - b0);
        const int32_t* pp = P.perms + (int64_t)E * row0 + (int64_t)e * n + b0;
        for (int i = tid; i < cn; i += SC_THREADS) {
          const int li = pp[i];
          sh.erow[i] = (int)(row0 + li);
          sh.elab[i] = P.labels[row0 + li];
        }
        __syncthreads();
      }

      // ---------------- forward: z = X_b W^T ----------------
      // invalid rows (>= bc) read a valid row and are zeroed after the load, so every
      // load is unconditional and the compiler can keep them all in flight.
      const float* xr[RT];
      bool xok[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int r = rt * 16 + l16;
        xok[rt] = r < bc;
        xr[rt] = P.phi + (int64_t)sh.erow[cb + (xok[rt] ? r : 0)] * ld;
      }
      floatx4 acc[RT][CT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = floatx4{0.f, 0.f, 0.f, 0.f};

      // UF tiles per iteration: all UF x 4 x (RT + CT) 16-byte loads are issued before the MFMAs
      for (int T0 = w; T0 < NT; T0 += UF * SC_WAVES) {
        const bool ok1 = UF > 1 && T0 + SC_WAVES < NT;
        const int T1 = ok1 ? T0 + SC_WAVES : T0;
        float4 xv[UF][4][RT], wv[UF][4][CT];
#pragma unroll
        for (int h = 0; h < UF; ++h) {
          const int64_t dof = 64 * (h ? T1 : T0) + 16 * lg;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) xv[h][q][rt] = ld4(xr[rt] + dof + 4 * q);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              const int c = min(ct * 16 + l16, C - 1);
              wv[h][q][ct] = WLDS ? ld4(sW + c * LDW + dof + 4 * q) : ld4(src + c * ld + dof + 4 * q);
            }
          }
        }
#pragma unroll
        for (int h = 0; h < UF; ++h) {
          if (h == 1 && !ok1) break;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) xv[h][q][rt] = sc_mask4(xv[h][q][rt], xok[rt]);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) wv[h][q][ct] = sc_mask4(wv[h][q][ct], ct * 16 + l16 < C);
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4)
#pragma unroll
              for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                  acc[rt][ct] = mfma4(comp(xv[h][q][rt], e4), comp(wv[h][q][ct], e4), acc[rt][ct]);
          }
        }
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int i = 0; i < 4; ++i) sh.zpart[w][rt * 16 + 4 * lg + i][ct * 16 + l16] = acc[rt][ct][i];
      __syncthreads();  // B1: partial logits of all waves; previous step's norm partials

      if (s > 0 || e > 0) {
        wn2 = 0.f;
#pragma unroll
        for (int i = 0; i < SC_WAVES; ++i) wn2 += sh.red[par ^ 1][i][1];
      }

      // ------- logits (fixed-order sum of the wave partials) + softmax / CE, one logit per thread -------
      {
        const float invb = 1.0f / (float)bc;
        float cep = 0.f;
        for (int idx = tid; idx < NZ; idx += SC_THREADS) {   // NC lanes of one wave hold one row
          const int r = idx / NC, c = idx % NC;
          float z = 0.f;
#pragma unroll
          for (int i = 0; i < SC_WAVES; ++i) z += sh.zpart[i][r][c];
          const bool valid = r < bc && c < C;
          const float m = sc_group_max<NC>(valid ? z : -INFINITY);
          const float se = sc_group_sum<NC>(valid ? expf(z - m) : 0.f);
          float gv = 0.f;
          if (valid) {
            const float lp = z - m - logf(se);               // log_softmax
            const bool isy = c == sh.elab[cb + r];
            gv = (isy ? -invb : 0.f) + expf(lp) * invb;      // d CE_mean / d z
            if (isy) cep -= lp;
          }
          sh.g[r][c] = gv;
        }
        cep = wave_sum(cep);
        if (lane == 0) sh.cep[par][w] = cep;
      }
      __syncthreads();  // B2: g and the CE partials visible

      if (tid == 0 && e == E - 1) {
        float ce = 0.f;
        for (int i = 0; i < SC_WAVES; ++i) ce += sh.cep[par][i];
        float loss = ce / (float)bc;                       // CrossEntropyLoss, mean
        if (P.reg) loss = loss + P.lam * sqrtf(wn2);       // + lambda * ||W||_F (the correction is no part of the loss)
        lsum += (double)loss * (double)bc;                 // Meter.update(loss.item(), |b|)
      }

      // ---------------- backward + fused SGD/variate/ridge update ----------------
      float gB[4 * RT][CT];
      const float* xk[4 * RT];
      bool kok[4 * RT];
#pragma unroll
      for (int kk = 0; kk < 4 * RT; ++kk) {
        const int r = 4 * kk + lg;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) gB[kk][ct] = sh.g[r][ct * 16 + l16];
        kok[kk] = r < bc;
        xk[kk] = P.phi + (int64_t)sh.erow[cb + (kok[kk] ? r : 0)] * ld + 4 * l16;
      }
      const float sr = (P.reg && wn2 > 0.f) ? P.lam / sqrtf(wn2) : 0.f;
      const float lr = P.lr;
      float nwn = 0.f;
      for (int T0 = w; T0 < NT; T0 += UB * SC_WAVES) {
        const bool ok1 = UB > 1 && T0 + SC_WAVES < NT;
        const int T1 = ok1 ? T0 + SC_WAVES : T0;
        float4 xv[UB][4 * RT];
#pragma unroll
        for (int h = 0; h < UB; ++h)
#pragma unroll
          for (int kk = 0; kk < 4 * RT; ++kk) xv[h][kk] = ld4(xk[kk] + 64 * (h ? T1 : T0));
#pragma unroll
        for (int h = 0; h < UB; ++h) {
          if (h == 1 && !ok1) break;
          const int T = h ? T1 : T0;
          floatx4 ga[CT][4];
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) ga[ct][e4] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < 4 * RT; ++kk) {
            const float4 x = sc_mask4(xv[h][kk], kok[kk]);
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4)
#pragma unroll
              for (int ct = 0; ct < CT; ++ct) ga[ct][e4] = mfma4(comp(x, e4), gB[kk][ct], ga[ct][e4]);
          }
          // ga[ct][e][q] = grad[c = ct*16 + l16][d = 64T + 16 lg + 4q + e]
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const int c = ct * 16 + l16;
            if (c < C) {
              float4 wv[4], cv[4], iv[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int64_t off = c * ld + 64 * T + 16 * lg + 4 * q;
                wv[q] = WLDS ? ld4(sW + (off - c * ld) + c * LDW) : ld4(src + off);
                cv[q] = ld4(cg + off);
                iv[q] = ld4(cij + off);
              }
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int64_t off = c * ld + 64 * T + 16 * lg + 4 * q;
                float o[4];
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4) {
                  const float wc = comp(wv[q], e4);
                  const float dv = comp(cv[q], e4) - comp(iv[q], e4);   // d = fl(c - c_i)
                  float gr = ga[ct][e4][q] + dv;                        // fl(grad_CE + d)
                  // the three fused multiply-adds local_train.hip's update compiles to, spelled
                  // out: left to the compiler's contraction the norm's o * o stayed unfused here,
                  // one ulp away from the single form's ||W||^2 every few hundred steps
                  if (P.reg) gr = __builtin_fmaf(wc, sr, gr);
                  o[e4] = __builtin_fmaf(-lr, gr, wc);
                  nwn = __builtin_fmaf(o[e4], o[e4], nwn);
                }
                if (WLDS) st4(sW + (off - c * ld) + c * LDW, make_float4(o[0], o[1], o[2], o[3]));
                else st4(Wj + off, make_float4(o[0], o[1], o[2], o[3]));
              }
            }
          }
        }
      }
      nwn = wave_sum(nwn);
      if (lane == 0) sh.red[par][w][1] = nwn;
      src = Wj;
    }
  }
  // W out of LDS, and the client's new variate from x = W_start and y = the trained weights: each
  // lane its own elements (the ones it updated above, so its own stores to Wj are what it reads)
  {
    const float inv = 1.0f / ((float)steps * P.lr);
    for (int T = w; T < NT; T += SC_WAVES)
      for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 16 + l16;
        if (c < C)
          for (int q = 0; q < 4; ++q) {
            const int64_t off = 64 * T + 16 * lg + 4 * q;
            const float4 y = WLDS ? ld4(sW + c * LDW + off) : ld4(Wj + c * ld + off);
            if (WLDS) st4(Wj + c * ld + off, y);
            st4(cij + c * ld + off,
                sc_variate(ld4(cij + c * ld + off), ld4(cg + c * ld + off), ld4(start + c * ld + off), y, inv));
          }
      }
  }
  if (tid == 0) P.loss[j] = lsum / (double)n;
}

template <int RT, int CT>
static int launch_sc(const LTSParams& P, hipStream_t st) {
  const size_t wbytes = sizeof(float) * (size_t)P.C * (size_t)(P.ld + 4);
  const size_t budget = 160 * 1024 - sizeof(SCShared<RT, CT>);
  if (wbytes <= budget) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&local_train_scaffold_kernel<RT, CT, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)wbytes);
    if (e != hipSuccess) return fail(FS_EHIP, std::string("fs_local_train_scaffold: ") + hipGetErrorString(e));
    hipLaunchKernelGGL((local_train_scaffold_kernel<RT, CT, true>), dim3(P.N), dim3(SC_THREADS), wbytes, st, P);
  } else {
    hipLaunchKernelGGL((local_train_scaffold_kernel<RT, CT, false>), dim3(P.N), dim3(SC_THREADS), 0, st, P);
  }
  return FS_OK;
}

// one workgroup per client; fs_local_train_scaffold's validation is in local_train_host.cpp
int launch_local_train_scaffold(const LTSParams& P, hipStream_t st) {
  const int RT = P.B <= 16 ? 1 : (P.B <= 32 ? 2 : 4);
  const int CT = P.C <= 16 ? 1 : 2;
  if (RT == 1 && CT == 1) return launch_sc<1, 1>(P, st);
  if (RT == 2 && CT == 1) return launch_sc<2, 1>(P, st);
  if (RT == 4 && CT == 1) return launch_sc<4, 1>(P, st);
  if (RT == 1 && CT == 2) return launch_sc<1, 2>(P, st);
  if (RT == 2 && CT == 2) return launch_sc<2, 2>(P, st);
  return launch_sc<4, 2>(P, st);
}

}  // namespace fs

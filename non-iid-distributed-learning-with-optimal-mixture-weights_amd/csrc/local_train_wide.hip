// fs_local_train, the wide form (FS_G_WIDE, FS_LT_WIDE): one workgroup per client as in
// local_train.hip, with the batch walked in 64-row blocks, so a step takes any batch size.
//
// A step of bc = min(B, rows left) rows, the weights W held fixed until its end:
//   pass 1    per 64-row block: forward z = X_blk W^T (v_mfma_f32_16x16x4_f32, the 64-column
//             tiles dealt round-robin to the 8 waves), the fixed-order sum of the 8 waves'
//             partial logits through LDS, softmax, g = (softmax - onehot) / bc -- the whole
//             batch's bc -- stored to this workgroup's workspace slot [row][class] with plain
//             vector stores; the CE partials accumulate per thread in block order.  The partial
//             logits are double-buffered (C <= 16), so a block costs one barrier and a wave
//             runs its next block's forward beside the others' softmax.
//   pass 2    per group of TG of the wave's tiles: grad^T = X_b^T g accumulated in registers
//             over ALL blocks (16 CT VGPRs per tile; the block's g read once per group, the
//             rows re-read, L2-resident by now), then the fused SGD / prox / ridge update and
//             the two squared norms for the next step, once per batch.  No barrier inside a
//             pass 2 whose batch fits one staged chunk.
// Rows are read once from HBM (pass 1) and once more (pass 2: every tile group reads its own
// columns), whatever the width; g goes through the L2-resident slot, 1/4 (C <= 16) of the
// bytes of a row tile.
// One pass (a wave holds the gradient of ALL its tiles: one tile group, ld <= 2048 at C <= 16,
// ld <= 1024 above): g depends on its own block and on bc alone, so block k - 1's gradient is
// accumulated right after block k's softmax, from g in LDS (two buffers), one block after its
// rows were streamed -- the two passes above re-read a whole batch -- and the slot is not
// touched.  A block then costs one barrier (two above 16 classes), the update still runs once
// per batch.  (Accumulating block k's own gradient right after its softmax, behind a second
// barrier, keeps the re-read one block closer, but that instance spills: 24 to 112 bytes per
// lane of scratch, so it is not shipped.)
// Lane <-> element ownership as in local_train.hip: the lane that produces grad[c][d] is the
// lane that reads W[c][d] as the forward's B operand, so chained clients need no hand-off.
// (row, label) of the batch are staged in LDS by chunks of WD_CHUNK rows of the batch, for any B.
// No cross-workgroup wait: a workgroup reads and writes its own slot only.
#include <type_traits>

#include "common.h"
#include "local_train_wide.h"

namespace fs {

constexpr int WD_THREADS = WD_WAVES * kWave;
constexpr int WD_CHUNK = 512;                     // batch rows whose (row, label) are staged in LDS at once
constexpr int WD_CBLK = WD_CHUNK / WD_BLOCK;      // blocks per staged chunk
constexpr int WD_RT = WD_BLOCK / 16;              // 16-row tiles per block

template <int CT>
struct WDShared {
  int erow[WD_CHUNK];                 // global feature row of each staged batch position
  int elab[WD_CHUNK];                 // its label
  float zpart[2 / CT][WD_WAVES][WD_BLOCK][CT * 16];   // 64 KB: two blocks' partials at C <= 16, one above
  float g[2][WD_BLOCK][CT * 16];      // one pass: d CE / d z of this block and of the one before
  float red[WD_WAVES][2];
  float cep[WD_WAVES];
  float pro[WD_WAVES];                // (sizeof stays a multiple of 16 B: the dynamic W image follows)
};

__device__ __forceinline__ float4 wd_mask4(float4 v, bool keep) {
  return keep ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int W>
__device__ __forceinline__ float wd_group_max(float v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

template <int W>
__device__ __forceinline__ float wd_group_sum(float v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// WLDS: the client's weights live in LDS for the whole local training (row stride ld + 4
// floats), else in the (L2-resident) output buffer -- as in local_train.hip.
// OP: the one-pass instance (every wave's tiles are one tile group).
template <int CT, bool WLDS, bool OP>
__global__ __launch_bounds__(WD_THREADS) void local_train_wide_kernel(LTParams P, WideWS X) {
  __shared__ WDShared<CT> sh;
  extern __shared__ __attribute__((aligned(16))) float sW[];   // [C][ld + 4] when WLDS
  constexpr int NC = CT * 16;           // padded classes
  constexpr int NZ = WD_BLOCK * NC;     // padded logits per block
  constexpr int ZB = 2 / CT;            // partial-logit buffers
  constexpr int TG = 4 / CT;            // tiles whose gradient a wave holds at once (16 CT VGPRs each)
  constexpr int RT = WD_RT;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int l16 = lane & 15;
  const int lg = lane >> 4;
  const int64_t ld = P.ld;
  const int NT = (int)(ld >> 6);
  const int C = P.C;
  const int E = P.E;
  const int ngrp = ((NT + WD_WAVES - 1) / WD_WAVES + TG - 1) / TG;   // tile groups of the busiest wave (uniform)
  constexpr bool onepass = OP;          // a wave holds the gradient of all its tiles: ld <= 2048 (C <= 16), 1024 above
  const int64_t LDW = ld + 4;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float* gws = X.g + (int64_t)blockIdx.x * X.slot_floats;
  const int nwalk = P.chained ? P.N : (P.N - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;

  for (int k = 0; k < nwalk; ++k) {
    const int ci = P.chained ? k : (int)blockIdx.x + k * (int)gridDim.x;
    const int j = P.chained ? k : (P.order ? P.order[ci] : ci);
    const int64_t row0 = P.row_off[j];
    const int n = (int)(P.row_off[j + 1] - row0);
    const float* start = (P.chained && j > 0) ? P.W_out + (int64_t)(j - 1) * C * ld : P.W_start;
    const float* anchor = start;  // global_model = deepcopy(model)  (tools.py:180)
    float* Wj = P.W_out + (int64_t)j * C * ld;
    const int B = min(P.B, max(n, 1));              // the effective batch: min(B, n_j)
    const int nb = (n + B - 1) / B;
    const int steps = E * nb;
    // a client whose batch the slot was not planned for (a workspace from another plan) is not
    // trained: its start comes back with a NaN loss, and nothing is written outside the slot
    const bool fits = wd_slot_rows(B) <= (int64_t)X.slot_rows;

    if (steps == 0 || !fits) {
      for (int T = w; T < NT; T += WD_WAVES)
        for (int ct = 0; ct < CT; ++ct) {
          const int c = ct * 16 + l16;
          if (c < C)
            for (int q = 0; q < 4; ++q) {
              const int64_t off = c * ld + 64 * T + 16 * lg + 4 * q;
              st4(Wj + off, ld4(start + off));
            }
        }
      if (tid == 0) P.loss[j] = steps == 0 ? 0.0 : (double)NAN;
      __syncthreads();
      continue;
    }

    // ||W_start||^2 for the ridge term of the first step (the prox norm starts at 0).
    float wn2 = 0.f, pn2 = 0.f;
    if (P.reg) {
      float acc = 0.f;
      for (int T = w; T < NT; T += WD_WAVES)
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
      for (int i = 0; i < WD_WAVES; ++i) wn2 += sh.pro[i];
    }

    const float* src = start;
    if (WLDS) {
      // lane-owned copy: every lane later reads and writes exactly these elements
      for (int T = w; T < NT; T += WD_WAVES)
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
      for (int s = 0; s < nb; ++s) {
        const int b0 = s * B;
        const int bc = min(B, n - b0);
        const int nblk = (bc + WD_BLOCK - 1) / WD_BLOCK;
        const int nchunk = (bc + WD_CHUNK - 1) / WD_CHUNK;
        const int32_t* pp = P.perms + (int64_t)E * row0 + (int64_t)e * n + b0;
        // stage chunk q of this batch: (global row, label) of its shuffled rows into LDS
        auto stage = [&](int q) {
          __syncthreads();                // every wave is done with the previous chunk
          const int c0 = q * WD_CHUNK;
          const int cn = min(WD_CHUNK, bc - c0);
          for (int i = tid; i < cn; i += WD_THREADS) {
            const int li = pp[c0 + i];
            sh.erow[i] = (int)(row0 + li);
            sh.elab[i] = P.labels[row0 + li];
          }
          __syncthreads();
        };

        // the gradient of the tiles in hand, accumulated over the blocks of the batch
        floatx4 ga[TG][CT][4];
        auto clear_ga = [&]() {
#pragma unroll
          for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
              for (int e4 = 0; e4 < 4; ++e4) ga[t][ct][e4] = floatx4{0.f, 0.f, 0.f, 0.f};
        };
        // ga += X_blk^T g_blk for tile group tg of block kb (its chunk staged); g from LDS (one
        // pass) or from the slot (two passes)
        auto backward = [&](int kb, int tg, auto from_lds) {
          const int cb = (kb % WD_CBLK) * WD_BLOCK;
          const int rows = min(WD_BLOCK, bc - kb * WD_BLOCK);
          if constexpr (decltype(from_lds)::value) {
            // one pass: the accumulators of all the wave's tiles stay live across the forward, so
            // g and the row indices are read from LDS where they are used, and a tile's rows are
            // loaded in two halves of 8 (register budget)
#pragma unroll
            for (int t = 0; t < TG; ++t) {
              const int T = w + WD_WAVES * t;
              if (T < NT) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                  float4 xv[2 * RT];
#pragma unroll
                  for (int k2 = 0; k2 < 2 * RT; ++k2) {
                    const int r = 4 * (2 * RT * h + k2) + lg;
                    xv[k2] = ld4(P.phi + (int64_t)sh.erow[cb + (r < rows ? r : 0)] * ld + 4 * l16 + 64 * T);
                  }
#pragma unroll
                  for (int k2 = 0; k2 < 2 * RT; ++k2) {
                    const int r = 4 * (2 * RT * h + k2) + lg;
                    const float4 x = wd_mask4(xv[k2], r < rows);
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                      const float gb = sh.g[kb & 1][r][ct * 16 + l16];
#pragma unroll
                      for (int e4 = 0; e4 < 4; ++e4) ga[t][ct][e4] = mfma4(comp(x, e4), gb, ga[t][ct][e4]);
                    }
                  }
                }
              }
            }
            return;
          }
          float gB[4 * RT][CT];
          int xrow[4 * RT];
          bool kok[4 * RT];
#pragma unroll
          for (int kk = 0; kk < 4 * RT; ++kk) {
            const int r = 4 * kk + lg;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
              gB[kk][ct] = decltype(from_lds)::value ? sh.g[kb & 1][r][ct * 16 + l16]
                                                     : gws[(int64_t)(kb * WD_BLOCK + r) * NC + ct * 16 + l16];
            kok[kk] = r < rows;
            xrow[kk] = sh.erow[cb + (kok[kk] ? r : 0)];
          }
#pragma unroll
          for (int t = 0; t < TG; ++t) {
            const int T = w + WD_WAVES * (tg * TG + t);
            if (T < NT) {
              float4 xv[4 * RT];
#pragma unroll
              for (int kk = 0; kk < 4 * RT; ++kk) xv[kk] = ld4(P.phi + (int64_t)xrow[kk] * ld + 4 * l16 + 64 * T);
#pragma unroll
              for (int kk = 0; kk < 4 * RT; ++kk) {
                const float4 x = wd_mask4(xv[kk], kok[kk]);
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4)
#pragma unroll
                  for (int ct = 0; ct < CT; ++ct) ga[t][ct][e4] = mfma4(comp(x, e4), gB[kk][ct], ga[t][ct][e4]);
              }
            }
          }
        };

        // ---------------- pass 1: per block, forward, logits, softmax, g to LDS or the slot ----------------
        const float invb = 1.0f / (float)bc;
        float cep = 0.f;
        int pend = -1;                    // (one pass) the block whose gradient is still to be accumulated
        if (onepass) clear_ga();
        for (int kb = 0; kb < nblk; ++kb) {
          const int cb = (kb % WD_CBLK) * WD_BLOCK;     // position of this block inside the staged chunk
          if (cb == 0) {
            if (pend >= 0) {              // (one pass) the pending block reads the chunk about to be replaced
              __syncthreads();
              backward(pend, 0, std::true_type{});
              pend = -1;
            }
            stage(kb / WD_CBLK);
            if (kb == 0 && (s > 0 || e > 0)) {          // the previous step's norm partials
              pn2 = 0.f;
              wn2 = 0.f;
#pragma unroll
              for (int i = 0; i < WD_WAVES; ++i) {
                pn2 += sh.red[i][0];
                wn2 += sh.red[i][1];
              }
            }
          }
          const int rows = min(WD_BLOCK, bc - kb * WD_BLOCK);   // valid rows of this block
          const int zb = kb % ZB;
          // invalid rows (>= rows) read a valid row and are zeroed after the load, so every
          // load is unconditional and the compiler can keep them all in flight.
          const float* xr[RT];
          bool xok[RT];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            const int r = rt * 16 + l16;
            xok[rt] = r < rows;
            xr[rt] = P.phi + (int64_t)sh.erow[cb + (xok[rt] ? r : 0)] * ld;
          }
          floatx4 acc[RT][CT];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = floatx4{0.f, 0.f, 0.f, 0.f};

          // per tile: all 4 x (RT + CT) 16-byte loads are issued before the MFMAs
          for (int T = w; T < NT; T += WD_WAVES) {
            float4 xv[4][RT], wv[4][CT];
            const int64_t dof = 64 * T + 16 * lg;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
              for (int rt = 0; rt < RT; ++rt) xv[q][rt] = ld4(xr[rt] + dof + 4 * q);
#pragma unroll
              for (int ct = 0; ct < CT; ++ct) {
                const int c = min(ct * 16 + l16, C - 1);
                wv[q][ct] = WLDS ? ld4(sW + c * LDW + dof + 4 * q) : ld4(src + c * ld + dof + 4 * q);
              }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
              for (int rt = 0; rt < RT; ++rt) xv[q][rt] = wd_mask4(xv[q][rt], xok[rt]);
#pragma unroll
              for (int ct = 0; ct < CT; ++ct) wv[q][ct] = wd_mask4(wv[q][ct], ct * 16 + l16 < C);
#pragma unroll
              for (int e4 = 0; e4 < 4; ++e4)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                  for (int ct = 0; ct < CT; ++ct)
                    acc[rt][ct] = mfma4(comp(xv[q][rt], e4), comp(wv[q][ct], e4), acc[rt][ct]);
            }
          }
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
              for (int i = 0; i < 4; ++i) sh.zpart[zb][w][rt * 16 + 4 * lg + i][ct * 16 + l16] = acc[rt][ct][i];
          __syncthreads();  // B1: partial logits of all waves (a buffer is rewritten two blocks on, past the next B1)

          // logits (fixed-order sum of the wave partials) + softmax / CE, one logit per thread
          for (int idx = tid; idx < NZ; idx += WD_THREADS) {   // NC lanes of one wave hold one row
            const int r = idx / NC, c = idx % NC;
            float z = 0.f;
#pragma unroll
            for (int i = 0; i < WD_WAVES; ++i) z += sh.zpart[zb][i][r][c];
            const bool valid = r < rows && c < C;
            const float m = wd_group_max<NC>(valid ? z : -INFINITY);
            const float se = wd_group_sum<NC>(valid ? expf(z - m) : 0.f);
            float gv = 0.f;
            if (valid) {
              const float lp = z - m - logf(se);               // log_softmax
              const bool isy = c == sh.elab[cb + r];
              gv = (isy ? -invb : 0.f) + expf(lp) * invb;      // d CE_mean / d z, over the whole batch
              if (isy) cep -= lp;
            }
            // (zero on the padding of the last block)
            if (onepass) sh.g[kb & 1][r][c] = gv;
            else gws[(int64_t)(kb * WD_BLOCK + r) * NC + c] = gv;
          }
          if (ZB == 1) __syncthreads();   // one buffer: the next block's partials wait for this softmax
          if (onepass) {
            // the block before this one: its g became visible at this block's B1, so its gradient
            // runs beside the others' softmax and forward, and a block costs one barrier
            if (pend >= 0) backward(pend, 0, std::true_type{});
            pend = kb;
          }
        }
        cep = wave_sum(cep);
        if (lane == 0) sh.cep[w] = cep;
        __syncthreads();  // B2: the batch's g (this workgroup's own global stores) and the CE partials visible

        if (tid == 0 && e == E - 1) {
          float ce = 0.f;
          for (int i = 0; i < WD_WAVES; ++i) ce += sh.cep[i];
          float loss = ce / (float)bc;                       // CrossEntropyLoss, mean
          if (P.prox) loss = loss + P.mu * sqrtf(pn2);       // + mu * ||W - W_a||_F  (tools.py:197, 203-205)
          if (P.reg) loss = loss + P.lam * sqrtf(wn2);       // + lambda * ||W||_F    (tools.py:201, 203, 207)
          lsum += (double)loss * (double)bc;                 // Meter.update(loss.item(), |b|)
        }

        // ---------------- pass 2: gradient over all blocks + fused SGD/prox/ridge update ----------------
        const float sp = (P.prox && pn2 > 0.f) ? P.mu / sqrtf(pn2) : 0.f;
        const float sr = (P.reg && wn2 > 0.f) ? P.lam / sqrtf(wn2) : 0.f;
        const float lr = P.lr;
        float npn = 0.f, nwn = 0.f;
        for (int tg = 0; tg < ngrp; ++tg) {
          if (onepass) {
            backward(pend, 0, std::true_type{});      // the last block (its g visible since B2)
          } else {
            clear_ga();
            for (int q = 0; q < nchunk; ++q) {
              if (nchunk > 1) stage(q);     // (one chunk: pass 1 left it staged)
              const int kb1 = min(nblk, (q + 1) * WD_CBLK);
              for (int kb = q * WD_CBLK; kb < kb1; ++kb) backward(kb, tg, std::false_type{});
            }
          }
          // ga[t][ct][e][q] = grad[c = ct*16 + l16][d = 64T + 16 lg + 4q + e]
#pragma unroll
          for (int t = 0; t < TG; ++t) {
            const int T = w + WD_WAVES * (tg * TG + t);
            if (T < NT) {
#pragma unroll
              for (int ct = 0; ct < CT; ++ct) {
                const int c = ct * 16 + l16;
                if (c < C) {
                  float4 wv[4], av[4];
#pragma unroll
                  for (int q = 0; q < 4; ++q) {
                    const int64_t off = c * ld + 64 * T + 16 * lg + 4 * q;
                    wv[q] = WLDS ? ld4(sW + (off - c * ld) + c * LDW) : ld4(src + off);
                    av[q] = P.prox ? ld4(anchor + off) : zero4;
                  }
#pragma unroll
                  for (int q = 0; q < 4; ++q) {
                    const int64_t off = c * ld + 64 * T + 16 * lg + 4 * q;
                    float o[4];
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                      const float wc = comp(wv[q], e4);
                      const float ac = comp(av[q], e4);
                      float gr = ga[t][ct][e4][q];
                      if (P.prox) gr = gr + (wc - ac) * sp;
                      if (P.reg) gr = gr + wc * sr;
                      o[e4] = wc - lr * gr;
                      const float dp = o[e4] - ac;
                      npn += dp * dp;
                      nwn += o[e4] * o[e4];
                    }
                    if (WLDS) st4(sW + (off - c * ld) + c * LDW, make_float4(o[0], o[1], o[2], o[3]));
                    else st4(Wj + off, make_float4(o[0], o[1], o[2], o[3]));
                  }
                }
              }
            }
          }
        }
        npn = wave_sum(npn);
        nwn = wave_sum(nwn);
        if (lane == 0) {              // read after the next step's first staging barrier
          sh.red[w][0] = npn;
          sh.red[w][1] = nwn;
        }
        src = Wj;
      }
    }
    if (WLDS) {
      for (int T = w; T < NT; T += WD_WAVES)
        for (int ct = 0; ct < CT; ++ct) {
          const int c = ct * 16 + l16;
          if (c < C)
            for (int q = 0; q < 4; ++q) {
              const int64_t off = 64 * T + 16 * lg + 4 * q;
              st4(Wj + c * ld + off, ld4(sW + c * LDW + off));
            }
        }
    }
    if (tid == 0) P.loss[j] = lsum / (double)n;
    __syncthreads();
  }
}

template <int CT, bool OP>
static int launch_wd(const LTParams& P, const WideWS& X, int grid, hipStream_t st) {
  const size_t wbytes = sizeof(float) * (size_t)P.C * (size_t)(P.ld + 4);
  const size_t budget = 160 * 1024 - sizeof(WDShared<CT>);
  if (wbytes <= budget) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&local_train_wide_kernel<CT, true, OP>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)wbytes);
    if (e != hipSuccess) return fail(FS_EHIP, std::string("fs_local_train: ") + hipGetErrorString(e));
    hipLaunchKernelGGL((local_train_wide_kernel<CT, true, OP>), dim3(grid), dim3(WD_THREADS), wbytes, st, P, X);
  } else {
    hipLaunchKernelGGL((local_train_wide_kernel<CT, false, OP>), dim3(grid), dim3(WD_THREADS), 0, st, P, X);
  }
  return FS_OK;
}

// `grid` workgroups (wd_grid) walk the clients, each with its own slot of X; fs_local_train's
// validation and the workspace's layout are in local_train_host.cpp
int launch_local_train_wide(const LTParams& P, const WideWS& X, int grid, hipStream_t st) {
  // one pass where a wave's tiles are one group of TG = 4 / CT: ld <= 2048 (C <= 16), ld <= 1024 (above)
  const int tpw = ((int)(P.ld >> 6) + WD_WAVES - 1) / WD_WAVES;
  if (P.C <= 16) return tpw <= 4 ? launch_wd<1, true>(P, X, grid, st) : launch_wd<1, false>(P, X, grid, st);
  return tpw <= 2 ? launch_wd<2, true>(P, X, grid, st) : launch_wd<2, false>(P, X, grid, st);
}

}  // namespace fs

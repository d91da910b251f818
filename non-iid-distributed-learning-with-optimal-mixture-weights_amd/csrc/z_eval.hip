// fs_z_eval_* -- per-client evaluation: the (loss, accuracy) of every one of N client models on
// a row set, from their logits Z in fs_mix_z's layout (row v: C segments of ldN = (N + 3) & ~3
// floats, client j at Z[v][c * ldN + j]).  The reference evaluates one model per test_loop call
// (functions/tools.py:218-237); its local_weights[j] (tools.py:340-343) are never scored.
//
// A pure stream: Z is read once, 16 bytes per lane, lanes along the client axis, so a wave reads
// contiguous bytes of one class segment.  A lane keeps its 4 clients' C logits in registers and
// takes max, arg-max (strict >: ties to the lowest class), sum of exp and log from them:
//     ce = log(sum_c exp(z_c - m)) + (m - z_y)        (eval_rows.h's value, never -0)
// MSE (C = 1): (z - y)^2 in fp32, "correct" = (y == 0) as fs_eval_mse.
//
// Work split: a workgroup takes one row block of ZE_ROWS rows (fixed boundaries in ABSOLUTE row
// numbers) times one column tile of ZE_TILE_Q quads (256 clients); the grid runs the column
// tiles of a row block side by side (config 5's Z: 3.8 TB/s, against 3.4 with the row blocks
// fastest).  Its 256 threads walk the (row, quad) items of that rectangle, item
// i -> row i / tq, quad i % tq (tq = quads of the tile), so with few clients (N = 10: 3 quads) a
// wave covers all 16 rows of the block at once instead of idling 61 lanes.  Each item leaves its 4
// per-row fp32 losses and correct flags in LDS; then thread t sums client t's rows IN ROW ORDER in
// fp64 and writes the block's partial pair to the workspace [row block][ldN][2].  That sum does not depend on how items met lanes, so a client's partial
// depends on its own column and the labels alone (column independence), and a row block's partial
// on its rows alone (chunk independence).  The finaliser folds the row blocks per client in a
// fixed order (ZF_STRIDES strided sums, then those in order).  No atomics, no cross-workgroup
// wait, no spin: bitwise reproducible.
#include "common.h"

namespace fs {

constexpr int ZE_ROWS = 16;        // rows per row block (fs_z_eval_block_rows)
constexpr int ZE_TILE_Q = 64;      // quads (of 4 clients) per column tile
constexpr int ZE_THREADS = 256;
constexpr int ZF_STRIDES = 8;      // finaliser: strided sums over the row blocks
constexpr int ZF_CLIENTS = 32;     // finaliser: clients per workgroup

// items a thread has in flight per trip: enough 16-byte loads outstanding at few classes
constexpr int ze_unroll(int C) { return C <= 2 ? 4 : (C <= 8 ? 2 : 1); }

template <int CC, bool MSE>
__global__ __launch_bounds__(ZE_THREADS) void z_eval_kernel(const float* __restrict__ Z,
                                                            const void* __restrict__ tgt, int64_t row0, int rows,
                                                            int N, int ldN, int tiles, double* __restrict__ ws) {
  constexpr int U = ze_unroll(CC);
  __shared__ float ce_s[ZE_ROWS][4 * ZE_TILE_Q];
  __shared__ uint32_t cor_s[ZE_ROWS][ZE_TILE_Q];
  const int tid = threadIdx.x;
  const int nq = ldN >> 2;
  // column tiles fastest: workgroups that run side by side read neighbouring pieces of the same rows
  const int rb = (int)(blockIdx.x / (unsigned)tiles);           // chunk-local row block
  const int q0 = (int)(blockIdx.x - (unsigned)rb * (unsigned)tiles) * ZE_TILE_Q;
  const int tq = min(ZE_TILE_Q, nq - q0);
  const int64_t r0 = (int64_t)rb * ZE_ROWS;                     // chunk-local first row of the block
  const int vr = (int)min((int64_t)ZE_ROWS, (int64_t)rows - r0);
  const int items = vr * tq;

  for (int base = tid; base < items; base += U * ZE_THREADS) {
    float4 z[U][CC];
    int rr[U], qq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int item = min(base + u * ZE_THREADS, items - 1);   // clamped: a valid address; masked below
      if (tq == ZE_TILE_Q) {
        rr[u] = item >> 6;
        qq[u] = item & 63;
      } else {
        rr[u] = item / tq;
        qq[u] = item - rr[u] * tq;
      }
      const float* zp = Z + (r0 + rr[u]) * (int64_t)CC * ldN + 4 * (int64_t)(q0 + qq[u]);
#pragma unroll
      for (int c = 0; c < CC; ++c) z[u][c] = ld4(zp + (int64_t)c * ldN);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (base + u * ZE_THREADS >= items) break;
      float4 ce;
      uint32_t cor;
      if (MSE) {
        const float y = static_cast<const float*>(tgt)[row0 + r0 + rr[u]];
        const float4 v = z[u][0];
        const float a = v.x - y, b = v.y - y, c = v.z - y, d = v.w - y;
        ce = make_float4(a * a, b * b, c * c, d * d);
        cor = (y == 0.0f) ? 0x01010101u : 0u;      // top-1 of one column is index 0 (tools.py:88-90)
      } else {
        const int yy = static_cast<const int32_t*>(tgt)[row0 + r0 + rr[u]];
        float4 m = z[u][0], zy = z[u][0];
        int ax = 0, ay = 0, az = 0, aw = 0;
#pragma unroll
        for (int c = 1; c < CC; ++c) {
          const float4 v = z[u][c];
          if (v.x > m.x) { m.x = v.x; ax = c; }
          if (v.y > m.y) { m.y = v.y; ay = c; }
          if (v.z > m.z) { m.z = v.z; az = c; }
          if (v.w > m.w) { m.w = v.w; aw = c; }
          if (c == yy) zy = v;
        }
        float4 se = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < CC; ++c) {
          const float4 v = z[u][c];
          se.x += __expf(v.x - m.x);
          se.y += __expf(v.y - m.y);
          se.z += __expf(v.z - m.z);
          se.w += __expf(v.w - m.w);
        }
        ce = make_float4(logf(se.x) + (m.x - zy.x), logf(se.y) + (m.y - zy.y), logf(se.z) + (m.z - zy.z),
                         logf(se.w) + (m.w - zy.w));
        cor = (ax == yy ? 1u : 0u) | (ay == yy ? 0x100u : 0u) | (az == yy ? 0x10000u : 0u) |
              (aw == yy ? 0x1000000u : 0u);
      }
      st4(&ce_s[rr[u]][4 * qq[u]], ce);
      cor_s[rr[u]][qq[u]] = cor;
    }
  }
  __syncthreads();
  const int j = 4 * q0 + tid;
  if (tid < 4 * tq && j < N) {
    double s = 0.0;
    uint32_t k = 0;
    const int sh = 8 * (tid & 3);
    for (int r = 0; r < vr; ++r) {
      s += (double)ce_s[r][tid];
      k += (cor_s[r][tid >> 2] >> sh) & 1u;
    }
    const int64_t blk = row0 / ZE_ROWS + (int64_t)rb;
    double* o = ws + 2 * (blk * ldN + j);
    o[0] = s;
    o[1] = (double)k;
  }
}

__global__ __launch_bounds__(ZF_STRIDES* ZF_CLIENTS) void z_eval_finish_kernel(const double* __restrict__ ws,
                                                                               int64_t nb, int n, int N, int ldN,
                                                                               double* __restrict__ out) {
  __shared__ double s[2][ZF_STRIDES][ZF_CLIENTS];
  const int jl = threadIdx.x % ZF_CLIENTS, g = threadIdx.x / ZF_CLIENTS;
  const int j = (int)blockIdx.x * ZF_CLIENTS + jl;
  double a = 0.0, b = 0.0;
  if (j < N) {
    for (int64_t i = g; i < nb; i += ZF_STRIDES) {
      const double* p = ws + 2 * (i * ldN + j);
      a += p[0];
      b += p[1];
    }
  }
  s[0][g][jl] = a;
  s[1][g][jl] = b;
  __syncthreads();
  if (g == 0 && j < N) {
    for (int i = 1; i < ZF_STRIDES; ++i) {
      a += s[0][i][jl];
      b += s[1][i][jl];
    }
    out[2 * j] = a / (double)n;
    out[2 * j + 1] = 100.0 * b / (double)n;
  }
}

static int64_t z_eval_ws_doubles(int64_t n, int N) {
  return (n + ZE_ROWS - 1) / ZE_ROWS * (int64_t)((N + 3) & ~3) * 2;
}

template <int CC, bool MSE>
static void z_eval_launch(const float* Z, const void* tgt, int64_t row0, int rows, int N, double* ws,
                          hipStream_t st) {
  const int ldN = (N + 3) & ~3;
  const int tiles = (ldN / 4 + ZE_TILE_Q - 1) / ZE_TILE_Q;
  const int64_t blocks = ((int64_t)rows + ZE_ROWS - 1) / ZE_ROWS;
  hipLaunchKernelGGL((z_eval_kernel<CC, MSE>), dim3((unsigned)(blocks * tiles)), dim3(ZE_THREADS), 0, st, Z, tgt,
                     row0, rows, N, ldN, tiles, ws);
}

static int z_eval_add(const float* d_Z, const void* d_tgt, int n, int row0, int rows, int N, int C, bool mse,
                      double* d_ws, int64_t ws_doubles, hipStream_t st) {
  FS_REQUIRE(n >= 1 && N >= 1, "n and N must be >= 1");
  FS_REQUIRE(C >= 1 && C <= 32, "num_classes must be in [1, 32]");
  FS_REQUIRE(((int64_t)rows / ZE_ROWS + 1) * (((int64_t)N + 4 * ZE_TILE_Q - 1) / (4 * ZE_TILE_Q)) < ((int64_t)1 << 31),
             "rows x N too large for one launch: add the rows in chunks");
  FS_REQUIRE(d_Z && d_tgt && d_ws, "null pointer");
  FS_REQUIRE(rows >= 1 && row0 >= 0 && (int64_t)row0 + rows <= n, "rows [row0, row0 + rows) must lie in [0, n)");
  FS_REQUIRE(row0 % ZE_ROWS == 0, "row0 must be a multiple of the row block (fs_z_eval_block_rows)");
  FS_REQUIRE(rows % ZE_ROWS == 0 || row0 + rows == n, "only the last chunk may end inside a row block");
  FS_REQUIRE(ws_doubles >= z_eval_ws_doubles(n, N), "workspace too small (fs_z_eval_ws_doubles)");
  if (mse) {
    z_eval_launch<1, true>(d_Z, d_tgt, row0, rows, N, d_ws, st);
  } else {
    switch (C) {
#define FS_ZE_CASE(c) \
  case c:             \
    z_eval_launch<c, false>(d_Z, d_tgt, row0, rows, N, d_ws, st); \
    break;
      FS_ZE_CASE(1) FS_ZE_CASE(2) FS_ZE_CASE(3) FS_ZE_CASE(4) FS_ZE_CASE(5) FS_ZE_CASE(6) FS_ZE_CASE(7) FS_ZE_CASE(8)
      FS_ZE_CASE(9) FS_ZE_CASE(10) FS_ZE_CASE(11) FS_ZE_CASE(12) FS_ZE_CASE(13) FS_ZE_CASE(14) FS_ZE_CASE(15)
      FS_ZE_CASE(16) FS_ZE_CASE(17) FS_ZE_CASE(18) FS_ZE_CASE(19) FS_ZE_CASE(20) FS_ZE_CASE(21) FS_ZE_CASE(22)
      FS_ZE_CASE(23) FS_ZE_CASE(24) FS_ZE_CASE(25) FS_ZE_CASE(26) FS_ZE_CASE(27) FS_ZE_CASE(28) FS_ZE_CASE(29)
      FS_ZE_CASE(30) FS_ZE_CASE(31) FS_ZE_CASE(32)
#undef FS_ZE_CASE
    }
  }
  FS_LAUNCH_CHECK();
  return FS_OK;
}

static int z_eval_finish(const double* d_ws, int64_t ws_doubles, int n, int N, double* d_out, hipStream_t st) {
  FS_REQUIRE(n >= 1 && N >= 1, "n and N must be >= 1");
  FS_REQUIRE(d_ws && d_out, "null pointer");
  FS_REQUIRE(ws_doubles >= z_eval_ws_doubles(n, N), "workspace too small (fs_z_eval_ws_doubles)");
  const int64_t nb = ((int64_t)n + ZE_ROWS - 1) / ZE_ROWS;
  hipLaunchKernelGGL(z_eval_finish_kernel, dim3((N + ZF_CLIENTS - 1) / ZF_CLIENTS), dim3(ZF_STRIDES * ZF_CLIENTS), 0,
                     st, d_ws, nb, n, N, (N + 3) & ~3, d_out);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace fs

extern "C" int fs_z_eval_block_rows(void) { return fs::ZE_ROWS; }

extern "C" int64_t fs_z_eval_ws_doubles(int n, int N) {
  return (n < 1 || N < 1) ? 0 : fs::z_eval_ws_doubles(n, N);
}

extern "C" int fs_z_eval_add(const float* d_Z, const int32_t* d_labels, int n, int row0, int rows, int N, int C,
                             double* d_ws, int64_t ws_doubles, void* stream) {
  return fs::z_eval_add(d_Z, d_labels, n, row0, rows, N, C, false, d_ws, ws_doubles,
                        reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_z_eval_add_mse(const float* d_Z, const float* d_y, int n, int row0, int rows, int N, double* d_ws,
                                 int64_t ws_doubles, void* stream) {
  return fs::z_eval_add(d_Z, d_y, n, row0, rows, N, 1, true, d_ws, ws_doubles,
                        reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_z_eval_finish(const double* d_ws, int64_t ws_doubles, int n, int N, double* d_out, void* stream) {
  return fs::z_eval_finish(d_ws, ws_doubles, n, N, d_out, reinterpret_cast<hipStream_t>(stream));
}

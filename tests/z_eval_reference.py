"""A float64 per-client reference of the per-client evaluation (fs_z_eval_*, csrc/z_eval.hip), a
numpy-fp32 emulation of the kernel's per-row formula, and the inputs of tests/test_gpu_z_eval.py.

The kernel reads logits Z in fs_mix_z's layout: row v holds C segments of ldN = (N + 3) & ~3
floats, client j's class-c logit at Z[v][c * ldN + j].  The tests build Z on the host, so the
reference sees the same fp32 logits as the kernel and the only error left is the softmax
arithmetic.  All builders produce integers times one power of two, small enough that every
difference of two logits is exact in fp32 -- the premise of ``eval_reference.loss_bound``.

The tile constants below restate csrc/z_eval.hip; the sweep takes its boundaries from them.
"""
import numpy as np

from tests.eval_reference import loss_bound

ZE_ROWS = 16            # rows per row block (fs_z_eval_block_rows)
ZE_TILE = 256           # clients per column tile (ZE_TILE_Q = 64 quads of 4)
ZE_THREADS = 256        # (row, quad) items per trip at unroll 1
ZE_UNROLL = ((2, 4), (8, 2), (32, 1))     # C <= 2: 4 items in flight per thread, C <= 8: 2, else 1
ZF_STRIDES = 8          # finaliser: strided sums over the row blocks
ZF_CLIENTS = 32         # finaliser: clients per workgroup

# N: the base list; one below / at / above the finaliser's client tile (31, 32, 33) and the
# column tile (255, 256, 257); one quad (1, 4) against two (5)
SWEEP_N = (1, 4, 5, 31, 32, 33, 100, 255, 256, 257, 1000)
# C: the base list plus both sides of the unroll steps (2 | 3, 8 | 9)
SWEEP_C = (1, 2, 3, 8, 9, 10, 16, 17, 32)
# n: the base list; one below / at / above one and two row blocks; ZF_STRIDES row blocks plus
# one row -- the finaliser's second stride
SWEEP_ROWS = (1, 15, 16, 17, 31, 32, 33, 65, ZF_STRIDES * ZE_ROWS + 1)
assert len(SWEEP_C) == len(SWEEP_ROWS)


def sweep_cases():
    """(n, N, C): every N meets every C and every n once (C and n paired by a shift that moves
    with N), 99 cases instead of the full product."""
    k = len(SWEEP_C)
    return [(SWEEP_ROWS[(i + a) % k], N, SWEEP_C[i]) for a, N in enumerate(SWEEP_N) for i in range(k)]


def case_seed(n, N, C):
    return (n * 1000003 + N * 1009 + C) % (2 ** 31 - 1)


def ldn(N):
    return (N + 3) & ~3


def to_layout(A, pad=0.0):
    """Per-client logits A [n, N, C] -> Z [n, C * ldN] fp32 in fs_mix_z's layout; the padding
    columns N..ldN-1 of every class segment hold ``pad``."""
    A = np.asarray(A, np.float32)
    n, N, C = A.shape
    Z = np.full((n, C, ldn(N)), pad, np.float32)
    Z[:, :, :N] = A.transpose(0, 2, 1)
    return np.ascontiguousarray(Z.reshape(n, C * ldn(N)))


def from_layout(Z, N, C):
    """Z [n, C * ldN] -> A [n, N, C]."""
    n = Z.shape[0]
    return np.asarray(Z).reshape(n, C, ldn(N))[:, :, :N].transpose(0, 2, 1)


def per_client_ref(Z, y, N, C):
    """float64 reference from the fp32 Z: (ce [N, n] per row, loss [N], correct [N]).  Log-sum-exp
    with the maximum subtracted, np.argmax's first maximum (ties to the lowest class)."""
    z = from_layout(Z, N, C).astype(np.float64)           # [n, N, C]
    y = np.asarray(y).astype(np.int64)
    m = z.max(axis=2)
    lse = m + np.log(np.exp(z - m[:, :, None]).sum(axis=2))
    zy = np.take_along_axis(z, y[:, None, None].repeat(N, 1), axis=2)[:, :, 0]
    ce = (lse - zy).T
    correct = (np.argmax(z, axis=2) == y[:, None]).sum(axis=0)
    return ce, ce.mean(axis=1), correct.astype(np.int64)


def mse_ref(Z, y, N):
    """float64 reference of the MSE twin: (mse [N], accuracy % -- 100 #{y == 0} / n, one value)."""
    z = np.asarray(Z, np.float64)[:, :N]
    y = np.asarray(y, np.float64)
    return ((z - y[:, None]) ** 2).mean(axis=0), 100.0 * float((y == 0).sum()) / len(y)


def kernel_formula_f32(Z, y, N, C, subtract_max=True, pad_slot=False):
    """z_eval.hip's per-row arithmetic in numpy float32: log(sum_c exp(z_c - m)) + (m - z_y), the
    sum over the classes in order; the rows' mean in float64.  Returns (ce [N, n], loss [N]).
    Two deliberately broken variants show what the saturated inputs catch: ``subtract_max=False``
    (m = 0 in the exponent) and ``pad_slot`` (a padded class slot entering the maximum as 0)."""
    z = from_layout(Z, N, C).astype(np.float32)
    y = np.asarray(y).astype(np.int64)
    m = z.max(axis=2)
    if pad_slot:
        m = np.maximum(m, np.float32(0))
    ms = m if subtract_max else np.zeros_like(m)
    se = np.zeros_like(m)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for c in range(C):
            se = (se + np.exp((z[:, :, c] - ms).astype(np.float32))).astype(np.float32)
        zy = np.take_along_axis(z, y[:, None, None].repeat(N, 1), axis=2)[:, :, 0]
        ce = (np.log(se).astype(np.float32) + (ms - zy).astype(np.float32)).astype(np.float32)
        ce = ce.astype(np.float64).T
        return ce, ce.mean(axis=1)


def bounds(C, ce_rows):
    """loss_bound per client from the reference's per-row cross-entropies [N, n]."""
    return np.array([loss_bound(C, r) for r in ce_rows])


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def grid_logits(rs, n, N, C, spread=20.0):
    """(Z, y): logits that are integers in about +-4 spread times 2^-6 -- every difference exact
    in fp32 -- and labels that include 0 and C - 1 whenever n >= 2."""
    A = np.round(rs.normal(size=(n, N, C)) * (spread / 3.0) * 64.0) / 64.0
    y = rs.randint(0, C, size=n).astype(np.int64)
    y[0] = 0
    if n >= 2:
        y[-1] = C - 1
    return to_layout(A), y


def tied_logits(rs, n, N, C):
    """(Z, y, info): ``grid_logits`` with client 0's C logits equal within every row (another
    value per row), and on every fourth row (1, 5, 9, ...) client 1 (if N >= 2, C >= 2) given two
    tied maxima, the row labelled with the lower, higher, lower of the pair in turn, as
    ``eval_reference.exact_problem`` labels its ties.  info: 'flat_correct' client 0's exact count
    (#{y == 0}), 'tied_low' / 'tied_high' the rows of client 1 labelled low / high."""
    Z, y = grid_logits(rs, n, N, C)
    A = from_layout(Z, N, C).copy()
    A[:, 0, :] = (rs.randint(-640, 641, size=n) / 64.0)[:, None]
    low = high = 0
    if N >= 2 and C >= 2:
        for k, v in enumerate(range(1, n, 4)):
            a, b = sorted(rs.choice(C, size=2, replace=False))
            top = A[v, 1].max() + 1.0
            A[v, 1, a] = A[v, 1, b] = top
            if k % 3 == 1:
                y[v], high = b, high + 1
            else:
                y[v], low = a, low + 1
    return to_layout(A), y, dict(flat_correct=int((y == 0).sum()), tied_low=low, tied_high=high)


SAT_OFFSETS = (0, 64, -64, 128, -128)


def saturated_logits(rs, n, N, C):
    """(Z, y, info): saturated rows at common offsets.  Row v sits at offset SAT_OFFSETS[v % 5];
    each client's winner is offset + b (b an integer in [-8, 8]) and every other class trails it
    by 200 + r (r in [0, 16]), all integers.  At offsets -64 and -128 every logit of the row is
    negative.  Client 0's winner is the row's label in every row: each of its rows contributes
    exactly 0.0 (exp(-200) is 0 in fp32, the sum is 1, log 1 = 0, m - z_y = 0), so its loss is
    exactly 0.0 and its accuracy 100.  For any other client a row labelled with a loser
    contributes exactly its trail, an integer.  info: 'negative_rows' the all-negative rows."""
    off = np.array([SAT_OFFSETS[v % 5] for v in range(n)], np.float64)
    y = rs.randint(0, C, size=n).astype(np.int64)
    win = rs.randint(0, C, size=(n, N))
    win[:, 0] = y
    top = off[:, None] + rs.randint(-8, 9, size=(n, N))
    A = top[:, :, None] - (200 + rs.randint(0, 17, size=(n, N, C)))
    np.put_along_axis(A, win[:, :, None], top[:, :, None], axis=2)
    return to_layout(A), y, dict(negative_rows=np.nonzero(off < 0)[0])


def mse_values(rs, n, N):
    """(Z [n, ldN], y [n]): fp32 predictions and targets of the MSE twin; every third target is
    exactly 0 (the degenerate accuracy counts them)."""
    Z = to_layout(rs.normal(size=(n, N, 1)).astype(np.float32) * 3.0)
    y = (rs.normal(size=n) * 2.0).astype(np.float32)
    y[::3] = 0.0
    return Z, y

"""A float64 reference of the local evaluation (fs_eval_clients, csrc/eval_clients.hip) -- a model
scored on every client's own row segment -- and the partitions tests/test_gpu_eval_clients.py
sweeps.

``segment_ref``      ``eval_reference.ce_acc_ref`` per row segment: one shared model [C, D] (the
                     logits of all rows at once, then cut), or one model per client [N, C, D].
``segment_mse_ref``  the MSE twin: mean (x . w_j - y)^2 per segment and fs_eval_mse's degenerate
                     accuracy 100 #{y == 0} / n_j.
``client_models``    N different models from one: the class rows rolled by j and scaled by a
                     power of two, so exact logits stay exact and tied maxima stay tied.
``ws_doubles``       the documented workspace size (include/fedsim.h).
``sweep_cases``      the structural sweep: the boundaries of the 16-row groups counted from each
                     client's first row, of the class tiles and of the finaliser's stride.
"""
import numpy as np

from tests.eval_reference import ce_acc_ref

GROUP = 16             # rows per workgroup, counted from the client's first row
FIN_THREADS = 256      # the per-client finaliser: a second stride from 257 groups on

# one partition, in this order: 1 row; one short group; exactly one; one over; two groups less one;
# two and one over; a full group BETWEEN ragged neighbours; a 1-row client after it; 17 groups
SIZES9 = (1, 15, 16, 17, 31, 33, 16, 1, 257)
SINGLES = (1, 4113)    # N = 1: 4113 rows = 258 groups, the finaliser's second stride
SWEEP_C = (1, 2, 10, 16, 17, 32)            # eval_clients_kernel<1> up to 16 classes, <2> above
SWEEP_LD = ((64, 27), (128, 91), (2048, 2048))   # (ld, D): D = ld - 37 reads zero padding; 32 tiles
MANY = ((300, 20, 40), (3000, 1, 1))        # (N, smallest, largest client): more workgroups than CUs


def partitions():
    return (SIZES9,) + tuple((n,) for n in SINGLES)


def sweep_cases():
    """(sizes, ld, D, C): every partition with every leading dimension and every class count."""
    return [(sizes, ld, D, C) for sizes in partitions() for ld, D in SWEEP_LD for C in SWEEP_C]


def case_seed(sizes, ld, D, C):
    return (sum(sizes) * 1000003 + len(sizes) * 7919 + D * 1009 + C) % (2 ** 31 - 1)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def groups(sizes):
    return int(sum((int(n) + GROUP - 1) // GROUP for n in sizes))


def ws_doubles(total_rows, N):
    """(N + 2) / 2 doubles hold the N + 1 int32 prefix entries; then one pair per group, at most
    total_rows / 16 + N of them (integer divisions)."""
    return (N + 2) // 2 + 2 * (total_rows // GROUP + N)


def client_models(W, N):
    """[N, C, D] from W [C, D]: model j is W with its class rows rolled down by j, times
    2^-(j % 3).  Products and partial sums stay integers times one power of two per model, and
    two equal logits of a row stay equal (on other class indices)."""
    return np.stack([np.roll(W, j, axis=0) * np.float32(2.0 ** -(j % 3)) for j in range(N)]).astype(np.float32)


def segment_ref(X, y, sizes, W):
    """Per client: (list of per-row cross-entropies, loss [N], correct count [N]) in float64.
    W [C, D]: the one model on every segment; W [N, C, D]: model j on segment j."""
    off = offsets(sizes)
    W = np.asarray(W)
    rows, loss, correct = [], np.empty(len(sizes)), np.empty(len(sizes), np.int64)
    if W.ndim == 2:
        # the pooled logits once, cut at the segment boundaries
        z = np.asarray(X, np.float64) @ W.astype(np.float64).T
        yy = np.asarray(y).astype(np.int64)
        m = z.max(axis=1)
        ce = m + np.log(np.exp(z - m[:, None]).sum(axis=1)) - z[np.arange(len(yy)), yy]
        hit = np.argmax(z, axis=1) == yy
        for j in range(len(sizes)):
            a, b = off[j], off[j + 1]
            rows.append(ce[a:b])
            loss[j], correct[j] = ce[a:b].mean(), hit[a:b].sum()
        return rows, loss, correct
    for j in range(len(sizes)):
        a, b = off[j], off[j + 1]
        r, loss[j], correct[j] = ce_acc_ref(X[a:b], y[a:b], W[j])
        rows.append(r)
    return rows, loss, correct


def segment_mse_ref(X, y, sizes, w):
    """Per client (mse [N], accuracy % [N]); w [D] shared or [N, D] per client."""
    off = offsets(sizes)
    w = np.asarray(w, np.float64)
    y = np.asarray(y, np.float64).reshape(-1)
    mse, acc = np.empty(len(sizes)), np.empty(len(sizes))
    for j in range(len(sizes)):
        a, b = off[j], off[j + 1]
        r = np.asarray(X[a:b], np.float64) @ (w if w.ndim == 1 else w[j]) - y[a:b]
        mse[j] = float((r * r).mean())
        acc[j] = 100.0 * float((y[a:b] == 0).sum()) / (b - a)
    return mse, acc


def mse_targets(rs, X, w):
    """float32 targets near x . w with every fourth one exactly 0 (the degenerate accuracy counts
    exact zeros)."""
    y = (np.asarray(X, np.float64) @ np.asarray(w, np.float64) + 0.25 * rs.normal(size=len(X))).astype(np.float32)
    y[::4] = 0.0
    return y


def objective(loss, sizes):
    """sum_j (n_j / n) loss_j in float64, client by client."""
    w = np.asarray(sizes, np.float64) / float(np.sum(sizes))
    acc = 0.0
    for j in range(len(sizes)):
        acc = acc + w[j] * loss[j]
    return acc


def many_sizes(rs, N, lo, hi):
    return tuple(int(v) for v in rs.randint(lo, hi + 1, size=N))

"""CPU restatement of FedTopK's operator (include/fedsim.h, csrc/aggregate_topk.hip) in numpy float32,
so that the kernels' output can be held to it bit for bit.

Over the sampled rows W [M, len] (already gathered, k ascending), x [len], the rows' residuals e [M, len]
(None: no memory), weights q [M] and 1 <= kcount <= len, every operation rounded to float32 on its own:

  a_k   = (W_k - x) + e_k                         (no memory: W_k - x)
  key   = bits(a_k) & 0x7fffffff                   (uint32: magnitude order, Inf above finite, NaN above Inf)
  tau_k = the kcount-th largest key of the row    (np.partition on the keys)
  kept  = key >= tau_k                            (ties all kept)
  e_k  <- where(kept, +0, a_k)
  W_g  <- x + fold_k q_k * where(kept, a_k, +0)   (tests/fold_restatement.py: the regimes of fs_aggregate)
"""
import numpy as np

from tests import fold_restatement as FR

F32 = np.float32
LDS_FLOATS = 40960      # an MI355X CU's 160 KiB of LDS in floats (the kernel stages no row; a test point all the same)


def keys(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32) & np.uint32(0x7fffffff)


def corrected(W, x, e=None):
    """a [M, len]: (W_k - x) + e_k, each operation rounded to float32 (NaN / Inf arithmetic is silent)."""
    with np.errstate(all='ignore'):
        a = (np.asarray(W, F32) - np.asarray(x, F32)[None, :]).astype(F32)
        if e is not None:
            a = (a + np.asarray(e, F32)).astype(F32)
    return a


def threshold(a, kcount):
    """(tau [M] uint32, n [M] int32, kept [M, len] bool) of the rows of a."""
    key = keys(a)
    L = key.shape[1]
    assert 1 <= kcount <= L
    tau = np.partition(key, L - kcount, axis=1)[:, L - kcount]
    kept = key >= tau[:, None]
    return tau.astype(np.uint32), kept.sum(axis=1).astype(np.int32), kept


def split(a, kept):
    """(s, e_new): the transmitted part and the residual, +0 where the other holds the value."""
    zero = np.zeros_like(a)
    return np.where(kept, a, zero), np.where(kept, zero, a)


def aggregate(W, x, e, q, kcount, chunks=0, ws_partials=None):
    """dict(out [len], e [M, len] or None, tau [M] float32 (the key's bits), kept [M] int32, a, s)."""
    W, x, q = np.asarray(W, F32), np.asarray(x, F32), np.asarray(q, F32)
    M = W.shape[0]
    a = corrected(W, x, e)
    tau, n, kept = threshold(a, kcount)
    s, e_new = split(a, kept)
    with np.errstate(all='ignore'):
        delta = FR.fold(M, chunks, ws_partials, lambda k, first: (q[k] * s[k]).astype(F32))
        out = (x + delta).astype(F32)
    return dict(out=out, e=None if e is None else e_new, tau=tau.view(F32), kept=n, a=a, s=s)


def dense(W, x, q, chunks=0, ws_partials=None):
    """fold_restatement's update fold: x + fold_k q_k (W_k - x) -- FedNova's mode 2, fs_aggregate_opt's AVGM
    at beta1 = 0, eta = 1 -- which FedTopK equals where every nonzero is kept and e = 0."""
    W, x, q = np.asarray(W, F32), np.asarray(x, F32), np.asarray(q, F32)
    with np.errstate(all='ignore'):
        delta = FR.fold(W.shape[0], chunks, ws_partials, lambda k, first: (q[k] * (W[k] - x).astype(F32)).astype(F32))
        return (x + delta).astype(F32)


def topk_count(ratio, C, D):
    """tools.topk_count restated: an int is the count, a fraction gives max(1, floor(ratio * C * D))."""
    if isinstance(ratio, (int, np.integer)) and not isinstance(ratio, bool):
        return int(ratio)
    return max(1, int(np.floor(float(ratio) * C * D)))

"""CPU restatement of DP-FedAvg's server step (include/fedsim.h, csrc/aggregate_dp.hip) in numpy, so that
the kernels' output can be held to it: Philox4x32-10, the noise field g, the norms, the coefficients, the
state update and the clipped fold.

Over the sampled rows W [M, len] (already gathered, k ascending), x [len], weights q [M] float32, clip S,
noise multiplier z, seed and round t:

  d_k   = fl(W_k - x)                              float32
  n_k   = sum_i d_k[i]^2                           float32 squares summed in float64 (as qffl_restatement.norms)
  r_k   = sqrt(n_k);  s_k = 1 if r_k <= S else S / r_k              float64
  c_k   = f32(q_k * s_k); a row whose n_k is NaN or Inf is dropped: c_k = 0
  Delta = fold_k (c_k == 0 ? +0 : fl(c_k * d_k))   tests/fold_restatement.py: the regimes of fs_aggregate;
                                                   its left-fold regime is fedopt_restatement.delta
  sigma = (z * S) * max_k q_k                      float64; z == 0: 0
  x'    = fl(fl(x + Delta) + fl(f32(sigma) * g))   z == 0: fl(x + Delta)
"""
import numpy as np

from tests import fedopt_restatement as FO
from tests import fold_restatement as FR

F32 = np.float32
F64 = np.float64
U32 = np.uint32
U64 = np.uint64
STATE = ('clip', 'sigma', 'b', 'dropped', 'clip_next')
G_MAX = float(np.sqrt(66.0 * np.log(2.0)))


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC 2011).  counter: four uint32 arrays (or scalars) of one shape, key:
    two uint32 scalars.  Returns four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(a)).astype(U64) for a in counter]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(a, shape).copy() for a in c]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    mask = U64(0xffffffff)
    for _ in range(10):
        p0 = U64(0xD2511F53) * c[0]
        p1 = U64(0xCD9E8D57) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ U64(k0), p1 & mask, (p0 >> U64(32)) ^ c[3] ^ U64(k1), p0 & mask]
        k0 = (k0 + 0x9E3779B9) & 0xffffffff
        k1 = (k1 + 0xBB67AE85) & 0xffffffff
    return [a.astype(U32) for a in c]


def seed_key(seed):
    seed = int(seed)
    return seed & 0xffffffff, (seed >> 32) & 0xffffffff


def unit(w):
    """u = (w + 0.5) * 2^-32 in float64, in (0, 1)."""
    return (w.astype(F64) + 0.5) * 2.0 ** -32


def pair(w0, w1):
    """Box-Muller in float64, each normal rounded once to float32."""
    rad = np.sqrt(-2.0 * np.log(unit(w0)))
    ang = 6.283185307179586 * unit(w1)
    return (rad * np.cos(ang)).astype(F32), (rad * np.sin(ang)).astype(F32)


def noise(seed, t, length, stream=0):
    """The field g [length] float32 of (seed, t, stream): float4 position j from the block at counter (j, t, stream, 0)."""
    assert length % 4 == 0
    j = np.arange(length // 4, dtype=U64)
    w = philox4x32_10((j, t, stream, 0), seed_key(seed))
    g = np.empty((length // 4, 4), F32)
    g[:, 0], g[:, 1] = pair(w[0], w[1])
    g[:, 2], g[:, 3] = pair(w[2], w[3])
    return g.reshape(-1)


def count_normal(seed, t):
    """g_b: the first normal of the block at counter (0, t, 1, 0)."""
    w = philox4x32_10((0, t, 1, 0), seed_key(seed))
    return pair(w[0], w[1])[0][0]


def updates(W, x):
    with np.errstate(all='ignore'):
        return (np.asarray(W, F32) - np.asarray(x, F32)[None, :]).astype(F32)


def norms(W, x):
    """n [M] float64: float32 squares summed in float64 (overflowing squares give Inf, as on the device)."""
    d = updates(W, x)
    with np.errstate(all='ignore'):
        return np.sum((d * d).astype(F32).astype(F64), axis=1)


def norms_exact(W, x):
    """The float64 sum of the exact squares of the float32 differences: what fs_dp_norms is held to."""
    d = updates(W, x).astype(F64)
    with np.errstate(all='ignore'):
        return np.sum(d * d, axis=1)


def weights(q, M):
    """q [M] float32; None: uniform, (float)(1.0 / M)."""
    return np.full(M, F32(1.0 / M), F32) if q is None else np.asarray(q, F32)


def clip_next(S, b, M, adaptive, seed=0, t=0):
    """S_{t+1} = S_t exp(-lr ((b + count_noise g_b) / M - quantile)) in float64; S_t without ``adaptive``."""
    if adaptive is None:
        return float(S)
    bt = float(b) + float(adaptive.get('count_noise', 0.0)) * float(count_normal(seed, t))
    return float(float(S) * np.exp(-(float(adaptive['lr']) * (bt / float(M) - float(adaptive['quantile'])))))


def coef(n, q, S, z, seed=0, t=0, adaptive=None):
    """(c [M] float32, r [M] float64, state dict) from the norms n [M] float64.  ``adaptive``:
    dict(quantile, lr, count_noise) or None."""
    n = np.asarray(n, F64)
    M = len(n)
    q = weights(q, M)
    S = float(S)
    with np.errstate(all='ignore'):
        finite = n <= np.finfo(F64).max
        r = np.sqrt(n)
        s = np.where(r <= S, 1.0, S / r)
        c = np.where(finite, (q.astype(F64) * s).astype(F32), F32(0)).astype(F32)
        under = finite & (r <= S)
    b = float(np.sum(under))
    sigma = 0.0 if z == 0 else (float(z) * S) * float(np.max(q))
    nxt = clip_next(S, b, M, adaptive, seed, t)
    state = dict(clip=S, sigma=float(sigma), b=b, dropped=float(np.sum(~finite)), clip_next=float(nxt))
    return c, r, state


def state_vector(state):
    return np.array([state[k] for k in STATE], F64)


def fold(W, x, c, chunks=0, ws_partials=None):
    """Delta: the regimes' fold of (c_k == 0 ? +0 : fl(c_k * fl(W_k - x)))."""
    d = updates(W, x)
    c = np.asarray(c, F32)
    zero = np.zeros(d.shape[1], F32)

    def term(k, first):
        with np.errstate(all='ignore'):
            return zero if c[k] == 0 else (c[k] * d[k]).astype(F32)
    with np.errstate(all='ignore'):
        return FR.fold(d.shape[0], chunks, ws_partials, term)


def fold_left(W, x, c):
    """The same through fedopt_restatement.delta (the left-fold regime, M < 16): dropped rows are replaced by
    x itself under coefficient 1, whose term is +0 -- the select."""
    W, c = np.array(W, F32), np.array(c, F32)
    x = np.asarray(x, F32)
    for k in np.flatnonzero(c == 0):
        W[k], c[k] = x, F32(1)
    return FO.delta(list(W), c, x, F32)


def finish(x, delta, sigma, g, z, cols=None):
    """``cols``: None, or (ld, D): the values are rows of ld of which the first D are parameters; the others
    take no noise term."""
    with np.errstate(all='ignore'):
        y = (np.asarray(x, F32) + np.asarray(delta, F32)).astype(F32)
        if z == 0:
            return y
        noisy = (y + (F32(sigma) * np.asarray(g, F32)).astype(F32)).astype(F32)
        if cols is None:
            return noisy
        return np.where(np.arange(len(y)) % int(cols[0]) < int(cols[1]), noisy, y)


def aggregate(W, x, q, S, z, seed=0, t=0, adaptive=None, chunks=0, ws_partials=None, n=None, c=None, g=None,
              cols=None):
    """dict(out, c, r, n, state, g).  ``n``, ``c`` or ``g`` given: that stage's device output is used instead of
    the restatement's own (the layered checks)."""
    W, x = np.asarray(W, F32), np.asarray(x, F32)
    n = norms(W, x) if n is None else np.asarray(n, F64)
    c0, r, state = coef(n, q, S, z, seed, t, adaptive)
    c = c0 if c is None else np.asarray(c, F32)
    if z != 0 and g is None:
        g = noise(seed, t, W.shape[1])
    out = finish(x, fold(W, x, c, chunks, ws_partials), state['sigma'], g, z, cols)
    return dict(out=out, c=c, r=r, n=n, state=state, g=g)


def adaptive_trajectory(r_rounds, S0, M, adaptive, seed=0, t0=0):
    """The clips S_0 .. S_R of the adaptive rule on given per-round norms r_rounds [R][M_t] (no dropped rows)."""
    S = [float(S0)]
    for t, r in enumerate(r_rounds):
        r = np.asarray(r, F64)
        with np.errstate(invalid='ignore'):
            b = float(np.sum(r <= S[-1]))
        S.append(clip_next(S[-1], b, M if np.isscalar(M) else M[t], adaptive, seed, t0 + t))
    return np.array(S)

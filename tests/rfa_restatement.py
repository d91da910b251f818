"""fs_aggregate_rfa restated in numpy, in exactly the orders of include/fedsim.h: the kernels equal it bit
for bit.  W = width(M) columns to a stripe.

  distance   a stripe's partial = 0.0 + (double)e_i^2 in ascending i, e_i = fl(W_k[i] - v[i]) in float32;
             32 slices over the stripes (s, s + 32, ...), the pairwise tree; sqrt in float64.
  weights    beta_k = alpha_k / max(nu, d_k) (finite d_k, else 0); B over 256 slices of k and the tree;
             b_k = f32(beta_k / B), all 0 when B is 0 or not finite.
  fold       256 / W slices of k, 0.0 + (double)b_k * (double)W_k[i] for b_k != 0, the tree, one rounding.

A term that is left out and a term of +0.0 give the same bits here: every sum starts at +0.0, so no partial
sum is ever -0.0 (x + (-x) and 0.0 + (-0.0) are +0.0 in round-to-nearest), and p + 0.0 == p otherwise."""
import numpy as np

F32, F64 = np.float32, np.float64

MAX_M = 5047            # fs_aggregate_rfa_max_m()
MAX_M32, MAX_M16 = 1261, 2523
NT = 256                # threads of a workgroup: slices of B and of the objective
RS = 32                 # slices over the stripes
MAX_ITERS = 32
INITS = ('start', 'mean')


def width(M):
    """fs_rfa_width: columns of a stripe."""
    assert 1 <= M <= MAX_M
    return 32 if M <= MAX_M32 else 16 if M <= MAX_M16 else 8


def stripes(M, length):
    return -(-int(length) // width(M))


def ws_bytes(M, length):
    """fs_aggregate_rfa_ws_bytes."""
    up = lambda v: (v + 15) & ~15
    return up(stripes(M, length) * M * 8) + up(M * 8) + 2 * up(length * 4) + 16


def tree(p):
    """p[j] += p[j + h] for j = 0, 2h, 4h, ..., h = 1, 2, 4, ... over axis 0 (a power of two long)."""
    p = np.array(p, dtype=F64)
    n, h = p.shape[0], 1
    assert n & (n - 1) == 0
    with np.errstate(all='ignore'):
        while h < n:
            p[0::2 * h] = p[0::2 * h] + p[h::2 * h]
            h *= 2
    return p[0]


def sliced_sum(t, n):
    """Slice s = 0.0 + t[s], t[s + n], ... in ascending order over axis 0, the n slices joined by the tree."""
    t = np.asarray(t, F64)
    p = np.zeros((n,) + t.shape[1:], F64)
    with np.errstate(all='ignore'):
        for k0 in range(0, t.shape[0], n):
            r = min(n, t.shape[0] - k0)
            p[:r] = p[:r] + t[k0:k0 + r]
    return tree(p)


def partials(W, v):
    """float64 [stripes, M]: every row's squared distance to v over each stripe."""
    W = np.ascontiguousarray(W, dtype=F32)
    v = np.asarray(v, dtype=F32)
    M, L = W.shape
    Wd = width(M)
    S = -(-L // Wd)
    with np.errstate(all='ignore'):
        e = (W - v[None, :]).astype(F32)
        e2 = np.zeros((M, S * Wd), F64)
        e2[:, :L] = e.astype(F64) * e.astype(F64)
        e2 = e2.reshape(M, S, Wd)
        acc = np.zeros((M, S), F64)
        for c in range(Wd):
            have = (np.arange(S) * Wd + c) < L
            acc = np.where(have[None, :], acc + e2[:, :, c], acc)
    return np.ascontiguousarray(acc.T)


def reduce_d2(part):
    """float64 [M] from the partial table [stripes, M]."""
    return sliced_sum(part, RS)


def d2_of(W, v):
    return reduce_d2(partials(W, v))


def weights(d2, alpha, nu, mean=False):
    """fs_rfa_weights from d2: (dist [M] f64, b [M] f32, objective f64, flag 0 / 1)."""
    d2 = np.asarray(d2, F64)
    a = np.asarray(alpha, F32).astype(F64)
    nu = float(nu)
    with np.errstate(all='ignore'):
        d = np.sqrt(d2)
        ok = np.isfinite(d)
        beta = np.where(ok, a if mean else a / np.maximum(nu, np.where(ok, d, 0.0)), 0.0)
        B = sliced_sum(beta, NT)
        h = np.where(d > nu, d, d * d / (2.0 * nu) + nu / 2.0)
        G = sliced_sum(np.where(ok, a * h, 0.0), NT)
        good = bool(B > 0.0 and np.isfinite(B))
        b = (beta / B).astype(F32) if good else np.zeros(len(d), F32)
    return d, b, (float(G) if ok.any() else float('nan')), (0 if good else 1)


def fold(W, b):
    """float32 [len]: the fold of the rows with b_k != 0."""
    W = np.ascontiguousarray(W, dtype=F32)
    b = np.asarray(b, F32)
    T = NT // width(W.shape[0])
    with np.errstate(all='ignore'):
        t = np.where((b != 0)[:, None], b.astype(F64)[:, None] * W.astype(F64), 0.0)
        return sliced_sum(t, T).astype(F32)


def step(W, v, b=None, flag=0):
    """fs_rfa_step: (v' float32 [len], the partial table).  b None: pass 0."""
    vn = np.array(v, dtype=F32) if (b is None or flag) else fold(W, b)
    return vn, partials(W, vn)


def chain(W, x, alpha, T=3, nu=1e-6, init='start', step_b=None):
    """fs_aggregate_rfa: dict(out, dist, b, obj [T + 2], iterates, bs).  ``step_b``: a list of the weights to
    use at each fold instead of the restated ones (a device's own, to follow its chain step by step)."""
    assert 0 <= T <= MAX_ITERS and nu > 0 and init in INITS
    mean = init == 'mean'
    nfold = T + (1 if mean else 0)
    obj = np.full(T + 2, np.nan, F64)
    v, b, flag, d, its, bs = None, None, 0, None, [], []
    for i in range(nfold + 1):
        if i == 0:
            v, part = step(W, x)
        else:
            v, part = step(W, v, b if step_b is None else step_b[i - 1], flag)
        its.append(v)
        d, bn, obj[i], fn = weights(reduce_d2(part), alpha, nu, mean and i == 0)
        if i < nfold or nfold == 0:
            b, flag = bn, fn
            bs.append(bn)
    return dict(out=v, dist=d, b=b, obj=obj, iterates=its, bs=bs)


# ---- inputs ----

KINDS = ('normal', 'equal', 'zeros', 'mixed')


def inputs(kind, M, length, seed=0):
    """(W float32 [M, len], x float32 [len], alpha float32 [M]) of one kind.  'normal': model plus noise;
    'equal': every row the same and equal to x (all distances 0: the nu branch); 'zeros': +-0 only; 'mixed':
    magnitudes from 1e-30 to 1e30."""
    rs = np.random.RandomState(1000 * seed + 7 * M + length)
    x = rs.normal(size=length).astype(F32)
    if kind == 'normal':
        W = (x[None, :] + 0.05 * rs.normal(size=(M, length)) + 0.02 * rs.normal(size=length)[None, :]).astype(F32)
    elif kind == 'equal':
        W = np.repeat(x[None, :], M, 0).astype(F32)
    elif kind == 'zeros':
        W = np.where(rs.rand(M, length) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
        x = np.where(rs.rand(length) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    elif kind == 'mixed':
        W = (rs.normal(size=(M, length)) * 10.0 ** rs.uniform(-30, 30, size=(M, length))).astype(F32)
    else:
        raise ValueError(kind)
    alpha = rs.dirichlet(np.full(M, 5.0)).astype(F32)
    return W, x, alpha


ATTACKS = ('sign_flip', 'gaussian', 'nan', 'inf', 'huge')
ATTACK_CASES = ((5, 36, 1), (12, 132, 2), (12, 132, 5), (65, 36, 20), (257, 132, 100))


def attacked(M, length, bad, attack, seed=0):
    """(W, x, alpha, bad ids): model-plus-noise rows, ``bad`` of them replaced: sign_flip x 10, gaussian x 10,
    NaN rows, Inf in every third element, rows of 1e30.  alpha: Dirichlet(5), uniform where the draw would put
    more than 0.45 of the weight on the bad rows."""
    rs = np.random.RandomState(77 + 1000 * seed + 31 * M + length + bad)
    x = rs.normal(size=length).astype(F32)
    W = (x[None, :] + 0.05 * rs.normal(size=(M, length)) + 0.02 * rs.normal(size=length)[None, :]).astype(F32)
    ids = np.sort(rs.choice(M, bad, replace=False))
    if attack == 'sign_flip':
        W[ids] = (x[None, :] - 10.0 * (W[ids] - x[None, :])).astype(F32)
    elif attack == 'gaussian':
        W[ids] = (x[None, :] + 10.0 * rs.normal(size=(bad, length))).astype(F32)
    elif attack == 'nan':
        W[ids] = np.nan
    elif attack == 'inf':
        W[np.ix_(ids, np.arange(0, length, 3))] = np.inf
    elif attack == 'huge':
        W[ids] = F32(1e30)
    else:
        raise ValueError(attack)
    alpha = rs.dirichlet(np.full(M, 5.0)).astype(F32)
    if alpha[ids].astype(F64).sum() / alpha.astype(F64).sum() > 0.45:
        alpha = np.full(M, F32(1.0 / M), F32)
    return W, x, alpha, ids


def weiszfeld64(W, alpha, v0, iters=300, nu=1e-6):
    """A plain float64 smoothed Weiszfeld run over finite rows: the iterates r_0 = v0, r_1, ..., r_iters."""
    W = np.asarray(W, F64)
    a = np.asarray(alpha, F64)
    its = [np.asarray(v0, F64)]
    for _ in range(iters):
        d = np.sqrt(((W - its[-1][None, :]) ** 2).sum(1))
        w = a / np.maximum(nu, d)
        its.append((w[:, None] * W).sum(0) / w.sum())
    return its

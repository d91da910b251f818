"""A float64 reference of local training (fs_local_train) and of the p-solve (fs_mix_solve), and
inputs that leave only the softmax to go wrong (tests/test_gpu_softmax.py; the inputs themselves
are proven on the CPU in tests/test_softmax_reference.py).

``train_ref64``    oracle.fedsim_oracle.train_client restated in float64: the same pass_order
                   draws, the same batch loop, the same zero-norm rule; log-sum-exp with the
                   maximum subtracted.
``solve_ref64``    the same restatement of mixture_solve_z.
``train_problem``  clients whose first-step logits are exact in fp32 in any summation order
                   (small integers times a power of two, as eval_reference.exact_problem) and whose
                   batch rows sit at the common offsets 0, +-64 and +-128 (column 0 carries them).
                   'saturated': every row is won by about 256, so exp(z - m) is exactly 0 in fp32 for
                   every loser, the gradient entries are exactly +-1/b or 0 and -- b a power of two,
                   lr a power of two -- the whole step is exact in fp32, whatever the order of the
                   sums: the kernel's weights are compared bitwise.  'all_won': the same with every
                   row labelled with its winner (no step moves anything).  'mixed': saturated rows
                   (won by 120), rows whose logits all tie exactly, and plain rows, side by side in
                   ragged clients; compared within the project's fp32 bounds.
``z_problem``      the same three kinds of rows as validation logits Z [N, C, nv], at the offsets the
                   training logits see (0, +-64, +-128), with a dyadic p that sums to exactly 1
                   (zero and negative entries included).  Rows at -128 have every logit below -104:
                   a softmax that takes a padded class slot's 0 into its maximum underflows there
                   (at -64 it would only lose bits: a softmax is invariant under a common shift).
``*_CASES``        the cases of tests/test_gpu_softmax.py, shared with the CPU tests that prove
                   them: a 'mixed' case is admitted only if the fp32 oracle stays within a quarter
                   of the bound the GPU test asserts (``QUARTER``) -- a tolerance must not hide an
                   ill-conditioned case.
"""
import numpy as np

from oracle import fedsim_oracle as O

OFFSETS = (0.0, 32.0, -32.0, 64.0, -64.0)          # column 0 of X; W0[:, 0] = 2 doubles them in the logits
Z_OFFSETS = (0.0, 64.0, -64.0, 128.0, -128.0)      # of the validation logits: the same five, as the logits see them
TOL = 2e-5               # local training: |W - W_ref| <= TOL max(1, |W_ref|max), loss alike
P_TOL, BUF_TOL = 1e-5, 1e-4   # p-solve: relative to the largest reference entry
QUARTER = 0.25           # the fp32 oracle's share of a bound, at most, on every 'mixed' case
MU, LAM = 0.03, 0.002
LR_SAT = 2.0 ** -6       # saturated training: a power of two, the step stays exact
LR_P_SAT = 2.0 ** -10
LR_P_MIXED = 2.0 ** -14
# A saturated row starts about 256 ahead (GAP_START, asserted on every problem's first step).
# Training wears the lead down: a visit of a row with winner w labelled y takes lr / b * 64 = 2^-5
# from W[w, 1 + w] and adds it to W[y, 1 + w] -- 2 off the lead of every row won by w, 4 against y
# -- and moves column 0 by lr / b * offset, up to +-4 more between rows at +-64.  Half the rows
# carry random labels, so at C = 2 a 32-row batch costs each winner about 16 per step and no
# client of two batches keeps 200 through two epochs (measured 163 .. 186 over 8 draws at
# (n, D, C, B) = (64, 64, 2, 32); chained clients add up).  What exactness needs is less:
# exp(x) is exactly 0 in fp32 for x <= -104 (2^-150 = e^-103.97 rounds to 0, denormals or not),
# and from the second step on the fp32 logits carry rounding of at most 2^-24 * 400 * D terms < 1.
# GAP_EXACT = 128 leaves 24 for it, and is asserted over every step of every saturated case.
GAP_START, GAP_EXACT = 200.0, 128.0


# --------------------------------------------------------------------------- references
def _f32(v):
    """The hyper-parameter as the kernels and the oracle receive it: rounded to float32."""
    return float(np.float32(v))


def _top2_gap(z):
    if z.shape[1] < 2 or z.shape[0] == 0:
        return np.inf
    t = np.partition(z, z.shape[1] - 2, axis=1)
    return float((t[:, -1] - t[:, -2]).min())


def train_ref64(X, y, W0, lr, E, B, prox, mu, reg, lam):
    """train_client in float64.  Returns (W float64, last-epoch mean loss, the least gap between
    the two largest logits of a row over all steps -- inf at C = 1 or without rows)."""
    X = np.asarray(X, np.float64)
    y = np.asarray(y, np.int64)
    W = np.array(W0, dtype=np.float64, copy=True)
    Wa = W.copy()
    lr, mu, lam = _f32(lr), _f32(mu), _f32(lam)
    n = len(y)
    avg, gap = 0.0, np.inf
    for _ in range(E):
        order = O.pass_order(n)
        s, cnt = 0.0, 0
        for b0 in range(0, n, B):
            idx = order[b0:b0 + B]
            xb, yb = X[idx], y[idx]
            b = len(idx)
            z = xb @ W.T
            gap = min(gap, _top2_gap(z))
            m = z.max(axis=1, keepdims=True)
            lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
            loss = float((lse[:, 0] - z[np.arange(b), yb]).mean())
            g = np.exp(z - lse)
            g[np.arange(b), yb] -= 1.0
            g /= b
            grad = g.T @ xb
            if prox:
                dw = W - Wa
                pn = np.sqrt(np.sum(dw * dw))
                loss += mu * pn
                if pn > 0:
                    grad = grad + mu * (dw / pn)
            if reg:
                wn = np.sqrt(np.sum(W * W))
                loss += lam * wn
                if wn > 0:
                    grad = grad + lam * (W / wn)
            W = W - lr * grad
            s += loss * b
            cnt += b
        avg = s / cnt if cnt else 0.0
    return W, avg, gap


def solve_ref64(Z, y, p, buf, lr, epochs, Bv, momentum=0.9):
    """mixture_solve_z in float64 on Z [N, C, nv].  Returns (p, buf) in float64."""
    Zt = np.ascontiguousarray(np.asarray(Z, np.float64).transpose(2, 0, 1))      # [nv, N, C]
    y = np.asarray(y, np.int64)
    p = np.array(p, dtype=np.float64, copy=True)
    buf = None if buf is None else np.array(buf, dtype=np.float64, copy=True)
    lr, mom = _f32(lr), _f32(momentum)
    nv = len(y)
    for _ in range(epochs):
        order = O.pass_order(nv)
        for b0 in range(0, nv, Bv):
            idx = order[b0:b0 + Bv]
            b = len(idx)
            zb = Zt[idx]
            out = np.einsum('bnc,n->bc', zb, p)
            m = out.max(axis=1, keepdims=True)
            lse = m + np.log(np.exp(out - m).sum(axis=1, keepdims=True))
            g = np.exp(out - lse)
            g[np.arange(b), y[idx]] -= 1.0
            g /= b
            gp = np.einsum('bc,bnc->n', g, zb)
            buf = gp if buf is None else mom * buf + gp
            p = p - lr * buf
    return p, buf


def train_chain_ref64(Xs, ys, W0, lr, E, B, prox, mu, reg, lam, chained):
    """Every client through train_ref64 (client-major draws, as the launch's shuffles): chained
    clients start from the previous client's float64 result, parallel ones from W0.
    Returns ([W], [loss], least gap)."""
    Ws, losses, gap = [], [], np.inf
    start = np.asarray(W0, np.float64)
    for X, y in zip(Xs, ys):
        W, l, g = train_ref64(X, y, start, lr, E, B, prox, mu, reg, lam)
        Ws.append(W)
        losses.append(l)
        gap = min(gap, g)
        if chained:
            start = W
    return Ws, losses, gap


def train_chain_f32(Xs, ys, W0, lr, E, B, prox, mu, reg, lam, chained):
    """The fp32 oracle over the same clients, the same draws."""
    Ws, losses = [], []
    start = W0
    for X, y in zip(Xs, ys):
        W, l = O.train_client(X, y, start, lr, E, B, prox, mu, reg, lam)
        Ws.append(W)
        losses.append(l)
        if chained:
            start = W
    return Ws, losses


# --------------------------------------------------------------------------- inputs
def _labels_mixed(rs, n, C):
    """Labels of a 'mixed' run of n rows: random, class 0 on row 0 and C - 1 on row 2 (plain
    rows); saturated rows (i % 3 == 1) labelled with the winner C // 2 where i % 6 == 1 and with a
    loser where i % 6 == 4."""
    y = rs.randint(0, C, size=n).astype(np.int64)
    if n > 0:
        y[0] = 0
    if n > 2:
        y[2] = C - 1
    i = np.arange(n)
    w = C // 2
    y[i % 6 == 1] = w
    lose = i % 6 == 4
    if C >= 2:
        y[lose] = (w + 1 + rs.randint(0, C - 1, size=int(lose.sum()))) % C
    return y


def _labels_saturated(rs, win, C, all_won):
    """Even rows labelled with the winner; odd rows at random, row 1 with a loser."""
    y = win.copy()
    n = len(win)
    if not all_won and C >= 2:
        odd = np.arange(n) % 2 == 1
        y[odd] = rs.randint(0, C, size=int(odd.sum()))
        if n > 1:
            y[1] = (win[1] + 1) % C
    return y


def _winners(rs, n, C):
    win = rs.randint(0, C, size=n).astype(np.int64)
    if n > 0:
        win[0] = 0
    if n > 2:
        win[2] = C - 1
    return win


def train_problem(rs, sizes, D, C, kind, offset=1.0):
    """(Xs, ys, W0) of the given kind ('saturated', 'mixed', 'all_won'); D >= C + 2.  ``offset``
    scales the common offsets of the rows (a power of two)."""
    assert D >= C + 2 and kind in ('saturated', 'mixed', 'all_won')
    kx = int(np.round(np.log2(2.0 * np.sqrt(D))))
    Wi = rs.randint(-3, 4, size=(C, D)).astype(np.float64)
    W0 = Wi * 2.0 ** -(5 - kx)
    W0[:, 0] = 2.0
    if kind == 'mixed':
        W0[:, 1] = 0.0
        W0[C // 2, 1] = 2.5
    else:
        W0[:, 1:1 + C] = 0.0
        W0[np.arange(C), 1 + np.arange(C)] = 4.0
    Xs, ys = [], []
    for n in sizes:
        X = rs.randint(-3, 4, size=(n, D)).astype(np.float64) * 2.0 ** -kx
        i = np.arange(n)
        X[:, 0] = np.asarray(OFFSETS)[i % 5] * offset
        if kind == 'mixed':
            X[:, 1] = np.where(i % 3 == 1, 48.0, 0.0)
            X[i % 7 == 3, 1:] = 0.0
            y = _labels_mixed(rs, n, C)
        else:
            win = _winners(rs, n, C)
            X[:, 1:1 + C] = 0.0
            X[i, 1 + win] = 64.0
            y = _labels_saturated(rs, win, C, kind == 'all_won')
        Xs.append(X.astype(np.float32))
        ys.append(y)
    return Xs, ys, W0.astype(np.float32)


def dyadic_p(rs, N):
    """p0 [N] float32: integers over a power of two that sum to exactly 1, with an entry that
    is 0 and one that is negative wherever N >= 4.  Returns (p0, sum of |numerators|, denominator)."""
    if N == 1:
        return np.ones(1, np.float32), 1, 1
    k = rs.randint(1, 4, size=N).astype(np.int64)
    fixed = np.zeros(N, bool)
    if N >= 4:
        k[1], k[N - 2] = 0, -1
        k[3::7] = -1
        k[5::11] = 0
        fixed[1] = fixed[N - 2] = True
        fixed[3::7] = True
        fixed[5::11] = True
    den = 8
    while den < k.sum():
        den *= 2
    free = np.nonzero(~fixed)[0]
    r = den - int(k.sum())
    k[free] += r // len(free)
    k[free[:r % len(free)]] += 1
    assert k.sum() == den
    p = (k / float(den)).astype(np.float32)
    assert float(p.astype(np.float64).sum()) == 1.0
    return p, int(np.abs(k).sum()), den


def z_problem(rs, N, C, nv, kind, offset=1.0):
    """(Z [N, C, nv] float32, y [nv], p0 [N] float32) of the given kind ('saturated', 'mixed').
    Z is quarters plus the row's offset; p0 is dyadic and sums to exactly 1, so a logit
    sum_n p_n Z[n, c, v] is the row's offset plus a small term, exactly, and every partial sum of
    it stays below 2^24 quanta: exact in fp32 in any summation order."""
    assert kind in ('saturated', 'mixed')
    Z = rs.randint(-3, 4, size=(N, C, nv)).astype(np.float64) * 0.25
    v = np.arange(nv)
    Z += (np.asarray(Z_OFFSETS)[v % 5] * offset)[None, None, :]
    if kind == 'saturated':
        win = _winners(rs, nv, C)
        Z[:, win, v] += 256.0
        y = _labels_saturated(rs, win, C, False)
    else:
        sat = v % 3 == 1
        Z[:, C // 2, sat] += 120.0
        tie = v % 7 == 3
        Z[:, :, tie] = (np.asarray(Z_OFFSETS)[v[tie] % 5] * offset)[None, None, :]
        y = _labels_mixed(rs, nv, C)
    p0, mass, den = dyadic_p(rs, N)
    assert mass * 4 * np.abs(Z).max() * 4 < 2 ** 24      # quanta of 1 / (4 den): every partial sum
    return Z.astype(np.float32), y, p0


# --------------------------------------------------------------------------- cases
# (form, G, D, C, B): the forms of fs_local_train and the smallest shapes at which each one's
# softmax takes another path (class tiles, lane groups of 2 .. 32, weights in LDS or in HBM)
SAT_SINGLE = [(64, 1, 32), (64, 2, 32), (64, 3, 16), (200, 10, 32), (130, 17, 32), (64, 26, 64), (4000, 10, 32)]
SAT_TRAIN_CASES = (
    [('single', 1, D, C, B) for D, C, B in SAT_SINGLE]
    + [('split', G, 1000, C, 32) for G in (2, 4, 8, 16) for C in (3, 10, 16)]
    + [('mb', 2, 2024, C, 32) for C in (3, 10, 16)]
    + [('teams', 4, 2024, 10, 32), ('pair', 2, 1000, 10, 32), ('pipe', 2, 2024, 10, 32), ('dbuf', 2, 2024, 10, 32)])
MIXED_TRAIN_CASES = (
    [('single', 1, 200, 3, 16), ('single', 1, 200, 10, 32), ('single', 1, 130, 17, 32), ('single', 1, 64, 26, 64)]
    + [('split', G, 1000, 10, 32) for G in (2, 4, 8, 16)]
    + [('mb', 2, 2024, 10, 32), ('teams', 4, 2024, 10, 32), ('pair', 2, 1000, 10, 32), ('pipe', 2, 2024, 10, 32),
       ('dbuf', 2, 2024, 10, 32)])
BITWISE_SPLIT_FORMS = ('pair', 'pipe', 'dbuf')      # held bitwise to the split form at the same width
PARALLEL_ONLY_FORMS = ('pair', 'teams')


def split_fits(G, C, B=32):
    """The split form exchanges at most 512 values per step at G >= 8 (B rows x C classes and
    the two norms): wider class counts have no instance there and the planner refuses them."""
    return G < 8 or B * C + 2 <= 512


def train_case_seed(form, G, D, C, B, kind):
    return (G * 7919 + D * 1009 + C * 31 + B + len(form) * 100003 + len(kind)) % (2 ** 31 - 1)


def sat_sizes(B):
    """Client sizes of a saturated case: one full batch each (b a power of two; two steps per
    client -- every visit of a row labelled with a loser costs the rows of its winner 2 to 8 of
    their lead, see GAP_EXACT), the third client 'all_won'."""
    return [B, B, B, B]


ALL_WON_CLIENT = 2


def mixed_sizes(B):
    """Ragged client sizes of a mixed case: n % B in {1, 7, B - 3}, at most 128 rows."""
    if B >= 64:
        return [B + 1, B + 7, 2 * B - 3, B - 3]
    return [2 * B + 1, 3 * B + 7, 2 * B - 3, B + 1]


def saturated_train_inputs(form, G, D, C, B):
    """(Xs, ys, W0) of one saturated case: four clients, the third one 'all_won'."""
    rs = np.random.RandomState(train_case_seed(form, G, D, C, B, 'saturated'))
    sizes = sat_sizes(B)
    Xs, ys, W0 = train_problem(rs, sizes, D, C, 'saturated')
    j = ALL_WON_CLIENT
    Xa, ya, _ = train_problem(rs, [sizes[j]], D, C, 'all_won')
    Xs[j], ys[j] = Xa[0], ya[0]
    return Xs, ys, W0


def mixed_train_inputs(form, G, D, C, B):
    rs = np.random.RandomState(train_case_seed(form, G, D, C, B, 'mixed'))
    return train_problem(rs, mixed_sizes(B), D, C, 'mixed')


def mixed_terms(case):
    """Prox and ridge on in every other mixed case."""
    return MIXED_TRAIN_CASES.index(case) % 2 == 1


# (form, G, D, C, B) -> lr, where lr = 2^-6 misses QUARTER (the fp32 oracle at 0.29, 0.60 and 0.60
# of the bound: at offsets of +-128 and lr = 2^-6 the offset column itself trains at the edge of
# stability); at half the lr these sit at 0.02 to 0.07, the offsets untouched
MIXED_TRAIN_LR = {('single', 1, 130, 17, 32): 2.0 ** -7, ('pipe', 2, 2024, 10, 32): 2.0 ** -7,
                  ('dbuf', 2, 2024, 10, 32): 2.0 ** -7}


def mixed_train_lr(case):
    return MIXED_TRAIN_LR.get(tuple(case), LR_SAT)

# (solver, N, C, Bv, tuning): one saturated step, nv == Bv
SAT_SOLVE_CASES = (
    [('bin', N, 2, 16, dict(mix_exact_softmax=e)) for N in (10, 1) for e in (0, 1)]
    + [('wave', 16, 4, 16, {})]
    + [('quad', N, C, Bv, dict(mix_exact_softmax=e)) for N, C, Bv in ((100, 10, 16), (64, 7, 16), (37, 16, 16), (5, 3, 8))
       for e in (0, 1)]
    + [('reg', 37, 20, 16, {}), ('reg2', 200, 4, 16, {}), ('staged', 23, 5, 32, {}), ('global', 19, 24, 32, {}),
       ('mc', 300, 4, 16, {}), ('mc', 1000, 10, 16, {}), ('qmc', 300, 4, 16, {}),
       ('qmc', 1000, 10, 16, dict(mix_qmc_lane_clients=4)), ('qmc', 1000, 10, 16, dict(mix_qmc_lane_clients=8))])

# (solver, N, C, nv, Bv, tuning): 2 rounds of 2 epochs, nv % Bv != 0
MIXED_SOLVE_CASES = [
    ('bin', 10, 2, 203, 16, {}), ('wave', 16, 4, 77, 16, {}), ('quad', 5, 3, 40, 7, {}), ('quad', 100, 10, 77, 16, {}),
    ('reg', 37, 20, 90, 16, {}), ('reg2', 200, 4, 77, 16, {}), ('staged', 23, 5, 200, 24, {}),
    ('global', 19, 24, 70, 20, {}), ('mc', 300, 4, 60, 16, {}), ('mc', 1000, 10, 97, 16, {}),
    ('qmc', 300, 4, 60, 16, {}), ('qmc', 1000, 10, 97, 16, {})]
# (N, C, nv, Bv) -> (offset scale, lr_p) where the full offsets at LR_P_MIXED miss QUARTER
# (the fp32 oracle's share of the bound: staged 1.05 at 2^-14, 0.02 at 2^-15; N = 1000 2.3 at the full
# offsets, 6.4 at half, 0.92 at a quarter, 0.23 at a quarter and 2^-15 -- there the +-32 rows no
# longer underflow a softmax whose maximum is 0, the N <= 300 cases of each solver family do)
MIXED_SOLVE_SCALE = {(23, 5, 200, 24): (1.0, 2.0 ** -15), (1000, 10, 97, 16): (0.25, 2.0 ** -15)}


def solve_case_seed(N, C, nv, Bv):
    return (N * 1000003 + C * 1009 + nv * 31 + Bv) % (2 ** 31 - 1)


def saturated_solve_inputs(N, C, Bv):
    return z_problem(np.random.RandomState(solve_case_seed(N, C, Bv, Bv)), N, C, Bv, 'saturated')


def mixed_solve_inputs(N, C, nv, Bv):
    """(Z, y, p0, lr_p) of one mixed p-solve case."""
    off, lr = MIXED_SOLVE_SCALE.get((N, C, nv, Bv), (1.0, LR_P_MIXED))
    Z, y, p0 = z_problem(np.random.RandomState(solve_case_seed(N, C, nv, Bv)), N, C, nv, 'mixed', offset=off)
    return Z, y, p0, lr


def id_of(case):
    return '-'.join('+'.join('%s%d' % kv for kv in sorted(x.items())) or 'default' if isinstance(x, dict) else str(x)
                    for x in case)

"""CPU restatement of SCAFFOLD (Karimireddy et al., ICML 2020, option II) in numpy, with a dtype
argument: float32 is what the GPU kernels compute, float64 the exact evaluation the drift bounds
are measured against (tests/golden/make_golden_scaffold.py writes scaffold_drift.json, the method of
mse_drift.json).  Not in the reference: the step is the reference's train_loop step
(oracle.fedsim_oracle.train_client, restated here with one more gradient term), everything else
-- pass_order, mlp_init, lr_schedule, test_eval -- comes from the oracle unchanged.

State: server model x [C, D], server variate c [C, D], client variates c_i [N, C, D], all variates
zero before round 0.  Round t with the sample S (ascending ids; every client without ``sched``) at
the round's learning rate lr:

  client i in S   y = x; K_i = E*ceil(n_i/B) steps with grad = fl(grad_CE + d), d = fl(c - c_i) fixed
                  for the whole client, then the ridge term, then y -= lr*grad; the loss is
                  train_client's (the correction is no part of it).  Then
                  c_i <- fl(fl(c_i - c) + fl(fl(x - y) * inv)),  inv = 1 / fl(K_i * lr)
  server          x <- fl(x + sum_S fl(q_k * fl(y_k - x))),  c <- fl(fl(cs*c) + sum_S fl(r_k * fl(x - y_k)))
                  as left folds in ascending k, the first term the term itself,
                  q_k = server_lr * p_k / sum_S p,  r_k = p_k / (K_k lr),  cs = 1 - sum_S p_k
                  (exactly 0 when S is every client) -- float64 host scalars rounded once to float32
                  (the float64 run keeps them unrounded).  p_i = n_i / n ('size') or 1 / N ('uniform').
  train_loss[t] = sum_S (p_k / sum_S p) loss_k.
"""
import numpy as np

from oracle import fedsim_oracle as O

F32 = np.float32
F64 = np.float64


def weights(ns, weighting='size'):
    """p (float64) over all clients."""
    ns = np.asarray(ns, dtype=F64)
    if weighting == 'uniform':
        return np.ones(len(ns)) / len(ns)
    if weighting != 'size':
        raise ValueError("weighting must be 'size' or 'uniform'")
    return ns / ns.sum()


def steps(ns, epoch, batch_size):
    ns = np.asarray(ns, dtype=np.int64)
    return epoch * ((ns + batch_size - 1) // batch_size)


def round_coefficients(ns, S, epoch, batch_size, lr, server_lr=1.0, weighting='size', dtype=F32):
    """(q, r, cs, w) of one round: float64 arithmetic, rounded once to float32 and carried in
    ``dtype`` (float64: unrounded)."""
    S = np.asarray(S, dtype=np.int64)
    p = weights(ns, weighting)[S]
    tot = float(p.sum())
    K = steps(np.asarray(ns)[S], epoch, batch_size).astype(F64)
    q, r, w = server_lr * p / tot, p / (K * float(lr)), p / tot
    cs = 0.0 if len(S) == len(ns) else 1.0 - tot
    if dtype == F64:
        return q, r, cs, w
    return q.astype(F32).astype(dtype), r.astype(F32).astype(dtype), dtype(F32(cs)), w.astype(F32).astype(dtype)


def train_client(X, y, W, lr, epoch, batch_size, reg, lam, c, ci, dtype=F32):
    """One client's local training from W with the variates (c, c_i).  Returns
    (y, last-epoch mean loss, new c_i).  With c = c_i = 0 bitwise O.train_client (no prox)."""
    T = dtype
    X = np.asarray(X, dtype=T)
    y = np.asarray(y, dtype=np.int64)
    x0 = np.array(W, dtype=T, copy=True)
    W = x0.copy()
    c, ci = np.asarray(c, dtype=T), np.asarray(ci, dtype=T)
    d = (c - ci).astype(T)
    lrT, lamT = T(lr), T(lam)
    n = len(y)
    avg, K = 0.0, 0
    for _ in range(epoch):
        order = O.pass_order(n)
        s, cnt = 0.0, 0
        for b0 in range(0, n, batch_size):
            idx = order[b0:b0 + batch_size]
            xb, yb = X[idx], y[idx]
            bsz = len(idx)
            z = xb @ W.T
            m = z.max(axis=1, keepdims=True)
            se = np.exp(z - m).sum(axis=1, keepdims=True, dtype=T)
            logp = (z - m - np.log(se)).astype(T)
            ce = T(-logp[np.arange(bsz), yb].mean(dtype=T))
            g = np.exp(logp).astype(T)
            g[np.arange(bsz), yb] -= T(1.0)
            g /= T(bsz)
            grad = (g.T @ xb).astype(T)
            grad = (grad + d).astype(T)                    # the control-variate correction
            loss = ce
            if reg:
                wn = T(np.sqrt(np.sum(W * W, dtype=T)))
                loss = T(loss + lamT * wn)
                if wn > 0:
                    grad = grad + lamT * (W / wn)
            W = (W - lrT * grad.astype(T)).astype(T)
            s += float(loss) * bsz
            cnt += bsz
            K += 1
        avg = s / cnt if cnt else 0.0
    if K == 0:
        return W, 0.0, ci.copy()
    return W, avg, variate(ci, c, x0, W, K, lr, T)


def variate(ci, c, x, y, K, lr, dtype=F32):
    """Option II's new client variate, every operation rounded to ``dtype``."""
    T = dtype
    inv = T(T(1.0) / T(T(K) * T(lr)))
    return ((np.asarray(ci, T) - np.asarray(c, T)).astype(T)
            + ((np.asarray(x, T) - np.asarray(y, T)).astype(T) * inv).astype(T)).astype(T)


def server(x, c, Ws, q, r, cs, dtype=F32):
    """The two left folds of fs_aggregate_scaffold.  Returns (x_new, c_new)."""
    T = dtype
    x, c = np.asarray(x, T), np.asarray(c, T)
    q, r = np.asarray(q, T), np.asarray(r, T)
    aw = ac = None
    for k in range(len(Ws)):
        wk = np.asarray(Ws[k], T)
        tw = (q[k] * (wk - x).astype(T)).astype(T)
        tc = (r[k] * (x - wk).astype(T)).astype(T)
        aw = tw if aw is None else (aw + tw).astype(T)
        ac = tc if ac is None else (ac + tc).astype(T)
    return (x + aw).astype(T), ((T(cs) * c).astype(T) + ac).astype(T)


def scaffold(Xs, ys, Xt, yt, num_classes=10, D=200, lr=0.01, epoch=2, batch_size=32, reg=False, lam=0.01, R=100,
             sched=None, server_lr=1.0, weighting='size', dtype=F32):
    """Returns (train_loss[R], test_loss[R], test_acc[R], {'W': [R, C, D], 'c': [R, C, D],
    'ci': [R, N, C, D]}).  Draws from torch's global generator as FedAvg with parallel clients and
    the same sample does (MLP init, then per round the sampled clients' passes and the test pass):
    seed it first."""
    T = dtype
    saved = O.F32
    O.F32 = T                      # the oracle's working type (test_eval, mlp_init)
    try:
        ns = np.array([len(y) for y in ys])
        N = len(ns)
        Xs = [np.asarray(x, T) for x in Xs]
        ys = [np.asarray(y, np.int64).reshape(-1) for y in ys]
        Xt, yt = np.asarray(Xt, T), np.asarray(yt, np.int64).reshape(-1)
        Wg = O.mlp_init(D, num_classes).astype(T)
        c = np.zeros((num_classes, D), T)
        ci = np.zeros((N, num_classes, D), T)
        tr, tl, ta = np.zeros(R), np.zeros(R), np.zeros(R)
        Wt, ct, cit = [], [], []
        for t in range(R):
            lr = O.lr_schedule(t, lr, R)
            S = np.arange(N) if sched is None else np.asarray(sched[t])
            Ws, losses = [], []
            for j in S:
                W, l, cj = train_client(Xs[j], ys[j], Wg, lr, epoch, batch_size, reg, lam, c, ci[j], T)
                ci[j] = cj
                Ws.append(W)
                losses.append(l)
            q, r, cs, w = round_coefficients(ns, S, epoch, batch_size, lr, server_lr, weighting, T)
            tr[t] = np.sum(w * np.asarray(losses, dtype=F32).astype(T), dtype=T)
            Wg, c = server(Wg, c, Ws, q, r, cs, T)
            Wt.append(Wg.copy())
            ct.append(c.copy())
            cit.append(ci.copy())
            tl[t], ta[t] = O.test_eval(Xt, yt, Wg, batch_size)
        return tr, tl, ta, {'W': np.stack(Wt), 'c': np.stack(ct), 'ci': np.stack(cit)}
    finally:
        O.F32 = saved


# ---- the drop-in cases (tests/test_gpu_scaffold.py, tests/golden/make_golden_scaffold.py) ---------
SIZES = [21, 8, 37, 5, 16, 12]          # N = 6 unequal clients: one below B, short last batches
D, C, R, E, B, LR, LAM = 64, 4, 3, 2, 8, 0.5, 0.001
SCHED = [np.array([0, 2, 5]), np.array([1, 2, 3]), np.array([0, 4, 5])]    # M = 3, three distinct samples
TORCH_SEED = 100
CASES = {'%s_%s_eta%g' % (part, wt, eta): dict(sched=SCHED if part == 'sampled' else None, weighting=wt, server_lr=eta)
         for part in ('full', 'sampled') for wt in ('size', 'uniform') for eta in (1.0, 0.5)}


def case_data():
    """The inputs of every drop-in case: random-feature rows with a label skew across the clients."""
    rs = np.random.RandomState(77)
    n, nt = sum(SIZES), 40
    raw = rs.normal(size=(n + nt, 10)).astype(F32)
    phi = (np.cos(raw @ rs.normal(0, 0.7, size=(10, D)).astype(F32) + rs.uniform(0, 2 * np.pi, size=(1, D)).astype(F32))
           / np.sqrt(D)).astype(F32)
    lab = np.argmax(phi @ rs.normal(size=(D, C)).astype(F32) + 0.1 * rs.normal(size=(n + nt, C)), axis=1).astype(np.int64)
    order = np.argsort(lab[:n] + 1.5 * rs.normal(size=n), kind='stable')     # non-IID: clients sorted along the label
    off = np.concatenate([[0], np.cumsum(SIZES)])
    Xs = [phi[order][off[i]:off[i + 1]] for i in range(len(SIZES))]
    ys = [lab[:n][order][off[i]:off[i + 1]] for i in range(len(SIZES))]
    return Xs, ys, phi[n:], lab[n:]


def run_case(name, dtype=F32):
    """The restatement of a drop-in case; seeds the global generator."""
    import torch
    Xs, ys, Xt, yt = case_data()
    torch.manual_seed(TORCH_SEED)
    return scaffold(Xs, ys, Xt, yt, C, D, LR, E, B, True, LAM, R, dtype=dtype, **CASES[name])

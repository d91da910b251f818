"""CPU restatement of q-FedAvg (q-FFL; Li, Sanjabi, Beirami, Smith, ICLR 2020) in numpy, with a dtype
argument: float32 is what the GPU computes, float64 the exact evaluation the drift bounds are
measured against (tests/golden/make_golden_qffl.py writes qffl_drift.json, the method of
fedopt_drift.json).  Not in the reference.  Only the server step and the pre-round local evaluation
are restated here: training, test evaluation, RNG use, the learning-rate schedule and the
initialisation are FedAvg's with parallel clients, from oracle.fedsim_oracle (classification) and
tests/mse_restatement.py (regression), unchanged.

Round t with the sample S (ascending ids; every client without ``sched``), x = the global model,
L = 1 / lr_t (or the given Lipschitz estimate), p_k = n_k / n ('size') or 1 / N ('uniform') over ALL
clients:

  F_k  = the mean loss of x on client k's own rows (cross-entropy or squared error), Ft = F_k + 1e-10
  u_k  = p_k Ft^q,   g_k = p_k q Ft^(q-1) L^2             float64, rounded once to float32
                                                          (q = 0: u = p, g = 0 exactly)
  S    = sum_S fl(u_k * fl(W_k - x))                      the left fold of fedopt_restatement.delta
  n_k  = sum_i fl(W_k[i] - x[i])^2                        float64 sum of the float32 squares (the
                                                          kernel: within 16 * 2^-24 of the exact sum)
  U = sum_S u_k,  G = sum_S g_k n_k,  H = L U + G         float64, k ascending
  coef = f32(L / H), 0 when H is not finite or <= 0
  x'   = fl(x + fl(coef * S))

which is the paper's w - sum_S Delta_k / sum_S h_k with Delta_k = u_k L (x - W_k) and
h_k = p_k (q Ft^(q-1) ||L (x - W_k)||^2 + L Ft^q).  train_loss[t] = sum_S (n_k / sum_S n) loss_k, FedAvg's.
"""
import numpy as np

from oracle import fedsim_oracle as O
from tests import fednova_restatement as FR
from tests import fedopt_restatement as FO
from tests import mse_restatement as M

F32 = np.float32
F64 = np.float64
EPS = 1e-10


def client_weights(ns, weighting='size', dtype=F32):
    """p over all N clients: float64, rounded once to float32 and carried in ``dtype``."""
    ns = np.asarray(ns, F64)
    p = np.full(len(ns), 1.0 / len(ns)) if weighting == 'uniform' else ns / float(ns.sum())
    return p if dtype == F64 else p.astype(F32).astype(dtype)


def coefficients(F, p, q, L, dtype=F32):
    """(u, g) of fs_qffl_coef from the losses ``F`` and the weights ``p`` of the same clients: float64
    arithmetic in the kernel's order, rounded once to float32 (float64: unrounded)."""
    Ft = np.asarray(F, F64) + EPS
    p = np.asarray(p, F64)
    q, L = float(q), float(L)
    if q == 0.0:
        u, g = p.copy(), np.zeros_like(p)
    else:
        u = p * np.power(Ft, q)
        g = p * q * np.power(Ft, q - 1.0) * (L * L)
    if dtype == F64:
        return u, g
    return u.astype(F32).astype(dtype), g.astype(F32).astype(dtype)


def norms(Ws, x, dtype=F32):
    """n_k = ||W_k - x||^2: the differences and their squares in ``dtype``, summed in float64."""
    T = dtype
    x = np.asarray(x, T)
    out = np.zeros(len(Ws), F64)
    for k in range(len(Ws)):
        d = (np.asarray(Ws[k], T) - x).astype(T)
        out[k] = np.sum((d * d).astype(T).astype(F64).reshape(-1))
    return out


def finish(S, n, u, g, L, x, dtype=F32):
    """The finish on a folded update ``S`` and the norms ``n``: returns (x', H, coef).  The sums run
    in float64 with k ascending, one operation at a time (python floats are IEEE doubles)."""
    T = dtype
    U, G = 0.0, 0.0
    for k in range(len(u)):
        U += float(u[k])
        G += float(g[k]) * float(n[k])
    H = float(L) * U + G
    ok = np.isfinite(H) and H > 0.0
    coef = (float(L) / H) if ok else 0.0
    coef = T(F32(coef)) if T != F64 else F64(coef)
    x = np.asarray(x, T)
    if coef == 0:
        return x.copy(), H, coef
    return (x + (coef * np.asarray(S, T)).astype(T)).astype(T), H, coef


def server(x, Ws, u, g, L, dtype=F32):
    """fs_aggregate_qffl in its left-fold regime.  Returns (x', S, n, H, coef)."""
    S = FO.delta(Ws, u, x, dtype)
    n = norms(Ws, x, dtype)
    x2, H, coef = finish(S, n, u, g, L, x, dtype)
    return x2, S, n, H, coef


def paper_step(x, Ws, F, p, q, L):
    """The authors' formulation in float64: w - sum_k Delta_k / sum_k h_k."""
    x = np.asarray(x, F64)
    Ft = np.asarray(F, F64) + EPS
    num, den = np.zeros_like(x), 0.0
    for k in range(len(Ws)):
        dw = float(L) * (x - np.asarray(Ws[k], F64))
        num += float(p[k]) * Ft[k] ** q * dw
        den += float(p[k]) * (q * Ft[k] ** (q - 1.0) * float(np.sum(dw * dw)) + float(L) * Ft[k] ** q)
    return x - num / den


def local_loss(X, y, W, mse, dtype=F32):
    """F_k: the mean loss of the model on one client's rows, every row's loss in ``dtype``, their sum
    in float64 (fs_eval's accumulation); no draw from any generator."""
    T = dtype
    X = np.asarray(X, T)
    if mse:
        res = (X @ np.asarray(W, T).reshape(-1)).astype(T) - np.asarray(y, T).reshape(-1)
        rows = (res * res).astype(T)
    else:
        z = (X @ np.asarray(W, T).T).astype(T)
        z = z - z.max(axis=1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True, dtype=T)).astype(T)
        rows = -logp[np.arange(len(y)), np.asarray(y, np.int64).reshape(-1)].astype(T)
    return float(np.sum(rows.astype(F64))) / len(rows)


def lipschitz_schedule(lr, R, lipschitz=None):
    """L_t of every round: the given estimate, else 1 / lr_t with the decayed learning rate."""
    out = []
    for t in range(R):
        lr = O.lr_schedule(t, lr, R)
        out.append(float(lipschitz) if lipschitz is not None else 1.0 / float(lr))
    return out


def qfedavg(Xs, ys, Xt, yt, type='classification', num_classes=10, D=200, lr=0.01, epoch=2, batch_size=32,
            prox=False, mu=0.1, reg=False, lam=0.01, R=100, q=1.0, weighting='size', lipschitz=None, sched=None,
            dtype=F32):
    """Returns (train_loss[R], test_loss[R], test_acc[R], {'W': [R, C, D], 'F': [R, N], 'n': [R, N] (NaN
    where not sampled), 'hc': [R, 2]}).  Draws from torch's global generator as FedAvg with parallel
    clients and the same sample does: seed it first."""
    T = dtype
    mse = type == 'regression'
    saved = O.F32
    O.F32 = T
    try:
        ns = np.array([len(y) for y in ys])
        N = len(ns)
        Xs = [np.asarray(x, T) for x in Xs]
        Xt = np.asarray(Xt, T)
        if mse:
            ys = [np.asarray(y, T).reshape(-1) for y in ys]
            yt = np.asarray(yt, T).reshape(-1)
            Wg = O.mlp_init(D, 1).astype(T).reshape(-1)
        else:
            ys = [np.asarray(y, np.int64).reshape(-1) for y in ys]
            yt = np.asarray(yt, np.int64).reshape(-1)
            Wg = O.mlp_init(D, num_classes).astype(T)
        p = client_weights(ns, weighting, T)
        Ls = lipschitz_schedule(lr, R, lipschitz)
        tr, tl, ta = np.zeros(R), np.zeros(R), np.zeros(R)
        hist = {k: [] for k in ('W', 'F', 'n', 'hc')}
        shape = (1 if mse else num_classes, D)
        for t in range(R):
            lr = O.lr_schedule(t, lr, R)
            S = np.arange(N) if sched is None else np.asarray(sched[t])
            F = np.array([local_loss(Xs[j], ys[j], Wg, mse, T) for j in range(N)])
            u, g = coefficients(F[S], p[S], q, Ls[t], T)
            step = FR._round_mse if mse else FR._round_ce
            Ws, losses = step([Xs[j] for j in S], [ys[j] for j in S], Wg, lr, epoch, batch_size, prox, mu, reg, lam,
                              'parallel', T)
            tr[t] = np.sum(FR.weights(ns[S], T) * losses, dtype=T)
            Wg, _, n, H, coef = server(Wg, Ws, u, g, Ls[t], T)
            nn = np.full(N, np.nan)
            nn[S] = n
            for k, a in (('W', np.array(Wg, copy=True).reshape(shape)), ('F', F), ('n', nn),
                         ('hc', np.array([H, float(coef)]))):
                hist[k].append(a)
            tl[t], ta[t] = (M.test_eval(Xt, yt, Wg, batch_size, T) if mse else O.test_eval(Xt, yt, Wg, batch_size))
        return tr, tl, ta, {k: np.stack(a) for k, a in hist.items()}
    finally:
        O.F32 = saved


# ---- the drop-in cases (tests/test_gpu_qffl.py, tests/golden/make_golden_qffl.py) -----------------
# the FedOpt drop-in test's federation (fedopt_restatement.case_data: N = 6 ragged clients, D = 64,
# C = 3, and C = 1 for regression, E = 2, B = 8, R = 3, lr = 0.5 so L = 2)
SIZES, D, C, R, E, B, LR, LAM, MU = FO.SIZES, FO.D, FO.C, FO.R, FO.E, FO.B, FO.LR, FO.LAM, FO.MU
TORCH_SEED = FO.TORCH_SEED
PARTICIPATION, SAMPLE_SEED = 0.5, 0
CASES = {
    'q0_size_full': dict(q=0.0, weighting='size', sampled=False),
    'q0_size_sampled': dict(q=0.0, weighting='size', sampled=True),
    'q1_size_full': dict(q=1.0, weighting='size', sampled=False),
    'q1_uniform_sampled': dict(q=1.0, weighting='uniform', sampled=True),
    'q5_uniform_full': dict(q=5.0, weighting='uniform', sampled=False),
    'q5_size_sampled': dict(q=5.0, weighting='size', sampled=True),
    'q1_prox': dict(q=1.0, weighting='size', sampled=False, prox=True),
    'q5_regression': dict(q=5.0, weighting='size', sampled=False, type='regression'),
}
case_data = FO.case_data


def case_sched(name):
    """The sample of every round of a case: participation = 0.5 by the project's own sampler (host only)."""
    if not CASES[name]['sampled']:
        return None
    from fedamw_amd.functions.participation import make_schedule
    return make_schedule(len(SIZES), R, PARTICIPATION, SAMPLE_SEED)


def case_args(name):
    """(type, C, batch_size, prox) of a case."""
    k = CASES[name]
    type = k.get('type', 'classification')
    return type, (1 if type == 'regression' else C), B, k.get('prox', False)


def run_case(name, dtype=F32):
    """The restatement of a drop-in case; seeds the global generator."""
    import torch
    k = CASES[name]
    type, nc, bs, prox = case_args(name)
    Xs, ys, Xt, yt = case_data(type == 'regression')
    torch.manual_seed(TORCH_SEED)
    return qfedavg(Xs, ys, Xt, yt, type, nc, D, LR, E, bs, prox, MU, True, LAM, R, q=k['q'], weighting=k['weighting'],
                   sched=case_sched(name), dtype=dtype)

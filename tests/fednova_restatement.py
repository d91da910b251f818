"""CPU restatement of FedNova (tools.py:383-410) in numpy, with a dtype argument: float32 is what
the GPU kernels and the reference's torch CPU ops compute, float64 the exact evaluation the drift
bounds are measured against (tests/golden/make_golden_fednova.py writes fednova_drift.json, the
method of horizon_drift.py).

Two aggregation rules on top of FedAvg's round (training, evaluation, RNG use, learning-rate
schedule and initialisation come from oracle.fedsim_oracle for classification and from
tests/mse_restatement.py for regression, unchanged):

  variant 'reference'  tools.py:401-405, which scale the clients' WEIGHTS:
        W = W_0 * s0 + sum_{j>=1} ((p_j * W_j) * te) / b_j
     with the host scalars of tools.py:387-389: p float32, Tau = n*E/B float64,
     Tau_eff = sum(Tau*p) float64, and -- the weights being float32 tensors -- s0 =
     f32(f64(p_0)*Tau_eff/Tau_0), te = f32(Tau_eff), b_j = f32(Tau_j).  For unequal client sizes
     the coefficients sum to N * sum_j p_j^2 > 1.
  variant 'updates'    Wang et al. (2020): W = W_g + sum_j a_j (W_j - W_g), a_j = p_j tau_eff / tau_j,
     tau_j = E*ceil(n_j/B) the steps train_loop takes, tau_eff = sum_j p_j tau_j (float64).
     Parallel clients only.

``sched`` (a list of ascending id arrays, one per round) restricts every round to its sample: only
the sampled clients train and draw shuffles, and p, Tau, tau, Tau_eff and s0 are taken over the
sample, as FedAvg under participation restricts tools.py:333 to S.  train_loss is the plain
p-weighted loss (tools.py:400) in both variants.
"""
import numpy as np

from oracle import fedsim_oracle as O
from tests import mse_restatement as M

F32 = np.float32
F64 = np.float64


def weights(ns, dtype=F32):
    """tools.py:387: torch.tensor(n / sum(n), dtype=float32), carried in ``dtype``."""
    ns = np.asarray(ns)
    return (ns / sum(ns)).astype(F32).astype(dtype)


def reference_coefficients(ns, epoch, batch_size, dtype=F32):
    """(p, b, te, s0) of the reference form over the clients ``ns``.  float32: the scalars as the
    reference's float32 weight tensors receive them; float64: unrounded."""
    ns = np.asarray(ns)
    p = weights(ns, F64)
    Tau = ns * epoch / batch_size
    Tau_eff = np.sum(Tau * p)
    s0 = p[0] * Tau_eff / Tau[0]
    return p.astype(dtype), Tau.astype(dtype), dtype(Tau_eff), dtype(s0)


def update_coefficients(ns, epoch, batch_size, dtype=F32):
    """(p, a) of the update-normalised form over the clients ``ns``."""
    ns = np.asarray(ns)
    p = weights(ns, F64)
    tau = (epoch * -(-ns // batch_size)).astype(F64)
    tau_eff = np.sum(p * tau)
    return p.astype(dtype), (p * tau_eff / tau).astype(dtype)


def aggregate_reference(Ws, q, b, te, s0, dtype=F32):
    """The left fold of fs_aggregate_nova mode 1: every product, the quotient and every sum
    rounded to ``dtype``.  b[0] is not used."""
    T = dtype
    q, b = np.asarray(q, T), np.asarray(b, T)
    acc = (np.asarray(Ws[0], T) * T(s0)).astype(T)
    for k in range(1, len(Ws)):
        term = (((q[k] * np.asarray(Ws[k], T)).astype(T) * T(te)).astype(T) / b[k]).astype(T)
        acc = (acc + term).astype(T)
    return acc


def aggregate_updates(Ws, a, base, dtype=F32):
    """The left fold of fs_aggregate_nova mode 2: base + sum_k a_k (W_k - base), the first term the
    product itself."""
    T = dtype
    a, base = np.asarray(a, T), np.asarray(base, T)
    acc = None
    for k in range(len(Ws)):
        term = (a[k] * (np.asarray(Ws[k], T) - base).astype(T)).astype(T)
        acc = term if acc is None else (acc + term).astype(T)
    return (base + acc).astype(T)


def _round_ce(Xs, ys, Wg, lr, E, B, prox, mu, reg, lam, clients, dtype):
    Ws, losses = O._local_round(Xs, ys, Wg, lr, E, B, prox, mu, reg, lam, clients)
    return Ws, np.asarray(losses, dtype=F32).astype(dtype)


def _round_mse(Xs, ys, wg, lr, E, B, prox, mu, reg, lam, clients, dtype):
    Ws, losses = M._local_round(Xs, ys, wg, lr, E, B, prox, mu, reg, lam, clients, dtype)
    return Ws, np.asarray(losses, dtype=F32).astype(dtype)


def fednova(Xs, ys, Xt, yt, type='classification', num_classes=10, D=200, lr=0.01, epoch=2, batch_size=32,
            prox=False, mu=0.1, reg=False, lam=0.01, R=100, clients='sequential', variant='reference', sched=None,
            dtype=F32, rule='fednova'):
    """Returns (train_loss[R], test_loss[R], test_acc[R], {'W': [R, C, D]}).  ``rule='fedavg'``: the
    plain aggregate of tools.py:345-350 in place of FedNova's (the FedAvg restatement on the same
    code path, for the equal-sizes check).  Draws from torch's global generator as the reference:
    seed it first."""
    if variant == 'updates' and clients != 'parallel':
        raise ValueError("variant='updates' needs clients='parallel'")
    mse = type == 'regression'
    saved = O.F32
    O.F32 = dtype                  # the classification oracle's working type (horizon_drift.py's method)
    try:
        ns = np.array([len(y) for y in ys])
        if mse:
            Xs = [np.asarray(x, dtype) for x in Xs]
            ys = [np.asarray(y, dtype).reshape(-1) for y in ys]
            Xt, yt = np.asarray(Xt, dtype), np.asarray(yt, dtype).reshape(-1)
            Wg = O.mlp_init(D, 1).astype(dtype).reshape(-1)
        else:
            Xs = [np.asarray(x, dtype) for x in Xs]
            ys = [np.asarray(y, np.int64).reshape(-1) for y in ys]
            Xt, yt = np.asarray(Xt, dtype), np.asarray(yt, np.int64).reshape(-1)
            Wg = O.mlp_init(D, num_classes).astype(dtype)
        tr, tl, ta = np.zeros(R), np.zeros(R), np.zeros(R)
        Wt = []
        for t in range(R):
            lr = O.lr_schedule(t, lr, R)
            S = np.arange(len(ns)) if sched is None else np.asarray(sched[t])
            step = _round_mse if mse else _round_ce
            Ws, losses = step([Xs[j] for j in S], [ys[j] for j in S], Wg, lr, epoch, batch_size, prox, mu, reg, lam,
                              clients, dtype)
            p = weights(ns[S], dtype)
            tr[t] = np.sum(p * losses, dtype=dtype)
            if rule == 'fedavg':
                Wg = M.aggregate(Ws, p, dtype)
            elif variant == 'reference':
                q, b, te, s0 = reference_coefficients(ns[S], epoch, batch_size, dtype)
                Wg = aggregate_reference(Ws, q, b, te, s0, dtype)
            else:
                Wg = aggregate_updates(Ws, update_coefficients(ns[S], epoch, batch_size, dtype)[1], Wg, dtype)
            Wt.append(np.array(Wg, copy=True).reshape(1 if mse else num_classes, D))
            tl[t], ta[t] = (M.test_eval(Xt, yt, Wg, batch_size, dtype) if mse else O.test_eval(Xt, yt, Wg, batch_size))
        return tr, tl, ta, {'W': np.stack(Wt)}
    finally:
        O.F32 = saved


def run_case(d, dtype=F32, **kw):
    """The restatement of a fixture case (tests/fednova_fixtures.py ``load``); seeds the global
    generator as the generator script did.  Keywords override (clients, variant, sched, rule)."""
    import torch
    off = np.concatenate([[0], np.cumsum(d['sizes'])])
    Xs = [d['X_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]
    ys = [d['y_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]
    args = dict(type=str(d['type']), num_classes=int(d['C']), D=int(d['D']), lr=float(d['lr']), epoch=int(d['epoch']),
                batch_size=int(d['batch_size']), prox=bool(d['prox']), mu=float(d['mu']), reg=bool(d['reg']),
                lam=float(d['lam']), R=int(d['R']), clients='sequential', variant='reference', dtype=dtype)
    args.update(kw)
    torch.manual_seed(int(d['torch_seed']))
    return fednova(Xs, ys, d['X_test'], d['y_test'], **args)

"""CPU restatement of the FedOpt server optimizers (Reddi et al., ICLR 2021, Algorithm 2: FedAdagrad /
FedAdam / FedYogi; FedAvgM, Hsu et al. 2019) in numpy, with a dtype argument: float32 is what the GPU
kernel computes, float64 the exact evaluation the drift bounds are measured against
(tests/golden/make_golden_fedopt.py writes fedopt_drift.json, the method of scaffold_drift.json).
Not in the reference.  Only the server step is restated here: training, evaluation, RNG use, the
learning-rate schedule and the initialisation are FedAvg's with parallel clients, from
oracle.fedsim_oracle (classification) and tests/mse_restatement.py (regression), unchanged.

Round t with the sample S (ascending ids; every client without ``sched``), x = the global model:

  delta = sum_S fl(q_k * fl(W_k - x)),  q = n[S] / sum(n[S]) (FedAvg's weights), a left fold in
          ascending k whose first term is the term itself
  avgm      m' = fl(fl(beta1*m) + delta),                      x' = fl(x + fl(eta*m'))
  others    m' = fl(fl(beta1*m) + fl(omb1*delta)),  d2 = fl(delta*delta)
    adagrad   v' = fl(v + d2)
    adam      v' = fl(fl(beta2*v) + fl(omb2*d2))
    yogi      v' = fl(v - fl(fl(omb2*d2) * sgn(fl(v - d2))))
              x' = fl(x + fl(fl(eta*m') / fl(sqrt(v') + tau)))

m0 = 0, v0 = tau^2 unless given; no bias correction.  The scalars (eta, beta1, omb1 = 1 - beta1, beta2,
omb2 = 1 - beta2, tau) are float64 host values rounded once to float32 (the float64 run keeps them
unrounded).  train_loss[t] = sum_S q_k loss_k, FedAvg's.
"""
import numpy as np

from oracle import fedsim_oracle as O
from tests import fednova_restatement as FR
from tests import mse_restatement as M

F32 = np.float32
F64 = np.float64
RULES = ('avgm', 'adagrad', 'adam', 'yogi')


def scalars(server_lr, beta1, beta2, tau, dtype=F32):
    """(eta, beta1, omb1, beta2, omb2, tau): float64 arithmetic, rounded once to float32 and carried
    in ``dtype`` (float64: unrounded)."""
    s = (float(server_lr), float(beta1), 1.0 - float(beta1), float(beta2), 1.0 - float(beta2), float(tau))
    if dtype == F64:
        return tuple(F64(a) for a in s)
    return tuple(dtype(F32(a)) for a in s)


def delta(Ws, q, x, dtype=F32):
    """The left fold of the updates: fs_aggregate_nova's mode 2 before it adds its base."""
    T = dtype
    q, x = np.asarray(q, T), np.asarray(x, T)
    acc = None
    for k in range(len(Ws)):
        term = (q[k] * (np.asarray(Ws[k], T) - x).astype(T)).astype(T)
        acc = term if acc is None else (acc + term).astype(T)
    return acc


def finish(rule, d, x, m, v, sc, dtype=F32):
    """The element-wise server step on a folded delta ``d``.  Returns (x', m', v'); avgm returns v
    as it came (None allowed)."""
    T = dtype
    eta, b1, o1, b2, o2, tau = (T(a) for a in sc)
    d, x, m = np.asarray(d, T), np.asarray(x, T), np.asarray(m, T)
    if rule == 'avgm':
        m2 = ((b1 * m).astype(T) + d).astype(T)
        return (x + (eta * m2).astype(T)).astype(T), m2, v
    v = np.asarray(v, T)
    d2 = (d * d).astype(T)
    m2 = ((b1 * m).astype(T) + (o1 * d).astype(T)).astype(T)
    if rule == 'adagrad':
        v2 = (v + d2).astype(T)
    elif rule == 'adam':
        v2 = ((b2 * v).astype(T) + (o2 * d2).astype(T)).astype(T)
    elif rule == 'yogi':
        s = np.sign((v - d2).astype(T)).astype(T)
        v2 = (v - ((o2 * d2).astype(T) * s).astype(T)).astype(T)
    else:
        raise ValueError('unknown rule %r' % (rule,))
    den = (np.sqrt(v2).astype(T) + tau).astype(T)
    return (x + ((eta * m2).astype(T) / den).astype(T)).astype(T), m2, v2


def server(rule, x, m, v, Ws, q, sc, dtype=F32):
    """fs_aggregate_opt in its left-fold regime.  Returns (x', m', v')."""
    return finish(rule, delta(Ws, q, x, dtype), x, m, v, sc, dtype)


def fedopt(Xs, ys, Xt, yt, type='classification', num_classes=10, D=200, lr=0.01, epoch=2, batch_size=32,
           prox=False, mu=0.1, reg=False, lam=0.01, R=100, rule='adam', server_lr=0.1, beta1=0.9, beta2=0.99,
           tau=1e-3, v0=None, sched=None, dtype=F32):
    """Returns (train_loss[R], test_loss[R], test_acc[R], {'W', 'm', 'v', 'delta', 'v_prev': [R, C, D]})
    ('delta' and 'v_prev': the round's folded update and the second moment it met, for the generator's
    check of YOGI's sign).  Draws from torch's global generator as FedAvg with parallel clients and
    the same sample does: seed it first."""
    T = dtype
    mse = type == 'regression'
    saved = O.F32
    O.F32 = T
    try:
        ns = np.array([len(y) for y in ys])
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
        sc = scalars(server_lr, beta1, beta2, tau, T)
        m = np.zeros_like(Wg)
        v = np.full_like(Wg, T(F32(float(tau) ** 2 if v0 is None else v0)) if T != F64
                         else (float(tau) ** 2 if v0 is None else float(v0)))
        tr, tl, ta = np.zeros(R), np.zeros(R), np.zeros(R)
        hist = {k: [] for k in ('W', 'm', 'v', 'delta', 'v_prev')}
        shape = (1 if mse else num_classes, D)
        for t in range(R):
            lr = O.lr_schedule(t, lr, R)
            S = np.arange(len(ns)) if sched is None else np.asarray(sched[t])
            step = FR._round_mse if mse else FR._round_ce
            Ws, losses = step([Xs[j] for j in S], [ys[j] for j in S], Wg, lr, epoch, batch_size, prox, mu, reg, lam,
                              'parallel', T)
            q = FR.weights(ns[S], T)
            tr[t] = np.sum(q * losses, dtype=T)
            d = delta(Ws, q, Wg, T)
            hist['delta'].append(d.reshape(shape).copy())
            hist['v_prev'].append(v.reshape(shape).copy())
            Wg, m, v = finish(rule, d, Wg, m, v, sc, T)
            for k, a in (('W', Wg), ('m', m), ('v', v)):
                hist[k].append(np.array(a, copy=True).reshape(shape))
            tl[t], ta[t] = (M.test_eval(Xt, yt, Wg, batch_size, T) if mse else O.test_eval(Xt, yt, Wg, batch_size))
        return tr, tl, ta, {k: np.stack(a) for k, a in hist.items()}
    finally:
        O.F32 = saved


# ---- the drop-in cases (tests/test_gpu_fedopt.py, tests/golden/make_golden_fedopt.py) -------------
# the SCAFFOLD drop-in test's scale: N = 6 unequal clients, C = 3, D = 64, E = 2, B = 8, R = 3
SIZES = [21, 8, 37, 5, 16, 12]
D, C, R, E, B, LR, LAM, MU = 64, 3, 3, 2, 8, 0.5, 0.001, 0.1
SCHED = [np.array([0, 2, 5]), np.array([1, 2, 3]), np.array([0, 4, 5])]    # M = 3, three distinct samples
TORCH_SEED = 100
# tau = server_lr = 0.1: the step's Lipschitz factor in delta is eta*omb1/(2 tau) = 0.25 for the adaptive
# rules (beta1 = 0.5) and eta/(1 - beta1) = 0.2 for avgm -- below 1, so a round adds at most one
# training-kernel tolerance
SERVER = dict(server_lr=0.1, beta1=0.5, beta2=0.9, tau=0.1)
CASES = {'%s_%s' % (rule, part): dict(rule=rule, sched=SCHED if part == 'sampled' else None)
         for rule in RULES for part in ('full', 'sampled')}
CASES['adam_prox'] = dict(rule='adam', sched=None, prox=True)
CASES['yogi_regression'] = dict(rule='yogi', sched=None, type='regression')
CASES['adam_wide'] = dict(rule='adam', sched=None, batch_size=80)
DATA_SEED = 77


def case_data(regression=False):
    """The inputs of every drop-in case: random-feature rows with a label skew across the clients;
    regression: a noisy linear target of the same rows."""
    rs = np.random.RandomState(DATA_SEED)
    n, nt = sum(SIZES), 40
    raw = rs.normal(size=(n + nt, 10)).astype(F32)
    phi = (np.cos(raw @ rs.normal(0, 0.7, size=(10, D)).astype(F32) + rs.uniform(0, 2 * np.pi, size=(1, D)).astype(F32))
           / np.sqrt(D)).astype(F32)
    lab = np.argmax(phi @ rs.normal(size=(D, C)).astype(F32) + 0.1 * rs.normal(size=(n + nt, C)), axis=1).astype(np.int64)
    order = np.argsort(lab[:n] + 1.5 * rs.normal(size=n), kind='stable')     # non-IID: clients sorted along the label
    y = lab
    if regression:
        y = (phi @ rs.normal(size=D).astype(F32) + 0.05 * rs.normal(size=n + nt)).astype(F32)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    Xs = [phi[order][off[i]:off[i + 1]] for i in range(len(SIZES))]
    ys = [y[:n][order][off[i]:off[i + 1]] for i in range(len(SIZES))]
    return Xs, ys, phi[n:], y[n:]


def case_args(name):
    """(type, C, batch_size, prox) of a case."""
    k = CASES[name]
    type = k.get('type', 'classification')
    return type, (1 if type == 'regression' else C), k.get('batch_size', B), k.get('prox', False)


def run_case(name, dtype=F32):
    """The restatement of a drop-in case; seeds the global generator."""
    import torch
    k = CASES[name]
    type, nc, bs, prox = case_args(name)
    Xs, ys, Xt, yt = case_data(type == 'regression')
    torch.manual_seed(TORCH_SEED)
    return fedopt(Xs, ys, Xt, yt, type, nc, D, LR, E, bs, prox, MU, True, LAM, R, rule=k['rule'], sched=k['sched'],
                  dtype=dtype, **SERVER)

"""CPU restatement of the regression task (type='regression', num_classes = 1) in numpy,
with a dtype argument: float32 is what the GPU kernels and the reference's torch CPU ops
compute, float64 the exact evaluation the drift bounds are measured against
(tests/golden/make_golden_mse.py writes mse_drift.json, the method of horizon_drift.py).

Restates the three loops of the reference under nn.MSELoss(reduction='mean'):
  train_client    tools.py:177-215 (criterion tools.py:183-184)
  test_eval       tools.py:218-237 (criterion tools.py:223-224; comp_accuracy tools.py:82-96)
  mixture_solve_z tools.py:441-453 (criterion tools.py:421-422)
and the six drivers on top of them.  RNG use, learning-rate schedule, initialisation and the
fp32 aggregate come from oracle.fedsim_oracle unchanged.
"""
import numpy as np
import torch

from oracle.fedsim_oracle import aggregate as _aggregate_f32
from oracle.fedsim_oracle import lr_schedule, mlp_init, pass_order

F32 = np.float32


def aggregate(Ws, p, dtype=F32):
    """tools.py:345-350: the left fold p0*W0 + p1*W1 + ..., every product and sum rounded."""
    if dtype == F32:
        return _aggregate_f32([np.asarray(w, F32) for w in Ws], p)
    p = np.asarray(p, dtype)
    acc = Ws[0] * p[0]
    for j in range(1, len(Ws)):
        acc = acc + p[j] * Ws[j]
    return acc


def train_client(X, y, w, lr, epoch, batch_size, prox, mu, reg, lam, dtype=F32):
    """One train_loop call.  X [n, D], y [n], w [D].  Per batch b (tools.py:190-211):
      o = X_b w;  L = mean((o - y)^2) [+ mu ||w - w_a||] [+ lam ||w||]
      dL/do = (2 / |b|) (o - y);  w -= lr (X_b^T dL/do + mu (w - w_a)/||w - w_a|| + lam w/||w||)
    (a zero norm contributes a zero gradient).  Returns (w, |b|-weighted mean loss of the
    last epoch, accumulated in double)."""
    T = dtype
    X = np.asarray(X, T)
    y = np.asarray(y, T).reshape(-1)
    w = np.array(w, T, copy=True).reshape(-1)
    wa = w.copy()
    lr_, mu_, lam_ = T(lr), T(mu), T(lam)
    n = len(y)
    avg = 0.0
    for _ in range(epoch):
        order = pass_order(n)
        s, cnt = 0.0, 0
        for b0 in range(0, n, batch_size):
            idx = order[b0:b0 + batch_size]
            xb, yb = X[idx], y[idx]
            bsz = len(idx)
            res = (xb @ w).astype(T) - yb
            loss = T(np.sum(res * res, dtype=T) / T(bsz))
            g = (T(2.0) / T(bsz)) * res
            grad = (g @ xb).astype(T)
            if prox:
                dw = w - wa
                pn = T(np.sqrt(np.sum(dw * dw, dtype=T)))
                loss = T(loss + mu_ * pn)
                if pn > 0:
                    grad = grad + dw * (mu_ / pn)
            if reg:
                wn = T(np.sqrt(np.sum(w * w, dtype=T)))
                loss = T(loss + lam_ * wn)
                if wn > 0:
                    grad = grad + w * (lam_ / wn)
            w = (w - lr_ * grad).astype(T)
            s += float(loss) * bsz
            cnt += bsz
        avg = s / cnt if cnt else 0.0
    return w, avg


def test_eval(X, y, w, batch_size=32, dtype=F32):
    """One test_loop call: loss = sum_b mean_b |b| / n; "accuracy" = 100 #{y == 0} / n (the
    top-1 index of a one-column output is 0, compared with the float target)."""
    T = dtype
    X = np.asarray(X, T)
    y = np.asarray(y, T).reshape(-1)
    w = np.asarray(w, T).reshape(-1)
    n = len(y)
    order = pass_order(n)
    ls, acs = 0.0, 0.0
    for b0 in range(0, n, batch_size):
        idx = order[b0:b0 + batch_size]
        bsz = len(idx)
        res = (X[idx] @ w).astype(T) - y[idx]
        ls += float(T(np.sum(res * res, dtype=T) / T(bsz))) * bsz
        acs += float(F32(F32((y[idx] == 0).sum()) * F32(100.0 / bsz))) * bsz
    return ls / n, acs / n


def mixture_solve_z(Z, yv, p, buf, lr_p, epochs, batch_size=16, momentum=0.9, dtype=F32):
    """The p-SGD on Z [n_val, N] (Z[v][n] = x_v . w_n).  Returns (p, buf); buf None = the
    optimiser has not stepped yet."""
    T = dtype
    Z = np.asarray(Z, T)
    yv = np.asarray(yv, T).reshape(-1)
    p = np.array(p, T, copy=True)
    lr_, mom = T(lr_p), T(momentum)
    nv = len(yv)
    for _ in range(epochs):
        order = pass_order(nv)
        for b0 in range(0, nv, batch_size):
            idx = order[b0:b0 + batch_size]
            zb = Z[idx]
            res = (zb @ p).astype(T) - yv[idx]
            g = (T(2.0) / T(len(idx))) * res
            gp = (g @ zb).astype(T)
            buf = gp.copy() if buf is None else (mom * buf + gp).astype(T)
            p = (p - lr_ * buf).astype(T)
    return p, buf


def make_z(Ws, Xv, dtype=F32):
    return (np.asarray(Xv, dtype) @ np.stack([np.asarray(w, dtype).reshape(-1) for w in Ws], axis=1)).astype(dtype)


def _weights(ys, dtype):
    num = np.array([len(y) for y in ys])
    return (num / sum(num)).astype(F32).astype(dtype)      # torch.tensor(..., dtype=float32)


def _local_round(Xs, ys, wg, lr, epoch, B, prox, mu, reg, lam, clients, dtype):
    Ws, losses = [], []
    w = wg
    for X, y in zip(Xs, ys):
        w, l = train_client(X, y, wg if clients == 'parallel' else w, lr, epoch, B, prox, mu, reg, lam, dtype)
        Ws.append(w)
        losses.append(l)
    return Ws, losses


def _tl(p, losses, dtype):
    return np.sum(np.asarray(p, dtype) * np.asarray(losses, dtype=F32).astype(dtype), dtype=dtype)


def fed(algo, Xs, ys, Xt, yt, D, lr, epoch, B, prox, mu, reg, lam, R, clients='sequential', Xv=None, yv=None,
        lr_p=0.0, Bv=16, dtype=F32):
    """FedAvg / FedProx / FedAMW (tools.py:329-353, 356-380, 413-463).  Returns (train_loss,
    test_loss, test_acc, {'W': [R, 1, D], 'p': [R, N] (fedamw)})."""
    wg = mlp_init(D, 1).astype(dtype).reshape(-1)
    p = _weights(ys, dtype)
    buf = None
    tr, tl, ta = np.zeros(R), np.zeros(R), np.zeros(R)
    Wt, Pt = [], []
    for t in range(R):
        lr = lr_schedule(t, lr, R)
        Ws, losses = _local_round(Xs, ys, wg, lr, epoch, B, prox, mu, reg, lam, clients, dtype)
        tr[t] = _tl(p, losses, dtype)
        if algo == 'fedamw':
            p, buf = mixture_solve_z(make_z(Ws, Xv, dtype), yv, p, buf, lr_p, R, Bv, 0.9, dtype)
            Pt.append(p.copy())
        wg = aggregate(Ws, p, dtype)
        Wt.append(wg.copy()[None])
        tl[t], ta[t] = test_eval(Xt, yt, wg, B, dtype)
    trace = {'W': np.stack(Wt)}
    if Pt:
        trace['p'] = np.stack(Pt)
    return tr, tl, ta, trace


def centralized(Xs, ys, Xt, yt, D, lr, epoch, B, prox, mu, reg, lam, dtype=F32):
    """tools.py:240-255."""
    w = mlp_init(D, 1).astype(dtype).reshape(-1)
    w, loss = train_client(np.concatenate(Xs), np.concatenate([np.asarray(y).reshape(-1) for y in ys]), w, lr, epoch,
                           B, prox, mu, reg, lam, dtype)
    tl, ta = test_eval(Xt, yt, w, B, dtype)
    return loss, tl, ta, {'W': w[None, None]}


def _chain(Xs, ys, w, lr, epoch, B, prox, mu, reg, lam, dtype):
    return _local_round(Xs, ys, w, lr, epoch, B, prox, mu, reg, lam, 'sequential', dtype)


def distributed(Xs, ys, Xt, yt, D, lr, epoch, B, prox, mu, reg, lam, dtype=F32):
    """tools.py:258-276."""
    w = mlp_init(D, 1).astype(dtype).reshape(-1)
    p = _weights(ys, dtype)
    Ws, losses = _chain(Xs, ys, w, lr, epoch, B, prox, mu, reg, lam, dtype)
    wg = aggregate(Ws, p, dtype)
    tl, ta = test_eval(Xt, yt, wg, B, dtype)
    return _tl(p, losses, dtype), tl, ta, {'W': wg[None, None]}


def oneshot(Xs, ys, Xt, yt, Xv, yv, D, lr, epoch, B, prox, mu, reg, lam, R, lr_p, Bv=16, dtype=F32):
    """tools.py:279-326 (momentum 0; the compounding aggregate of oracle.FedAMW_OneShot)."""
    w = mlp_init(D, 1).astype(dtype).reshape(-1)
    p = _weights(ys, dtype)
    Ws, losses = _chain(Xs, ys, w, lr, epoch, B, prox, mu, reg, lam, dtype)
    tr = _tl(p, losses, dtype)
    Z = make_z(Ws, Xv, dtype)
    S = Ws[0].copy()
    tl, ta = np.zeros(R), np.zeros(R)
    Wt, Pt = [], []
    one = np.ones(1, dtype)
    for t in range(R):
        p, _ = mixture_solve_z(Z, yv, p, None, lr_p, 1, Bv, 0.0, dtype)
        wg = aggregate([(S * p[0]).astype(dtype)] + Ws[1:], np.concatenate([one, p[1:]]).astype(dtype), dtype)
        S = wg
        Wt.append(wg.copy()[None])
        Pt.append(p.copy())
        tl[t], ta[t] = test_eval(Xt, yt, wg, B, dtype)
    return tr, tl, ta, {'W': np.stack(Wt), 'p': np.stack(Pt)}


def run_case(d, dtype=F32):
    """The restatement of a round or single-shot fixture case: ``d`` is mse_data.npz merged with
    the case file (tests/mse_fixtures.py ``load_case``).  Seeds the global generator as the
    generator script did.  Returns (train_loss, test_loss, test_acc, trace)."""
    D, Bv = int(d['D']), int(d['Bv'])
    off = np.concatenate([[0], np.cumsum(d['sizes'])])
    Xs = [d['X_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]
    ys = [d['y_train'][off[i]:off[i + 1]].reshape(-1) for i in range(len(d['sizes']))]
    Xt, yt, Xv, yv = d['X_test'], d['y_test'].reshape(-1), d['X_val'], d['y_val'].reshape(-1)
    hp = (float(d['lr']), int(d['epoch']), int(d['batch_size']), bool(d['prox']), float(d['mu']), bool(d['reg']),
          float(d['lam']))
    torch.manual_seed(int(d['torch_seed']))
    algo = str(d['algo'])
    if algo in ('fedavg', 'fedprox', 'fedamw'):
        mode = 'parallel' if str(d['mode']) == 'par' else 'sequential'
        return fed(algo, Xs, ys, Xt, yt, D, *hp, int(d['R']), clients=mode, Xv=Xv, yv=yv,
                   lr_p=float(d['lr_p']) if 'lr_p' in d else 0.0, Bv=Bv, dtype=dtype)
    if algo == 'centralized':
        return centralized(Xs, ys, Xt, yt, D, *hp, dtype=dtype)
    if algo == 'distributed':
        return distributed(Xs, ys, Xt, yt, D, *hp, dtype=dtype)
    return oneshot(Xs, ys, Xt, yt, Xv, yv, D, *hp, int(d['R']), float(d['lr_p']), Bv=Bv, dtype=dtype)

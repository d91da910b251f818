"""Golden-vector generator for the regression task: runs the UNMODIFIED reference
``functions/tools.py`` with ``type='regression'``, ``num_classes = 1`` and float targets of
shape [n, 1] (the reference's synthetic regression loader, utils.py:81-82, 121, 167).

Run only in the build container, after make_golden.py's conventions:
``python tests/golden/make_golden_mse.py``.  Writes data only, every file named ``mse_*``
(tests/fixtures.py globs ``fed*``, ``unit_train_*``, ``single_*`` ...: none may match):

  mse_data.npz     the shared inputs, stored once: three clients of 37, 70 and 33 rows, D = 200
                   (ld = 256: the padding is exercised), 45 test rows, 40 validation rows
                   (Bv = 16: the last batch is a ragged 8), targets clipped to [0, 100] with at
                   least two exact zeros in the test set
  mse_<case>.npz   hyper-parameters, seeds and the reference's outputs only: the per-round
                   global W, the learned p per round, the three return values and
                   ``rng_after`` (the global generator's position after the call)
  mse_drift.json   per case and quantity, delta = the distance of the float32 and the float64
                   run of tests/mse_restatement.py (how far any correct fp32 evaluation sits
                   from the exact one) and the bound max(1e-5, 2 delta) the tests use

Cases: mse_fedavg_{seq,par}, mse_fedprox_{seq,par} (ridge on), mse_fedamw_{seq,par} (``par`` is
the harness variant of make_golden.py: a fresh copy of the global model per client, the
reference's own MLP / train_loop / test_loop), mse_single_{centralized,distributed,oneshot},
mse_unit_train_{plain,prox,ridge,proxridge} (one train_loop call each), mse_unit_test.
E = 2, B = 32 (every client has a ragged last batch), R = 4 (both lr boundaries crossed).
"""
import contextlib
import copy
import io
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as G  # noqa: E402  (imports the reference unmodified and wraps its test_loop)
from tests import mse_restatement as M  # noqa: E402

T = G.T
_trace = G._trace
SIZES, D, N_TEST, N_VAL, BV = [37, 70, 33], 200, 45, 40, 16
TORCH_SEED = 100
EPOCH, B, R = 2, 32, 4


def synth():
    rs = np.random.RandomState(61)
    total = sum(SIZES) + N_TEST + N_VAL
    Xraw = (rs.rand(total, 14) < 0.3).astype(np.float32)
    Wr = rs.normal(0, 0.5, size=(14, D)).astype(np.float32)
    br = rs.uniform(0, 2 * np.pi, size=(1, D)).astype(np.float32)
    phi = (np.cos(Xraw @ Wr + br) / np.sqrt(D)).astype(np.float32)
    teacher = rs.normal(size=D).astype(np.float32)
    z = phi @ teacher
    y = np.clip(40.0 + 30.0 * (z - z.mean()) / z.std() + 2.0 * rs.normal(size=total), 0.0, 100.0).astype(np.float32)
    # client skew: client j's rows are drawn around a different quantile of the target
    order = np.argsort(y[:sum(SIZES)] + 15.0 * rs.normal(size=sum(SIZES)))
    tr = order
    nt0 = sum(SIZES)
    d = dict(X_train=phi[tr], y_train=y[tr].reshape(-1, 1), sizes=np.array(SIZES, np.int64),
             X_test=phi[nt0:nt0 + N_TEST], y_test=y[nt0:nt0 + N_TEST].reshape(-1, 1),
             X_val=phi[nt0 + N_TEST:], y_val=y[nt0 + N_TEST:].reshape(-1, 1))
    assert int((d['y_test'] == 0).sum()) >= 2, int((d['y_test'] == 0).sum())
    return d


def _split(d):
    off = np.concatenate([[0], np.cumsum(d['sizes'])])
    Xs = [torch.from_numpy(d['X_train'][off[i]:off[i + 1]].copy()) for i in range(len(d['sizes']))]
    ys = [torch.from_numpy(d['y_train'][off[i]:off[i + 1]].copy()) for i in range(len(d['sizes']))]
    return Xs, ys, torch.from_numpy(d['X_test']), torch.from_numpy(d['y_test'])


def _valid(d):
    return torch.utils.data.DataLoader(
        torch.utils.data.TensorDataset(torch.from_numpy(d['X_val']), torch.from_numpy(d['y_val'])),
        batch_size=BV, shuffle=True)


def _fedamw_par(X_train, y_train, X_test, y_test, validloader, type, num_classes, D, lr, epoch,
                batch_size, prox, mu, lambda_reg_if, lambda_reg, round, lr_p):
    """Harness: FedAMW with a fresh copy of the global model per client (make_golden.py's
    _fedamw_par with the criterion of tools.py:421-422)."""
    model = T.MLP(D, num_classes).to(T.device)
    n = np.array([len(y) for y in y_train])
    p = torch.tensor(n / sum(n), dtype=torch.float32, requires_grad=True)
    opt = torch.optim.SGD([p], lr_p, momentum=0.9)
    crit = torch.nn.MSELoss(reduction='mean')
    out = [torch.zeros(round) for _ in range(3)]
    for t in range(round):
        lr = T.update_learning_rate(t, lr, round)
        Ws, losses = [], []
        for i in range(len(y_train)):
            local = copy.deepcopy(model)
            w, l, _ = T.train_loop(X_train[i], y_train[i], type=type, model=local, lr=lr, epoch=epoch,
                                   batch_size=batch_size, prox=prox, mu=mu,
                                   lambda_reg_if=lambda_reg_if, lambda_reg=lambda_reg)
            Ws.append(copy.deepcopy(w)['classifier.weight'])
            losses.append(l)
        out[0][t] = torch.sum(p * torch.tensor(losses)).detach()
        Wst = torch.stack(Ws, dim=2)
        for _ in range(round):
            for data, label in validloader:
                opt.zero_grad()
                o = torch.matmul(torch.matmul(Wst.permute(2, 0, 1), data.T).permute(2, 1, 0), p)
                crit(o, label).backward()
                opt.step()
        with torch.no_grad():
            g = Ws[0] * p[0]
            for j in range(1, len(Ws)):
                g = g + p[j] * Ws[j]
        model.load_state_dict({'classifier.weight': g})
        out[1][t], out[2][t] = T.test_loop(X_test=X_test, y_test=y_test, type=type, model=model,
                                           batch_size=batch_size)
    return out


ROUND_CASES = [
    ('mse_fedavg_seq', 'fedavg', 'seq', dict(lr=0.5, prox=False, mu=0.0, reg=False, lam=0.0)),
    ('mse_fedavg_par', 'fedavg', 'par', dict(lr=0.5, prox=False, mu=0.0, reg=False, lam=0.0)),
    ('mse_fedprox_seq', 'fedprox', 'seq', dict(lr=0.5, prox=True, mu=0.5, reg=True, lam=0.1)),
    ('mse_fedprox_par', 'fedprox', 'par', dict(lr=0.05, prox=True, mu=0.5, reg=True, lam=0.1)),
    ('mse_fedamw_seq', 'fedamw', 'seq', dict(lr=0.05, prox=False, mu=0.0, reg=True, lam=0.01, lr_p=1e-5)),
    ('mse_fedamw_par', 'fedamw', 'par', dict(lr=0.5, prox=False, mu=0.0, reg=True, lam=0.01, lr_p=1e-6)),
]
SINGLE_CASES = [
    ('mse_single_centralized', 'centralized', dict(lr=0.5, epoch=3, prox=False, mu=0.0, reg=False, lam=0.0)),
    ('mse_single_distributed', 'distributed', dict(lr=0.05, epoch=2, prox=True, mu=0.5, reg=True, lam=0.1)),
    ('mse_single_oneshot', 'oneshot', dict(lr=0.5, epoch=2, prox=False, mu=0.0, reg=True, lam=0.01, R=3, lr_p=1e-5)),
]
UNIT_TRAIN = [('plain', False, False), ('prox', True, False), ('ridge', False, True), ('proxridge', True, True)]


def _f(v):
    return np.asarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)


def _rng_after():
    return torch.empty(4, dtype=torch.int64).random_().numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _loss_rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def drift_of(name, rec, data):
    d = dict(data, D=D, Bv=BV)
    d.update(rec)
    a = M.run_case(d, np.float32)
    b = M.run_case(d, np.float64)
    out = {'delta_W': _rel(a[3]['W'], b[3]['W']), 'delta_loss': max(_loss_rel(a[0], b[0]), _loss_rel(a[1], b[1]))}
    if 'p' in a[3]:
        out['delta_p'] = _rel(a[3]['p'], b[3]['p'])
    # how far the fp32 restatement sits from the reference itself (printed; the CPU test asserts it)
    ref = {'W': _rel(a[3]['W'], rec['W']), 'loss': max(_loss_rel(a[0], rec['train_loss']),
                                                         _loss_rel(a[1], rec['test_loss']))}
    if 'p' in rec:
        ref['p'] = _rel(a[3]['p'], rec['p'])
    return out, ref


def main():
    warnings.simplefilter('error')        # a broadcast warning from MSELoss would mean 1-D targets
    torch.set_num_threads(1)
    data = synth()
    np.savez_compressed(os.path.join(HERE, 'mse_data.npz'), **data, torch_seed=TORCH_SEED, C=1, D=D, Bv=BV)
    Xs, ys, Xt, yt = _split(data)
    drift = {}
    for name, algo, mode, hp in ROUND_CASES:
        _trace['W'].clear()
        _trace['p'].clear()
        pos = ('regression', 1, D, hp['lr'], EPOCH, B, hp['prox'], hp['mu'], hp['reg'], hp['lam'], R)
        torch.manual_seed(TORCH_SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            if algo == 'fedamw':
                tr, tl, ta = {'seq': T.FedAMW, 'par': _fedamw_par}[mode](Xs, ys, Xt, yt, _valid(data), *pos, hp['lr_p'])
            else:
                fn = {'seq': T.FedAvg if algo == 'fedavg' else T.FedProx, 'par': G._fed_par}[mode]
                tr, tl, ta = fn(Xs, ys, Xt, yt, *pos)
        rec = {k: np.asarray(v) for k, v in hp.items()}
        rec.update(algo=algo, mode=mode, epoch=EPOCH, batch_size=B, R=R, torch_seed=TORCH_SEED, train_loss=_f(tr),
                   test_loss=_f(tl), test_acc=_f(ta), W=np.stack(_trace['W']), rng_after=_rng_after())
        if _trace['p']:
            rec['p'] = np.stack(_trace['p'])
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **rec)
        drift[name], ref = drift_of(name, rec, data)
        print(name, 'test loss', np.round(_f(tl), 3), 'acc', _f(ta)[:1], 'drift', drift[name], 'vs reference', ref)
    for name, algo, hp in SINGLE_CASES:
        _trace['W'].clear()
        _trace['p'].clear()
        pos = ('regression', 1, D, hp['lr'], hp['epoch'], B, hp['prox'], hp['mu'], hp['reg'], hp['lam'])
        torch.manual_seed(TORCH_SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            if algo == 'centralized':
                tr, tl, ta = T.Centralized(Xs, ys, Xt, yt, *pos)
            elif algo == 'distributed':
                tr, tl, ta = T.Distributed(Xs, ys, Xt, yt, *pos)
            else:
                tr, tl, ta = T.FedAMW_OneShot(Xs, ys, Xt, yt, _valid(data), *pos, hp['R'], hp['lr_p'])
        rec = {k: np.asarray(v) for k, v in hp.items()}
        rec.update(algo=algo, batch_size=B, torch_seed=TORCH_SEED, train_loss=_f(tr), test_loss=_f(tl),
                   test_acc=_f(ta), W=np.stack(_trace['W']), rng_after=_rng_after())
        if _trace['p']:
            rec['p'] = np.stack(_trace['p'])
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **rec)
        drift[name], ref = drift_of(name, rec, data)
        print(name, 'test loss', np.round(_f(tl), 3), 'drift', drift[name], 'vs reference', ref)
    # one train_loop call from a start moved off the initialisation (client 1: 70 rows), one test_loop call
    X1, y1 = Xs[1], ys[1]
    for tag, prox, reg in UNIT_TRAIN:
        torch.manual_seed(123)
        model = T.MLP(D, 1)
        with torch.no_grad():
            model.classifier.weight.add_(0.5 * torch.randn(1, D))
        W0 = model.classifier.weight.detach().clone().numpy()
        torch.manual_seed(7)
        w, loss, _ = T.train_loop(X1, y1, 'regression', model, 0.5, 3, B, prox, 0.5, reg, 0.1)
        rec = dict(W0=W0, W=w['classifier.weight'].numpy().copy(), loss=np.float64(loss), lr=0.5, epoch=3,
                   batch_size=B, prox=prox, mu=0.5, reg=reg, lam=0.1, seed=7, client=1, rng_after=_rng_after())
        np.savez_compressed(os.path.join(HERE, 'mse_unit_train_%s.npz' % tag), **rec)
        out = {}
        for T_ in (np.float32, np.float64):
            torch.manual_seed(7)
            out[T_] = M.train_client(X1.numpy(), y1.numpy(), W0, 0.5, 3, B, prox, 0.5, reg, 0.1, T_)
        drift['mse_unit_train_' + tag] = {'delta_W': _rel(out[np.float32][0], out[np.float64][0]),
                                          'delta_loss': _loss_rel(out[np.float32][1], out[np.float64][1])}
        print('mse_unit_train_' + tag, 'loss', loss, 'drift', drift['mse_unit_train_' + tag], 'vs reference',
              _rel(out[np.float32][0], rec['W'].reshape(-1)), _loss_rel(out[np.float32][1], loss))
    torch.manual_seed(5)
    model = T.MLP(D, 1)
    with torch.no_grad():
        model.classifier.weight.mul_(40.0)
    W = model.classifier.weight.detach().clone().numpy()
    torch.manual_seed(9)
    with contextlib.redirect_stdout(io.StringIO()):
        tl, ta = G._orig_test_loop(Xt, yt, 'regression', model, B)
    np.savez_compressed(os.path.join(HERE, 'mse_unit_test.npz'), W=W, loss=np.float64(tl), acc=np.float64(ta), seed=9,
                        batch_size=B, rng_after=_rng_after())
    out = {}
    for T_ in (np.float32, np.float64):
        torch.manual_seed(9)
        out[T_] = M.test_eval(Xt.numpy(), yt.numpy(), W, B, T_)
    drift['mse_unit_test'] = {'delta_loss': _loss_rel(out[np.float32][0], out[np.float64][0])}
    print('mse_unit_test', tl, ta, 'drift', drift['mse_unit_test'], 'vs reference', _loss_rel(out[np.float32][0], tl))
    for name, rec in drift.items():
        for k in [k for k in rec if k.startswith('delta_')]:
            assert rec[k] <= 5e-6, (name, k, rec[k])       # the 1e-5 floor stays the operative bound
            rec['rtol_' + k[6:]] = max(1e-5, 2.0 * rec[k])
    with open(os.path.join(HERE, 'mse_drift.json'), 'w') as f:
        json.dump(drift, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()

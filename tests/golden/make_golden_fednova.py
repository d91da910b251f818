"""Golden vectors for FedNova (``nova_*.npz``, ``fednova_drift.json``).

Run only where the reference is installed: ``python tests/golden/make_golden_fednova.py``.
It imports the reference through ``make_golden`` (``MG.T``, unmodified, with its recording
``test_loop``) as the participation generator does, and calls the reference's own ``T.FedNova``
(tools.py:383-410; exp.py:124 leaves the call commented out, the function is intact).  Nothing of
the reference's text is restated here.

Four cases, each N = 5-6 unequal clients with one smaller than B, D = 64, R = 3:
  nova_ce        classification, C = 4
  nova_ce_ridge  the same with the ridge term on
  nova_prox      prox=True
  nova_mse       regression, C = 1, B = 32 (float targets [n, 1], clipped to [0, 100])
Each file holds the inputs, the hyper-parameters, the three returns, ``W`` after every round and
``rng_after`` (four draws from the global generator after the run).  The files are named ``nova_*``
because tests/fixtures.py globs ``fed*.npz`` for the FedAvg / FedProx / FedAMW round cases.

fednova_drift.json: per case, delta = the distance of the float32 and the float64 run of
tests/fednova_restatement.py (W: max over rounds of max|W32 - W64| / max|W64|; loss: the larger
of the train and test loss distances, absolute / max(1, |l|)) and the bounds max(1e-5, 2 delta)
the tests use -- the method of horizon_drift.py.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as MG  # noqa: E402  (imports the reference unmodified and wraps its test_loop)
from tests import fednova_restatement as FR  # noqa: E402

T = MG.T
TORCH_SEED = 100


def synth_regression(seed, sizes, n_test, n_raw, D):
    """make_golden_mse.py's synthetic regression data at this script's shapes."""
    rs = np.random.RandomState(seed)
    total = sum(sizes) + n_test
    Xraw = (rs.rand(total, n_raw) < 0.3).astype(np.float32)
    Wr = rs.normal(0, 0.5, size=(n_raw, D)).astype(np.float32)
    br = rs.uniform(0, 2 * np.pi, size=(1, D)).astype(np.float32)
    phi = (np.cos(Xraw @ Wr + br) / np.sqrt(D)).astype(np.float32)
    z = phi @ rs.normal(size=D).astype(np.float32)
    y = np.clip(40.0 + 30.0 * (z - z.mean()) / z.std() + 2.0 * rs.normal(size=total), 0.0, 100.0).astype(np.float32)
    nt0 = sum(sizes)
    order = np.argsort(y[:nt0] + 15.0 * rs.normal(size=nt0))      # client skew along the target
    return dict(X_train=phi[order], y_train=y[order].reshape(-1, 1), sizes=np.array(sizes, np.int64),
                X_test=phi[nt0:], y_test=y[nt0:].reshape(-1, 1))


CASES = [
    # name, type, data kwargs, hyper-parameters
    ('nova_ce', 'classification', dict(seed=41, sizes=[37, 5, 112, 64, 9], n_test=50, n_raw=12, D=64, C=4),
     dict(lr=0.5, epoch=2, batch_size=32, prox=False, mu=0.0, reg=False, lam=0.0, R=3)),
    ('nova_ce_ridge', 'classification', dict(seed=42, sizes=[45, 32, 7, 64, 20, 33], n_test=45, n_raw=12, D=64, C=4),
     dict(lr=0.5, epoch=2, batch_size=32, prox=False, mu=0.0, reg=True, lam=0.001, R=3)),
    ('nova_prox', 'classification', dict(seed=43, sizes=[33, 65, 3, 20, 96], n_test=61, n_raw=10, D=64, C=4),
     dict(lr=0.5, epoch=2, batch_size=32, prox=True, mu=0.05, reg=False, lam=0.0, R=3)),
    ('nova_mse', 'regression', dict(seed=44, sizes=[37, 70, 33, 11, 50], n_test=45, n_raw=14, D=64),
     dict(lr=0.05, epoch=2, batch_size=32, prox=False, mu=0.0, reg=False, lam=0.0, R=3)),
]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a, b))


def _loss_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def run_case(name, type, dk, hp):
    C = dk.get('C', 1)
    d = MG.synth(**dk) if type == 'classification' else synth_regression(**dk)
    Xs, ys, Xt, yt = MG._split(d)
    MG._trace['W'].clear()
    MG._trace['p'].clear()
    torch.manual_seed(TORCH_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        tr, tl, ta = T.FedNova(Xs, ys, Xt, yt, type, C, dk['D'], hp['lr'], hp['epoch'], hp['batch_size'], hp['prox'],
                               hp['mu'], hp['reg'], hp['lam'], hp['R'])
    rng_after = torch.empty(4, dtype=torch.int64).random_().numpy()
    rec = dict(d)
    rec.update({k: np.asarray(v) for k, v in hp.items()})
    rec.update(algo='fednova', mode='seq', type=type, C=C, D=dk['D'], torch_seed=TORCH_SEED,
               train_loss=tr.detach().numpy().astype(np.float64), test_loss=tl.numpy().astype(np.float64),
               test_acc=ta.numpy().astype(np.float64), W=np.stack(MG._trace['W']), rng_after=rng_after)
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **rec)
    a, b = FR.run_case(rec, np.float32), FR.run_case(rec, np.float64)
    drift = {'delta_W': _rel(a[3]['W'], b[3]['W']), 'delta_loss': max(_loss_rel(a[0], b[0]), _loss_rel(a[1], b[1])),
             'restatement_vs_reference_W': _rel(a[3]['W'], rec['W']),
             'restatement_vs_reference_loss': max(_loss_rel(a[0], rec['train_loss']), _loss_rel(a[1], rec['test_loss']))}
    drift['rtol_W'] = max(1e-5, 2.0 * drift['delta_W'])
    drift['rtol_loss'] = max(1e-5, 2.0 * drift['delta_loss'])
    print(name, 'max|W|', [float(np.abs(w).max()) for w in rec['W']], 'test loss', np.round(rec['test_loss'], 4),
          'acc', np.round(rec['test_acc'], 2), drift, flush=True)
    return drift


if __name__ == '__main__':
    torch.set_num_threads(1)
    out = {name: run_case(name, type, dk, hp) for name, type, dk, hp in CASES}
    with open(os.path.join(HERE, 'fednova_drift.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)

"""Helpers to load the FedNova fixtures written by tests/golden/make_golden_fednova.py
(``nova_*.npz`` -- not ``fednova_*``: tests/fixtures.py globs ``fed*.npz`` for the FedAvg / FedProx /
FedAMW round cases) and the bounds derived for them (fednova_drift.json: per case and quantity
max(1e-5, 2 delta), delta the float32-versus-float64 distance of tests/fednova_restatement.py --
the method of horizon_drift.py, the project's rule as in tests/mse_fixtures.py)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

CASES = ['nova_ce', 'nova_ce_ridge', 'nova_prox', 'nova_mse']

with open(os.path.join(GOLDEN, 'fednova_drift.json')) as _f:
    DRIFT = json.load(_f)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def split_clients(d):
    off = np.concatenate([[0], np.cumsum(d['sizes'])])
    Xs = [d['X_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]
    ys = [d['y_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]
    return Xs, ys


def positional(d):
    """The positional hyper-parameters, in the reference's order (tools.py:383)."""
    return (str(d['type']), int(d['C']), int(d['D']), float(d['lr']), int(d['epoch']), int(d['batch_size']),
            bool(d['prox']), float(d['mu']), bool(d['reg']), float(d['lam']), int(d['R']))


def rtol(name, what):
    """The bound of case ``name`` for ``what`` in 'W', 'loss': max(1e-5, 2 delta)."""
    r = DRIFT[name]['rtol_' + what]
    assert r >= 1e-5
    return r


def acc_tol(d):
    return 100.0 / len(d['y_test']) + 1e-4


def w_err(W, Wref):
    """Per round, max|W - W_ref| / max|W_ref|."""
    W, Wref = np.asarray(W, np.float64), np.asarray(Wref, np.float64)
    assert W.shape == Wref.shape, (W.shape, Wref.shape)
    return np.array([np.abs(W[t] - Wref[t]).max() / np.abs(Wref[t]).max() for t in range(W.shape[0])])


def loss_err(got, ref):
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def check_against(name, d, tr, tl, ta, W, ref=None, rtol_W=None, rtol_loss=None):
    """The project's bounds (fixtures.py:63-69) with the derived floor, against the fixture's
    reference returns or against ``ref`` = (train_loss, test_loss, test_acc, W)."""
    rtr, rtl, rta, rW = ref if ref is not None else (d['train_loss'], d['test_loss'], d['test_acc'], d['W'])
    bw = rtol(name, 'W') if rtol_W is None else rtol_W
    bl = rtol(name, 'loss') if rtol_loss is None else rtol_loss
    ew = w_err(W, rW)
    el = max(loss_err(tr, rtr), loss_err(tl, rtl))
    print('%s: W err per round %s (bound %.3g), loss err %.3g (bound %.3g)' % (name, ew, bw, el, bl))
    assert ew.max() <= bw, (name, 'W', ew)
    assert el <= bl, (name, 'loss', el)
    assert np.abs(np.asarray(ta, np.float64) - np.asarray(rta, np.float64)).max() <= acc_tol(d), name

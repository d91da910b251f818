"""Helpers to load the regression fixtures written by tests/golden/make_golden_mse.py and the
bounds derived for them (mse_drift.json: per case and quantity max(1e-5, 2 delta), delta the
float32-versus-float64 distance of tests/mse_restatement.py -- the method of horizon_drift.py)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

ROUND_CASES = ['mse_fedavg_seq', 'mse_fedavg_par', 'mse_fedprox_seq', 'mse_fedprox_par', 'mse_fedamw_seq',
               'mse_fedamw_par']
SINGLE_CASES = ['mse_single_centralized', 'mse_single_distributed', 'mse_single_oneshot']
TRAIN_UNITS = ['mse_unit_train_plain', 'mse_unit_train_prox', 'mse_unit_train_ridge', 'mse_unit_train_proxridge']

with open(os.path.join(GOLDEN, 'mse_drift.json')) as _f:
    DRIFT = json.load(_f)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def load_case(name):
    """mse_data.npz (the shared inputs) merged with the case's hyper-parameters and outputs."""
    d = load('mse_data')
    d.update(load(name))
    return d


def split_clients(d):
    off = np.concatenate([[0], np.cumsum(d['sizes'])])
    Xs = [d['X_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]
    ys = [d['y_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]       # [n_j, 1] float targets
    return Xs, ys


def rtol(name, what):
    """The bound of case ``name`` for ``what`` in 'W', 'p', 'loss': max(1e-5, 2 delta)."""
    r = DRIFT[name]['rtol_' + what]
    assert r >= 1e-5
    return r


def acc_tol(d):
    return 100.0 / len(d['y_test']) + 1e-4


def check_against(name, d, tr, tl, ta, trace):
    """The project's bounds (fixtures.py:63-69) with the derived floor: W per round and p
    relative to the maximum magnitude, losses within rtol * max(1, |l|), accuracy within one
    test sample."""
    W, Wref = np.asarray(trace['W'], np.float64), d['W']
    assert W.shape == Wref.shape, (W.shape, Wref.shape)
    for t in range(W.shape[0]):
        err = np.abs(W[t] - Wref[t]).max() / np.abs(Wref[t]).max()
        assert err <= rtol(name, 'W'), (name, 'W', t, err)
    for got, key in ((tr, 'train_loss'), (tl, 'test_loss')):
        got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(d[key])
        err = (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()
        assert err <= rtol(name, 'loss'), (name, key, err)
    assert np.abs(np.atleast_1d(np.asarray(ta, np.float64)) - np.atleast_1d(d['test_acc'])).max() <= acc_tol(d), name
    if 'p' in d:
        err = np.abs(np.asarray(trace['p'], np.float64) - d['p']).max() / np.abs(d['p']).max()
        assert err <= rtol(name, 'p'), (name, 'p', err)

"""The numpy restatement of SCAFFOLD (tests/scaffold_restatement.py) against the oracle's step, the
properties that pin the signs of both variates, the invariant c = sum_j p_j c_j, the recorded
float32 drift, the drop-in's host tables and the header.  No GPU."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import fedsim_oracle as O
from tests import scaffold_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _client(seed=3, n=23, D=20, C=3):
    rs = np.random.RandomState(seed)
    X = (rs.normal(size=(n, D)) / np.sqrt(D)).astype(np.float32)
    y = rs.randint(0, C, size=n)
    W = rs.normal(size=(C, D)).astype(np.float32) * 0.3
    return X, y, W


@pytest.mark.parametrize('reg', [False, True])
def test_zero_variates_are_the_oracles_step(reg):
    """c = c_i = 0: the client step is bitwise O.train_client, and the new variate is (x - y)/(K lr)."""
    X, y, W = _client()
    z = np.zeros_like(W)
    torch.manual_seed(5)
    Wo, lo = O.train_client(X, y, W, 0.3, 2, 8, False, 0.0, reg, 0.01)
    torch.manual_seed(5)
    Ws, ls, ci = SR.train_client(X, y, W, 0.3, 2, 8, reg, 0.01, z, z)
    assert Ws.dtype == np.float32 and Ws.tobytes() == Wo.tobytes() and ls == lo
    inv = np.float32(1.0) / (np.float32(6) * np.float32(0.3))          # K = 2 * ceil(23 / 8)
    assert ci.tobytes() == ((W - Ws).astype(np.float32) * inv).astype(np.float32).tobytes()


def _full_gradient(X, y, W):
    """grad of the mean cross-entropy over all rows at W, float64."""
    z = X @ W.T
    z = z - z.max(axis=1, keepdims=True)
    g = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    g[np.arange(len(y)), y] -= 1.0
    return g.T @ X / len(y)


def test_drift_cancels_float64():
    """Full-batch steps (B >= n_i), E = 1, c_i = grad F_i(x), c = sum_i p_i c_i: every client's step is
    x - lr (grad F_i + c - c_i) = x - lr c, the same model for every client -- wrong with either sign
    flipped.  A scratch run gave a spread of 6e-17."""
    rs = np.random.RandomState(11)
    D, C, sizes, lr = 16, 3, [9, 30, 17, 4], 0.4
    x = rs.normal(size=(C, D)) * 0.5
    Xs = [rs.normal(size=(n, D)) / 4 + 0.3 * i for i, n in enumerate(sizes)]        # non-IID: shifted clients
    ys = [rs.randint(0, C, size=n) for n in sizes]
    ci = [_full_gradient(X, y, x) for X, y in zip(Xs, ys)]
    p = SR.weights(sizes)
    c = sum(pi * g for pi, g in zip(p, ci))
    assert max(np.abs(g - c).max() for g in ci) > 1e-2                               # the clients do drift
    torch.manual_seed(1)
    out = [SR.train_client(X, y, x, lr, 1, 32, False, 0.0, c, g, np.float64) for X, y, g in zip(Xs, ys, ci)]
    for (W, _, cn), g in zip(out, ci):
        assert np.abs(W - (x - lr * c)).max() <= 1e-12
        assert np.abs(cn - g).max() <= 1e-12          # c_i+ = c_i - c + (x - y) / lr = c_i, since y = x - lr c
    # and the plain step without variates does not agree across the clients
    torch.manual_seed(1)
    plain = [SR.train_client(X, y, x, lr, 1, 32, False, 0.0, 0 * c, 0 * c, np.float64)[0] for X, y in zip(Xs, ys)]
    assert np.abs(plain[0] - plain[1]).max() > 1e-3


@pytest.mark.parametrize('name', sorted(SR.CASES))
def test_invariant_c_is_the_weighted_mean_of_the_client_variates(name):
    """After every round |c - sum_j p_j c_j| <= (t+1)(N+4) 2^-24 (|c| + sum_j p_j |c_j|) elementwise
    over ALL N clients, for full and sampled rounds: the server fold never reads the old c_i."""
    res = SR.run_case(name)[3]
    N = len(SR.SIZES)
    p = SR.weights(SR.SIZES, SR.CASES[name]['weighting'])
    for t in range(SR.R):
        c, ci = res['c'][t].astype(np.float64), res['ci'][t].astype(np.float64)
        mean = np.tensordot(p, ci, 1)
        bound = (t + 1) * (N + 4) * U * (np.abs(c) + np.tensordot(p, np.abs(ci), 1))
        assert np.abs(c).max() > 0
        assert (np.abs(c - mean) <= bound).all(), (t, (np.abs(c - mean) / bound).max())
    if SR.CASES[name]['sched'] is not None:              # a client that sat a round out keeps its variate
        assert res['ci'][1][0].tobytes() == res['ci'][0][0].tobytes()      # client 0: rounds 0 and 2 only
        assert not res['ci'][0][1].any() and res['ci'][1][1].any()         # client 1: first trained in round 1


def test_drift_record():
    """tests/golden/scaffold_drift.json (make_golden_scaffold.py) covers every drop-in case, stays far
    below the GPU tests' bounds, and is reproduced here for one case."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'scaffold_drift.json')) as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(SR.CASES)
    for name, d in rec.items():
        assert 0 < d['delta_W'] <= 1e-5 and 0 < d['delta_c'] <= 1e-5 and 0 <= d['delta_loss'] <= 5e-6, (name, d)
    name = 'sampled_size_eta0.5'
    a, b = SR.run_case(name, np.float32), SR.run_case(name, np.float64)
    dW = max(np.abs(x - y).max() / np.abs(y).max() for x, y in zip(a[3]['W'].astype(np.float64), b[3]['W']))
    assert rec[name]['delta_W'] / 4 <= dW <= rec[name]['delta_W'] * 4


def test_host_tables_agree_with_the_restatement():
    from fedamw_amd.functions import tools
    ns, E, B = np.array(SR.SIZES), SR.E, SR.B
    assert tools.scaffold_lr_schedule(0.5, 4) == [0.5, 0.5, 0.05, 0.0005]
    for wt in ('size', 'uniform'):
        for S in (np.arange(len(ns)), SR.SCHED[0], SR.SCHED[1]):
            for lr, eta in ((0.5, 1.0), (0.05, 0.5)):
                q, r, cs, w = tools.scaffold_round_coefficients(ns, S, E, B, lr, eta, wt)
                q2, r2, cs2, w2 = SR.round_coefficients(ns, S, E, B, lr, eta, wt, np.float32)
                assert q.dtype == r.dtype == w.dtype == np.float32
                for a, b in ((q, q2), (r, r2), (w, w2)):
                    assert np.abs(a - b).max() <= U * np.abs(b).max()
                assert abs(cs - float(cs2)) <= U
                if len(S) == len(ns):
                    assert cs == 0.0
                else:
                    assert 0 < cs < 1
    q, r, cs, w = tools.scaffold_round_coefficients(ns, SR.SCHED[0], E, B, 0.5, 0.7, 'uniform')
    assert np.array_equal(q, np.full(3, np.float32(0.7 / 3))) and np.array_equal(w, np.full(3, np.float32(1 / 3)))
    K = E * -(-ns[SR.SCHED[0]] // B)
    assert np.array_equal(r, ((1.0 / len(ns)) / (K * 0.5)).astype(np.float32))
    assert cs == float(np.float32(1.0 - 3.0 / len(ns)))


def test_signature_and_python_rejections():
    from fedamw_amd.functions import tools
    sig = inspect.signature(tools.Scaffold)
    pos = [n for n, p in sig.parameters.items() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert pos == [n for n, p in inspect.signature(tools.FedAvg).parameters.items()
                   if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    kw = {n: p.default for n, p in sig.parameters.items() if p.kind == inspect.Parameter.KEYWORD_ONLY}
    assert kw == dict(server_lr=1.0, weighting='size', stats=None, verbose=True, options=None, participation=None,
                      sample_seed=0)
    Xs, ys = [torch.zeros(4, 8), torch.zeros(3, 8)], [torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)]
    a = (Xs, ys, torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='prox'):
        tools.Scaffold(*a, 'classification', 2, 8, 0.1, 1, 4, True, 0.1, False, 0.0, 1)
    with pytest.raises(ValueError, match='classification'):
        tools.Scaffold(*a, 'regression', 1, 8, 0.1, 1, 4, False, 0.1, False, 0.0, 1)
    with pytest.raises(ValueError, match='batch_size'):
        tools.Scaffold(*a, 'classification', 2, 8, 0.1, 1, 128, False, 0.1, False, 0.0, 1)
    with pytest.raises(ValueError, match='weighting'):
        tools.Scaffold(*a, 'classification', 2, 8, 0.1, 1, 4, False, 0.1, False, 0.0, 1, weighting='equal')


def test_header_declares_the_entry_points():
    from fedamw_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fedsim.h')).read()
    for name in ('fs_local_train_scaffold', 'fs_aggregate_scaffold', 'fs_plan_set_scaffold'):
        assert re.search(r'\bint %s\(' % name, src), name
        assert name in _lib.EXPORTS
    assert re.search(r'#define FS_ABI_VERSION 23\b', src) and _lib.ABI_VERSION == 23

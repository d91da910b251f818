"""tests/qffl_restatement.py on the CPU: the q-FedAvg server step's reductions and invariants, the
recorded float32 drift, the drop-in's signature and host rejections, and the header.  No GPU."""
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import fedsim_oracle as O
from tests import fedopt_restatement as FO
from tests import qffl_restatement as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24


def _inputs(seed=3, M=7, L=96, scale=0.3):
    rs = np.random.RandomState(seed)
    x = rs.normal(size=L).astype(F32)
    Ws = [(x + scale * rs.normal(size=L)).astype(F32) for _ in range(M)]
    n = rs.randint(1, 50, size=M)
    p = (n / (n.sum() + 40)).astype(F32)            # a sample: the weights do not sum to 1
    F = rs.uniform(0.2, 2.5, size=M)
    return x, Ws, p, F


@pytest.mark.parametrize('q', [0.0, 0.5, 1.0, 5.0])
def test_step_is_the_papers(q):
    """x + (L / H) S equals w - sum Delta_k / sum h_k in float64 to 1e-12."""
    x, Ws, p, F = _inputs()
    L = 3.7
    u, g = QR.coefficients(F, p, q, L, np.float64)
    x2, S, n, H, coef = QR.server(x, Ws, u, g, L, np.float64)
    ref = QR.paper_step(x, Ws, F, p, q, L)
    assert H > 0 and coef == L / H
    np.testing.assert_allclose(x2, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


def test_q0_is_the_sampled_fedavg_mean():
    """q = 0: u = p, g = 0 exactly, H = L sum_S p, and x' is the sample's weighted mean.  The restatement
    (bound (M + 5) 2^-24 sum_k |term_k| over x and the M weighted updates: per update the difference,
    the product, coef's rounding and the product with coef, M - 1 sums of the fold and the last
    sum) and the oracle's fold with f32(p_k / sum_S p) (bound
    (M + 2) 2^-24 sum_k |p_k W_k|: M products, M - 1 sums, the weights' rounding) both lie within their
    summation bounds of the float64 value."""
    x, Ws, p, F = _inputs()
    M, L = len(Ws), 2.0
    u, g = QR.coefficients(F, p, 0.0, L)
    assert u.tobytes() == p.tobytes() and not g.any()
    x2, S, n, H, coef = QR.server(x, Ws, u, g, L)
    p64 = p.astype(np.float64)
    assert H == L * sum(float(a) for a in p) and coef == F32(L / H)
    x64 = x.astype(np.float64)
    terms = (p64 / p64.sum())[:, None] * (np.stack(Ws).astype(np.float64) - x64)
    exact = x64 + terms.sum(0)
    assert (np.abs(x2 - exact) <= (M + 5) * U * (np.abs(terms).sum(0) + np.abs(x64))).all()
    w = (p64 / p64.sum()).astype(F32)
    fold = O.aggregate(Ws, w)
    prods = (p64 / p64.sum())[:, None] * np.stack(Ws).astype(np.float64)
    assert (np.abs(fold - prods.sum(0)) <= (M + 2) * U * np.abs(prods).sum(0)).all()
    np.testing.assert_allclose(prods.sum(0), exact, rtol=0, atol=1e-12)


def test_weights_grow_with_the_loss():
    """u_k / p_k = Ft^q is non-decreasing in F_k for q > 0 (after the float32 rounding too), and
    g >= 0."""
    rs = np.random.RandomState(0)
    F = np.sort(rs.uniform(0.0, 4.0, size=200))
    p = np.full(200, F32(1.0 / 200))
    for q in (0.5, 1.0, 2.0, 5.0):
        u, g = QR.coefficients(F, p, q, 2.0)
        assert u.dtype == F32 and (np.diff(u / p) >= 0).all() and (u[-1] > u[0]) and (g >= 0).all()


@pytest.mark.parametrize('q', [0.0, 1.0, 5.0])
def test_step_is_no_longer_than_the_longest_update(q):
    """H >= L U, so ||x' - x|| = (L / H) ||sum u_k d_k|| <= max_k ||d_k||."""
    x, Ws, p, F = _inputs(seed=8, scale=1.5)
    L = 2.0
    u, g = QR.coefficients(F, p, q, L)
    x2, S, n, H, coef = QR.server(x, Ws, u, g, L)
    assert H >= L * float(np.sum(u.astype(np.float64))) * (1 - 1e-15)
    assert np.linalg.norm((x2 - x).astype(np.float64)) <= np.sqrt(n.max()) * (1 + 1e-6)


def test_nonpositive_H_leaves_the_model():
    x, Ws, p, F = _inputs()
    zero = np.zeros(len(Ws), F32)
    for u, g in ((zero, zero), (p, (-1e6 * np.ones(len(Ws))).astype(F32)), (p, np.full(len(Ws), np.nan, F32))):
        x2, S, n, H, coef = QR.server(x, Ws, u, g, 2.0)
        assert coef == 0 and x2.tobytes() == x.tobytes() and not (H > 0)


def test_zero_update():
    x, Ws, p, F = _inputs()
    u, g = QR.coefficients(F, p, 1.0, 2.0)
    x2, S, n, H, coef = QR.server(x, [x] * len(Ws), u, g, 2.0)
    assert not S.any() and not n.any() and x2.tobytes() == x.tobytes() and coef > 0


def test_drift_record():
    """tests/golden/qffl_drift.json (make_golden_qffl.py) covers every drop-in case at q in {0, 1, 5},
    stays far below the GPU tests' bounds (which are therefore at least twice it), and is reproduced
    here for one case."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_qffl',
                                                  os.path.join(ROOT, 'tests', 'golden', 'make_golden_qffl.py'))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    with open(os.path.join(ROOT, 'tests', 'golden', 'qffl_drift.json')) as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(QR.CASES)
    assert {k['q'] for k in QR.CASES.values()} == {0.0, 1.0, 5.0}
    assert {k['weighting'] for k in QR.CASES.values()} == {'size', 'uniform'}
    for name, d in rec.items():
        assert 0 < d['delta_W'] < 1e-6 and 0 <= d['delta_loss'] < 1e-6 and 0 <= d['delta_F'] < 1e-6, name
        # the bounds of tests/test_gpu_qffl.py
        assert 2 * d['delta_W'] <= 2e-5 and 2 * d['delta_loss'] <= 1e-5 and 2 * d['delta_F'] <= 1e-5
    name = 'q5_size_sampled'
    got = G.drift(name)
    for k in ('delta_W', 'delta_loss', 'delta_F'):
        assert abs(got[k] - rec[name][k]) <= 0.5 * rec[name][k] + 1e-12, (k, got[k], rec[name][k])


def test_restatement_at_q0_against_fedavg():
    """q = 0 is FedAvg over the sample: the restatement's models stay within float32 rounding of the
    FedOpt restatement's plain update-form aggregate on the same training, sampled too."""
    import torch
    Xs, ys, Xt, yt = QR.case_data()
    for name in ('q0_size_full', 'q0_size_sampled'):
        a = QR.run_case(name)
        torch.manual_seed(QR.TORCH_SEED)
        b = FO.fedopt(Xs, ys, Xt, yt, 'classification', QR.C, QR.D, QR.LR, QR.E, QR.B, False, QR.MU, True, QR.LAM, QR.R,
                      rule='avgm', server_lr=1.0, beta1=0.0, beta2=0.0, tau=0.1, sched=QR.case_sched(name))
        assert np.abs(a[3]['W'] - b[3]['W']).max() <= 1e-5 * np.abs(b[3]['W']).max()
        assert np.abs(a[0] - b[0]).max() <= 1e-5
        assert np.isfinite(a[3]['F']).all() and (a[3]['hc'][:, 0] > 0).all()
        assert np.isnan(a[3]['n']).any() == (name == 'q0_size_sampled')


def test_signature_and_python_rejections():
    from fedamw_amd import engine
    from fedamw_amd.functions import tools
    pos_avg = [n for n, p in inspect.signature(tools.FedAvg).parameters.items()
               if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    sig = inspect.signature(tools.QFedAvg)
    assert [n for n, p in sig.parameters.items() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD] == pos_avg
    kwo = [n for n, p in sig.parameters.items() if p.kind == inspect.Parameter.KEYWORD_ONLY]
    assert set(kwo) == {'q', 'weighting', 'lipschitz', 'stats', 'verbose', 'options', 'participation', 'sample_seed'}
    assert (sig.parameters['q'].default, sig.parameters['weighting'].default, sig.parameters['lipschitz'].default,
            sig.parameters['participation'].default, sig.parameters['sample_seed'].default,
            sig.parameters['stats'].default) == (1.0, 'size', None, None, 0, None)
    assert 'clients' not in sig.parameters and 'all N clients' in tools.QFedAvg.__doc__
    for fn in (engine.Aggregator.run_qffl, engine.RoundPlan.set_qffl, engine.qffl_coef, engine.Aggregator.qffl_ws):
        assert fn.__doc__
    # the Lipschitz schedule: 1 / lr_t with the decayed rate, or the given constant
    assert tools.qffl_lipschitz(0.5, 4) == [2.0, 2.0, 20.0, 2000.0] == QR.lipschitz_schedule(0.5, 4)
    assert tools.qffl_lipschitz(0.5, 3, 7.0) == [7.0] * 3
    # raised before any device is touched
    a = ([np.zeros((4, 8), F32)], [np.zeros(4, np.int64)], np.zeros((2, 8), F32), np.zeros(2, np.int64))
    for kw in (dict(q=-0.5), dict(q=float('nan')), dict(lipschitz=0.0), dict(lipschitz=-2.0), dict(weighting='loss')):
        with pytest.raises(ValueError):
            tools.QFedAvg(*a, 'classification', 2, 8, verbose=False, **kw)
    with pytest.raises(ValueError, match='parallel'):
        tools.Federation('qfedavg', *a, None, 'classification', 2, 8, 0.1, 1, 4, False, 0.0, False, 0.0, 2, None,
                         'sequential', verbose=False)


def test_more_than_one_rank_is_refused(monkeypatch):
    from fedamw_amd.functions import tools
    monkeypatch.setattr(tools.dist, 'world', lambda: (0, 2))
    a = ([np.zeros((4, 8), F32)] * 2, [np.zeros(4, np.int64)] * 2, np.zeros((2, 8), F32), np.zeros(2, np.int64))
    with pytest.raises(NotImplementedError, match='rank'):
        tools.QFedAvg(*a, 'classification', 2, 8, 0.1, 1, 4, verbose=False)


def test_experiment_driver_lists_the_row():
    from fedamw_amd import experiment
    assert experiment.EXTRA_FAIR == ['QFedAvg'] and 'QFedAvg' not in experiment.NAMES + experiment.EXTRA
    sig = inspect.signature(experiment.run)
    assert sig.parameters['qffl_q'].default == 1.0 and sig.parameters['qffl_weighting'].default == 'size'
    consts = experiment.main.__code__.co_consts
    assert '--qffl-q' in consts and '--qffl-weighting' in consts


def test_header_declares_the_entry_points():
    from fedamw_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fedsim.h')).read()
    for name in ('fs_aggregate_qffl', 'fs_qffl_coef', 'fs_plan_set_qffl'):
        assert re.search(r'\bint %s\(' % name, src) and name in _lib.EXPORTS
    assert re.search(r'\bint64_t fs_aggregate_qffl_ws_doubles\(int M, int64_t len\)', src)
    assert 'fs_aggregate_qffl_ws_doubles' in _lib.EXPORTS
    assert re.search(r'#define FS_ABI_VERSION\s+23\b', src) and _lib.ABI_VERSION == 23
    block = src[src.index('q-FedAvg (q-FFL'):src.index('int fs_qffl_coef(')]
    for needle in ('Additive to ABI 23', '16 * 2^-24', 'FS_OPT_AVGM', 'coef   = (float)(Lc / H)', 'FS_EINVAL',
                   'd_S == d_W_g', 'No atomics', 'q = 0 gives d_u = d_p, d_g = 0 exactly'):
        assert needle in block, needle
    plan = src[src.index('q-FedAvg on this plan'):src.index('int fs_plan_set_qffl(')]
    for needle in ('chained plan', 'SCAFFOLD on', 'server-optimizer rule', 'on = 0 restores', 'before each round'):
        assert needle in plan, needle
    assert 'aggregate_qffl' in _lib.KERNEL_SOURCES and 'aggregate_qffl.hip' in _lib.KERNEL_SOURCES['aggregate_qffl']

"""tests/fedopt_restatement.py on the CPU: the server step's reductions and invariants, the recorded
float32 drift, the drop-ins' host scalars and signatures, and the header.  No GPU."""
import inspect
import json
import os
import re

import numpy as np
import pytest

from tests import fednova_restatement as FR
from tests import fedopt_restatement as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _inputs(seed=3, M=7, L=96):
    rs = np.random.RandomState(seed)
    Ws = [rs.normal(size=L).astype(F32) for _ in range(M)]
    n = rs.randint(1, 50, size=M)
    q = (n / n.sum()).astype(F32)
    x = rs.normal(size=L).astype(F32)
    m = (0.1 * rs.normal(size=L)).astype(F32)
    return Ws, q, x, m, rs


def test_avgm_without_momentum_is_the_update_form_aggregate():
    """beta1 = 0, eta = 1: x' is bitwise fednova_restatement.aggregate_updates and m' = delta."""
    Ws, q, x, m, _ = _inputs()
    sc = FO.scalars(1.0, 0.0, 0.0, 0.1)
    x2, m2, _ = FO.server('avgm', x, m, None, Ws, q, sc)
    ref = FR.aggregate_updates(Ws, q, x, F32)
    assert x2.dtype == F32 and x2.tobytes() == ref.tobytes()
    assert m2.tobytes() == FO.delta(Ws, q, x).tobytes()


def test_adam_without_memory_steps_by_the_normalised_update():
    """beta1 = beta2 = 0: v' = delta^2, so the step is eta*delta/(|delta| + tau) -- the sign of the
    step and the denominator's form."""
    Ws, q, x, m, rs = _inputs()
    v = rs.uniform(0.5, 2.0, size=x.shape)
    sc = FO.scalars(0.3, 0.0, 0.0, 0.05, np.float64)
    d = FO.delta(Ws, q, x, np.float64)
    x2, m2, v2 = FO.finish('adam', d, x, m, v, sc, np.float64)
    np.testing.assert_allclose(x2 - x, 0.3 * d / (np.abs(d) + 0.05), rtol=1e-12, atol=0)
    np.testing.assert_allclose(m2, d, rtol=0, atol=0)
    np.testing.assert_allclose(v2, d * d, rtol=0, atol=0)
    assert (np.sign(x2 - x) == np.sign(d)).all() and (np.abs(x2 - x) < 0.3).all()


def test_adagrad_second_moment_never_decreases():
    Ws, q, x, m, rs = _inputs()
    v = rs.uniform(0.0, 1e-3, size=x.shape).astype(F32)
    sc = FO.scalars(0.1, 0.9, 0.99, 1e-3)
    for _ in range(4):
        x, m, v2 = FO.server('adagrad', x, m, v, Ws, q, sc)
        assert (v2 >= v).all() and (v2 > v).any()
        v = v2


def test_yogi_moves_v_toward_d2_by_the_scaled_square():
    """|v' - v| = fl(omb2*d2) exactly (a float32 difference of neighbours this close is exact where it
    is checked in float64) and v' moves toward d2, with v on both sides of d2 and equal to it."""
    Ws, q, x, m, rs = _inputs()
    d = FO.delta(Ws, q, x)
    d2 = (d * d).astype(F32)
    v = (d2 * rs.choice([0.25, 4.0], size=d2.shape).astype(F32)).astype(F32)
    v[::5] = d2[::5]
    sc = FO.scalars(0.1, 0.9, 0.75, 1e-3)
    _, _, v2 = FO.finish('yogi', d, x, m, v, sc)
    step = (sc[4] * d2).astype(F32)
    above, below, equal = v > d2, v < d2, v == d2
    assert above.any() and below.any() and equal.any()
    assert (v2[above] == (v - step).astype(F32)[above]).all() and (v2[above] < v[above]).all()
    assert (v2[below] == (v + step).astype(F32)[below]).all() and (v2[below] > v[below]).all()
    assert (v2[equal] == v[equal]).all()
    # omb2 = 0.25 and v in {d2/4, 4 d2}: the step never overshoots d2
    assert (v2[above] >= d2[above]).all() and (v2[below] <= d2[below]).all()
    # float64: |v' - v| is the scaled square itself
    _, _, w2 = FO.finish('yogi', d.astype(np.float64), x, m, v.astype(np.float64), FO.scalars(0.1, 0.9, 0.75, 1e-3, np.float64),
                         np.float64)
    moved = ~equal
    np.testing.assert_allclose(np.abs(w2 - v)[moved], (0.25 * d.astype(np.float64) ** 2)[moved], rtol=1e-12)


def test_zero_update_leaves_the_model():
    """delta = 0 (every client returns x): x unchanged, m' = beta1*m, adam's v' = beta2*v, nothing NaN at
    v = 0."""
    _, q, x, m, _ = _inputs()
    sc = FO.scalars(0.1, 0.9, 0.99, 1e-3)
    for rule in FO.RULES:
        x2, m2, v2 = FO.server(rule, x, np.zeros_like(m), np.zeros_like(x), [x] * len(q), q, sc)
        assert x2.tobytes() == x.tobytes() and not m2.any()
        assert rule == 'avgm' or (np.isfinite(v2).all() and not v2.any())
    v = np.full_like(x, 0.5)
    _, m2, v2 = FO.server('adam', x, m, v, [x] * len(q), q, sc)
    assert m2.tobytes() == (sc[1] * m).astype(F32).tobytes() and v2.tobytes() == (sc[3] * v).astype(F32).tobytes()


def test_server_opt_scalars():
    from fedamw_amd import _lib
    from fedamw_amd.functions import tools
    rule, eta, b1, o1, b2, o2, tau = tools.server_opt_scalars('yogi', 0.0316, 0.9, 0.99, 1e-3)
    assert rule == _lib.OPT_YOGI == 4
    assert (eta, b1, o1, b2, o2, tau) == (F32(0.0316), F32(0.9), F32(1.0 - 0.9), F32(0.99), F32(1.0 - 0.99), F32(1e-3))
    assert all(isinstance(a, np.float32) for a in (eta, b1, o1, b2, o2, tau))
    # the subtraction is float64's on the caller's beta: not 1 - f32(beta), which differs
    assert o2 != F32(F32(1.0) - F32(0.99))
    assert (eta, b1, o1, b2, o2, tau) == FO.scalars(0.0316, 0.9, 0.99, 1e-3)
    assert [tools.server_opt_scalars(r)[0] for r in FO.RULES] == [1, 2, 3, 4]
    assert tools.server_opt_scalars('avgm')[1] == F32(1.0) and tools.server_opt_scalars('adam')[1] == F32(0.1)
    assert (_lib.OPT_AVGM, _lib.OPT_ADAGRAD, _lib.OPT_ADAM, _lib.OPT_YOGI) == (1, 2, 3, 4)
    for bad in (dict(server_opt='sgd'), dict(tau=0.0), dict(tau=-1.0), dict(beta1=1.0), dict(beta1=-0.1),
                dict(beta2=1.0), dict(server_lr=0.0), dict(server_lr=-1.0)):
        kw = dict(server_opt='adam', server_lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
        kw.update(bad)
        with pytest.raises(ValueError):
            tools.server_opt_scalars(**kw)


def test_signatures_and_python_rejections():
    from fedamw_amd.functions import tools
    pos_avg = [n for n, p in inspect.signature(tools.FedAvg).parameters.items()
               if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    for fn in (tools.FedOpt, tools.FedAvgM, tools.FedAdagrad, tools.FedAdam, tools.FedYogi):
        sig = inspect.signature(fn)
        pos = [n for n, p in sig.parameters.items() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
        assert pos == pos_avg, fn.__name__
        for n in ('server_lr', 'beta1', 'stats', 'verbose', 'options', 'participation', 'sample_seed'):
            assert sig.parameters[n].kind == inspect.Parameter.KEYWORD_ONLY
        assert 'clients' not in sig.parameters
    sig = inspect.signature(tools.FedOpt)
    assert sig.parameters['server_opt'].default == 'adam' and sig.parameters['v0'].default is None
    assert (sig.parameters['beta1'].default, sig.parameters['beta2'].default, sig.parameters['tau'].default) == \
        (0.9, 0.99, 1e-3)
    assert inspect.signature(tools.FedAvgM).parameters['server_lr'].default == 1.0
    assert 'beta2' not in inspect.signature(tools.FedAvgM).parameters
    for fn in (tools.FedAdagrad, tools.FedAdam, tools.FedYogi):
        assert inspect.signature(fn).parameters['server_lr'].default == 0.1 and 'not a tuned value' in fn.__doc__
    # raised before any device is touched
    a = ([np.zeros((4, 8), F32)], [np.zeros(4, np.int64)], np.zeros((2, 8), F32), np.zeros(2, np.int64))
    for kw in (dict(server_opt='sgd'), dict(tau=0.0), dict(beta1=1.0), dict(beta2=-0.5), dict(server_lr=0.0)):
        with pytest.raises(ValueError):
            tools.FedOpt(*a, 'classification', 2, 8, verbose=False, **kw)


def test_drift_record():
    """tests/golden/fedopt_drift.json (make_golden_fedopt.py) covers every drop-in case, stays far
    below the GPU tests' bounds, holds YOGI's sign margin, and is reproduced here for one case."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_fedopt',
                                                  os.path.join(ROOT, 'tests', 'golden', 'make_golden_fedopt.py'))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    with open(os.path.join(ROOT, 'tests', 'golden', 'fedopt_drift.json')) as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(FO.CASES)
    assert len(FO.CASES) == 11 and {k['rule'] for k in FO.CASES.values()} == set(FO.RULES)
    for name, d in rec.items():
        assert 0 < d['delta_W'] < 1e-6 and 0 <= d['delta_loss'] < 1e-6, name
        assert ('yogi_sign_margin' in d) == (FO.CASES[name]['rule'] == 'yogi')
        assert d.get('yogi_sign_margin', 1.0) > G.SIGN_MARGIN == 4e-5
    name = 'yogi_sampled'
    got = G.drift(name)
    for k, v in rec[name].items():
        assert abs(got[k] - v) <= 0.5 * v + 1e-12, (k, got[k], v)     # (libm and BLAS builds differ in the last bits)


def test_restatement_against_fedavg():
    """avgm with beta1 = 0, eta = 1 is FedAvg's update form: the restatement's models stay within
    float32 rounding of the plain aggregate's on the same training (parallel clients)."""
    import torch
    Xs, ys, Xt, yt = FO.case_data()
    torch.manual_seed(FO.TORCH_SEED)
    a = FO.fedopt(Xs, ys, Xt, yt, 'classification', FO.C, FO.D, FO.LR, FO.E, FO.B, False, 0.0, True, FO.LAM, FO.R,
                  rule='avgm', server_lr=1.0, beta1=0.0, beta2=0.0, tau=0.1)
    torch.manual_seed(FO.TORCH_SEED)
    b = FR.fednova(Xs, ys, Xt, yt, 'classification', FO.C, FO.D, FO.LR, FO.E, FO.B, False, 0.0, True, FO.LAM, FO.R,
                   clients='parallel', rule='fedavg')
    assert np.abs(a[3]['W'] - b[3]['W']).max() <= 1e-5 * np.abs(b[3]['W']).max()
    assert np.abs(a[0] - b[0]).max() <= 1e-5


def test_header_declares_the_entry_points():
    from fedamw_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'fedsim.h')).read()
    for name in ('fs_aggregate_opt', 'fs_plan_set_server_opt'):
        assert re.search(r'\bint %s\(' % name, src) and name in _lib.EXPORTS
    for k, name in enumerate(('FS_OPT_AVGM', 'FS_OPT_ADAGRAD', 'FS_OPT_ADAM', 'FS_OPT_YOGI'), 1):
        assert re.search(r'#define %s\s+%d\b' % (name, k), src)
    assert re.search(r'#define FS_ABI_VERSION\s+23\b', src) and _lib.ABI_VERSION == 23
    block = src[src.index('FedOpt server optimizers'):src.index('int fs_aggregate_opt(')]
    for needle in ('Additive to ABI 23', 'sgn(fl(v - d2))', 'correctly rounded IEEE', 'FS_EINVAL', 'FS_NOVA_UPDATES'):
        assert needle in block, needle

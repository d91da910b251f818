"""The regression task on the CPU: the numpy restatement (tests/mse_restatement.py, float32)
against the unmodified reference's fixtures (tests/golden/mse_*.npz), and the drop-ins' input
checks, which run before any device is touched."""
import numpy as np
import pytest
import torch

from tests import mse_restatement as M
from tests.mse_fixtures import (DRIFT, ROUND_CASES, SINGLE_CASES, TRAIN_UNITS, check_against, load, load_case, rtol)


def _rng_after():
    return torch.empty(4, dtype=torch.int64).random_().numpy()


@pytest.mark.parametrize('name', ROUND_CASES + SINGLE_CASES)
def test_restatement_reproduces_the_reference(name):
    d = load_case(name)
    tr, tl, ta, trace = M.run_case(d, np.float32)
    check_against(name, d, tr, tl, ta, trace)
    np.testing.assert_array_equal(_rng_after(), d['rng_after'])      # the generator is consumed draw for draw


@pytest.mark.parametrize('name', TRAIN_UNITS)
def test_train_loop_unit(name):
    data, d = load('mse_data'), load(name)
    off = np.concatenate([[0], np.cumsum(data['sizes'])])
    j = int(d['client'])
    X, y = data['X_train'][off[j]:off[j + 1]], data['y_train'][off[j]:off[j + 1]]
    torch.manual_seed(int(d['seed']))
    w, loss = M.train_client(X, y, d['W0'], float(d['lr']), int(d['epoch']), int(d['batch_size']), bool(d['prox']),
                             float(d['mu']), bool(d['reg']), float(d['lam']), np.float32)
    assert np.abs(w - d['W'].reshape(-1)).max() <= rtol(name, 'W') * np.abs(d['W']).max()
    assert abs(loss - float(d['loss'])) <= rtol(name, 'loss') * max(1.0, abs(float(d['loss'])))
    np.testing.assert_array_equal(_rng_after(), d['rng_after'])


def test_test_loop_unit():
    data, d = load('mse_data'), load('mse_unit_test')
    torch.manual_seed(int(d['seed']))
    loss, acc = M.test_eval(data['X_test'], data['y_test'], d['W'], int(d['batch_size']), np.float32)
    assert abs(loss - float(d['loss'])) <= rtol('mse_unit_test', 'loss') * max(1.0, abs(float(d['loss'])))
    zeros = int((data['y_test'] == 0).sum())
    assert zeros >= 2
    assert abs(float(d['acc']) - 100.0 * zeros / len(data['y_test'])) <= 1e-4     # the degenerate accuracy
    assert abs(acc - float(d['acc'])) <= 1e-4
    np.testing.assert_array_equal(_rng_after(), d['rng_after'])


def test_drift_file_keeps_the_floor_operative():
    """Every delta of mse_drift.json is <= 5e-6, so every bound is the project's 1e-5 floor."""
    for name, rec in DRIFT.items():
        for k, v in rec.items():
            if k.startswith('delta_'):
                assert v <= 5e-6, (name, k, v)
                assert rec['rtol_' + k[6:]] == max(1e-5, 2.0 * v)


def _call(y_train, y_test, type='regression', num_classes=1):
    from fedamw_amd.functions import tools
    X = [torch.zeros(6, 8), torch.zeros(5, 8)]
    return tools.FedAvg(X, y_train, torch.zeros(4, 8), y_test, type, num_classes, 8, 0.1, 1, 4, False, 0.0, False,
                        0.0, 2, verbose=False)


def _targets(fill=1.0, dtype=torch.float32):
    return [torch.full((6, 1), fill, dtype=dtype), torch.full((5, 1), fill, dtype=dtype)], \
        torch.full((4, 1), fill, dtype=dtype)


def test_one_dimensional_float_targets_are_rejected():
    """The reference broadcasts a [B, 1] output against [B] targets into a [B, B] loss; the
    drop-in refuses and names the fix.  (Fails on a tree without the regression task, which
    raises NotImplementedError for every non-classification type.)"""
    ys, yt = _targets()
    with pytest.raises(ValueError, match=r'reshape\(-1, 1\)') as e:
        _call([y.reshape(-1) for y in ys], yt)
    assert 'broadcast' in str(e.value)
    with pytest.raises(ValueError, match=r'reshape\(-1, 1\)'):
        _call(ys, yt.reshape(-1))


def test_regression_needs_one_output():
    ys, yt = _targets()
    with pytest.raises(NotImplementedError, match='num_classes'):
        _call(ys, yt, num_classes=2)


def test_integer_targets_are_rejected():
    ys, yt = _targets(dtype=torch.int64)
    with pytest.raises(ValueError, match='floating'):
        _call(ys, yt)


def test_non_finite_targets_are_rejected():
    ys, yt = _targets()
    ys[1][2, 0] = float('inf')
    with pytest.raises(ValueError, match='finite'):
        _call(ys, yt)
    ys, yt = _targets()
    yt[0, 0] = float('nan')
    with pytest.raises(ValueError, match='finite'):
        _call(ys, yt)


def test_unknown_type_is_a_value_error():
    ys, yt = _targets()
    with pytest.raises(ValueError, match='type'):
        _call(ys, yt, type='ranking')

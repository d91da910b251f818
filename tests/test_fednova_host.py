"""FedNova's host side: the drop-in's signature, its keyword checks (raised before any device is
touched), the header's declarations and the ABI number.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from fedamw_amd import _lib
from fedamw_amd.functions import tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools.py:383 of the reference: the positional parameters and their defaults
REFERENCE_SIGNATURE = [('X_train', inspect.Parameter.empty), ('y_train', inspect.Parameter.empty),
                       ('X_test', inspect.Parameter.empty), ('y_test', inspect.Parameter.empty),
                       ('type', 'classification'), ('num_classes', 10), ('D', 200), ('lr', 0.01), ('epoch', 2),
                       ('batch_size', 32), ('prox', False), ('mu', 0.1), ('lambda_reg_if', False), ('lambda_reg', 0.01),
                       ('round', 100)]


def test_signature_is_the_references():
    sig = inspect.signature(tools.FedNova)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert pos == REFERENCE_SIGNATURE
    kw = {n: p.default for n, p in sig.parameters.items() if p.kind == inspect.Parameter.KEYWORD_ONLY}
    assert kw == dict(clients='sequential', variant='reference', stats=None, verbose=True, options=None,
                      participation=None, sample_seed=0)


def _tiny():
    Xs = [torch.zeros(4, 8), torch.zeros(3, 8)]
    ys = [torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)]
    return Xs, ys, torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64)


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a device was touched')
    monkeypatch.setattr(tools, '_device', boom)
    monkeypatch.setattr(_lib, 'lib', boom)


def test_bogus_variant_is_rejected_before_any_device(no_device):
    with pytest.raises(ValueError, match='variant'):
        tools.FedNova(*_tiny(), 'classification', 2, 8, round=1, variant='bogus')


def test_updates_variant_needs_parallel_clients(no_device):
    with pytest.raises(ValueError, match='parallel'):
        tools.FedNova(*_tiny(), 'classification', 2, 8, round=1, variant='updates', clients='sequential')
    with pytest.raises(ValueError, match='parallel'):
        tools.Federation('fednova', *_tiny(), None, 'classification', 2, 8, 0.1, 1, 4, False, 0.0, False, 0.0, 1, None,
                         'sequential', variant='updates')


def test_header_declares_the_new_entry_points():
    src = open(os.path.join(ROOT, 'include', 'fedsim.h')).read()
    assert re.search(r'\bint\s+fs_aggregate_nova\s*\(', src)
    assert re.search(r'\bint\s+fs_plan_set_nova\s*\(', src)
    assert re.search(r'#define\s+FS_NOVA_REFERENCE\s+1\b', src) and re.search(r'#define\s+FS_NOVA_UPDATES\s+2\b', src)
    assert 'fs_aggregate_nova' in _lib.EXPORTS and 'fs_plan_set_nova' in _lib.EXPORTS
    assert (_lib.NOVA_REFERENCE, _lib.NOVA_UPDATES) == (1, 2)


def test_abi_version_is_23():
    src = open(os.path.join(ROOT, 'include', 'fedsim.h')).read()
    assert int(re.search(r'#define\s+FS_ABI_VERSION\s+(\d+)', src).group(1)) == 23 == _lib.ABI_VERSION


def test_host_coefficients_follow_the_restatement():
    """The drop-in's torch expressions (the reference's own) against the numpy restatement."""
    from tests import fednova_restatement as FR
    ns = np.array([37, 5, 112, 64, 9])
    p, b, te, s0 = tools.nova_reference_coefficients(ns, 2, 32)
    q, b2, te2, s02 = FR.reference_coefficients(ns, 2, 32, np.float32)
    np.testing.assert_array_equal(p.numpy(), q)
    np.testing.assert_array_equal(b.numpy(), b2)
    assert abs(te - float(te2)) <= 2e-7 * te and abs(s0 - float(s02)) <= 2e-7 * s0
    # the coefficients the reference form applies sum to N sum p^2 (1.7577 at these sizes), not to 1
    assert abs(float((p.double() * te / b.double()).sum()) - 1.7577) <= 1e-4
    p, a = tools.nova_update_coefficients(ns, 2, 32)
    np.testing.assert_allclose(a.numpy(), FR.update_coefficients(ns, 2, 32, np.float32)[1], rtol=2e-7)

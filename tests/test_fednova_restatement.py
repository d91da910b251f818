"""The numpy restatement of FedNova (tests/fednova_restatement.py) against the reference's own
``FedNova`` on the four fixture cases (tests/golden/make_golden_fednova.py), under the derived
bounds max(1e-5, 2 delta) of fednova_drift.json; and its aggregation rules against each other."""
import numpy as np
import pytest
import torch

from tests import fednova_restatement as FR
from tests.fednova_fixtures import CASES, DRIFT, check_against, load, rtol


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference(name):
    d = load(name)
    tr, tl, ta, trace = FR.run_case(d)
    check_against(name, d, tr, tl, ta, trace['W'])
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), d['rng_after'])


@pytest.mark.parametrize('name', CASES)
def test_drift_file_states_the_rule(name):
    rec = DRIFT[name]
    for what in ('W', 'loss'):
        assert rec['rtol_' + what] == max(1e-5, 2.0 * rec['delta_' + what])


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('clients', ['sequential', 'parallel'])
def test_reference_form_with_equal_sizes_is_fedavg(name, clients):
    """Equal client sizes: Tau_j = Tau_eff for every j up to rounding, so the reference form's
    coefficients are p_j and the run is FedAvg's to the case's bound."""
    d = dict(load(name))
    n = 40                                         # every client cut or wrapped to 40 rows (a ragged batch of 8)
    off = np.concatenate([[0], np.cumsum(d['sizes'])])
    rows = np.concatenate([off[j] + np.arange(n) % d['sizes'][j] for j in range(len(d['sizes']))])
    d['X_train'], d['y_train'] = d['X_train'][rows], d['y_train'][rows]
    d['sizes'] = np.full(len(d['sizes']), n, np.int64)
    nova = FR.run_case(d, clients=clients)
    avg = FR.run_case(d, clients=clients, rule='fedavg')
    check_against(name, d, *nova[:3], nova[3]['W'], ref=(avg[0], avg[1], avg[2], avg[3]['W']))


def test_reference_coefficients_sum_to_N_sum_p_squared():
    """The scale of the reference form: sum_j p_j Tau_eff / Tau_j = N sum_j p_j^2."""
    ns = np.array([37, 5, 112, 64, 9])
    p, b, te, s0 = FR.reference_coefficients(ns, 2, 32, np.float64)
    coef = p * te / b
    assert abs(coef[0] - s0) <= 1e-15
    # (p is n / sum(n) rounded to float32, 6e-8 relative: the identity holds to that)
    assert abs(coef.sum() - len(ns) * np.sum(p * p)) <= 1e-6
    assert abs(coef.sum() - 1.7577) <= 1e-4
    _, a = FR.update_coefficients(ns, 2, 32, np.float64)
    tau = 2 * np.ceil(ns / 32)
    np.testing.assert_allclose(a, p * np.sum(p * tau) / tau, rtol=1e-15)


def test_update_form_is_a_weighted_mean_of_updates():
    """W_g + sum a_j (W_j - W_g) in float64 against the closed form, and the first-term rule."""
    rs = np.random.RandomState(3)
    Ws = [rs.normal(size=(3, 8)) for _ in range(5)]
    base = rs.normal(size=(3, 8))
    a = rs.rand(5)
    got = FR.aggregate_updates(Ws, a, base, np.float64)
    np.testing.assert_allclose(got, base + sum(a[k] * (Ws[k] - base) for k in range(5)), rtol=1e-14)
    one = FR.aggregate_updates(Ws[:1], a[:1], base, np.float32)
    b32 = base.astype(np.float32)
    np.testing.assert_array_equal(one, b32 + a.astype(np.float32)[0] * (Ws[0].astype(np.float32) - b32))


def test_updates_variant_needs_parallel_clients():
    d = load('nova_ce')
    with pytest.raises(ValueError):
        FR.run_case(d, variant='updates', clients='sequential')

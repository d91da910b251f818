"""Batch sizes above 64 on the CPU: the oracle (oracle/fedsim_oracle.py) against the reference's
golden vectors at batch 65, 100, 256 and full batch (tests/golden/make_golden_bigbatch.py:
bb_*.npz), at the project's bounds (tests/fixtures.py), and what fs_local_train /
fs_local_train_plan answer for such a batch without a device (host arithmetic only)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import fedsim_oracle as O
from tests import bigbatch_cases as K
from tests import softmax_reference as R
from tests.fixtures import LOSS_RTOL, P_RTOL, W_RTOL, acc_tol, load

ROUND_CASES = ['bb_fedavg_seq', 'bb_fedavg_par', 'bb_fedprox_seq', 'bb_fedamw_par']
SINGLE_CASES = ['bb_central_256']
UNIT_B = (65, 100, 256, 300)
TRAIN_UNITS = ['bb_unit_%d_%s' % (B, tag) for B in UNIT_B for tag in ('plain', 'proxridge')]
SIZES = [130, 64, 257, 101, 1]


def load_case(name):
    """bb_data.npz (the shared inputs) merged with the case's hyper-parameters and outputs."""
    d = load('bb_data')
    d.update(load(name))
    return d


def split_clients(d):
    off = np.concatenate([[0], np.cumsum(d['sizes'])])
    Xs = [d['X_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]
    ys = [d['y_train'][off[i]:off[i + 1]] for i in range(len(d['sizes']))]
    return Xs, ys


def positional(d, rounds=True):
    """The positional hyper-parameters, in the reference's order (tools.py:329; tools.py:240 without ``round``)."""
    pos = ('classification', int(d['C']), int(d['D']), float(d['lr']), int(d['epoch']), int(d['batch_size']),
           bool(d['prox']), float(d['mu']), bool(d['reg']), float(d['lam']))
    return pos + (int(d['R']),) if rounds else pos


def check_rounds(name, d, tr, tl, ta, W, p=None):
    """W per round, the three returns and p at the project's bounds (tests/fixtures.py:63-69)."""
    Wref = d['W']
    assert W.shape == Wref.shape, (W.shape, Wref.shape)
    for t in range(W.shape[0]):
        err = np.abs(W[t] - Wref[t]).max()
        assert err <= W_RTOL * np.abs(Wref[t]).max(), (name, t, err)
    for got, key in ((tr, 'train_loss'), (tl, 'test_loss')):
        got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(d[key])
        np.testing.assert_allclose(got, ref, rtol=0, atol=LOSS_RTOL * max(1, np.abs(ref).max()), err_msg=name + ' ' + key)
    assert np.abs(np.atleast_1d(np.asarray(ta, np.float64)) - np.atleast_1d(d['test_acc'])).max() <= acc_tol(d), name
    if 'p' in d:
        assert np.abs(np.asarray(p, np.float64) - d['p']).max() <= P_RTOL * np.abs(d['p']).max(), name


def test_fixtures_are_what_the_cases_need():
    d = load('bb_data')
    assert list(d['sizes']) == SIZES and int(d['D']) == 80 and int(d['C']) == 5
    assert len(d['y_val']) % int(d['Bv']) != 0                    # a ragged validation batch
    for name in ROUND_CASES:
        assert int(load(name)['batch_size']) == 100 and int(load(name)['R']) == 3
    assert int(load('bb_central_256')['batch_size']) == 256
    assert sorted({int(load(n)['batch_size']) for n in TRAIN_UNITS}) == list(UNIT_B)
    assert max(UNIT_B) >= SIZES[2]                                # full batch: B >= n


@pytest.mark.parametrize('name', TRAIN_UNITS)
def test_train_loop_unit(name):
    u = load(name)
    Xs, ys = split_clients(load('bb_data'))
    j = int(u['client'])
    torch.manual_seed(int(u['seed']))
    W, loss = O.train_client(Xs[j], ys[j], u['W0'], float(u['lr']), int(u['epoch']), int(u['batch_size']),
                             bool(u['prox']), float(u['mu']), bool(u['reg']), float(u['lam']))
    assert np.abs(W - u['W']).max() <= W_RTOL * np.abs(u['W']).max()
    assert abs(loss - float(u['loss'])) <= LOSS_RTOL * max(1.0, abs(float(u['loss'])))
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), u['rng_after'])


@pytest.mark.parametrize('name', ROUND_CASES)
def test_round_drivers_match_reference(name):
    d = load_case(name)
    Xs, ys = split_clients(d)
    mode = 'parallel' if str(d['mode']) == 'par' else 'sequential'
    torch.manual_seed(int(d['torch_seed']))
    if str(d['algo']) == 'fedamw':
        tr, tl, ta, trace = O.FedAMW(Xs, ys, d['X_test'], d['y_test'], d['X_val'], d['y_val'], *positional(d),
                                     lr_p=float(d['lr_p']), clients=mode)
    else:
        fn = O.FedAvg if str(d['algo']) == 'fedavg' else O.FedProx
        tr, tl, ta, trace = fn(Xs, ys, d['X_test'], d['y_test'], *positional(d), clients=mode)
    check_rounds(name, d, tr, tl, ta, trace['W'], trace.get('p'))
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), d['rng_after'])


def test_centralized_256_matches_reference():
    d = load_case('bb_central_256')
    Xs, ys = split_clients(d)
    torch.manual_seed(int(d['torch_seed']))
    tr, tl, ta, trace = O.Centralized(Xs, ys, d['X_test'], d['y_test'], *positional(d, rounds=False))
    check_rounds('bb_central_256', d, tr, tl, ta, trace['W'])
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), d['rng_after'])


# ---- the inputs of the GPU test's exact and mixed cases, proven on the CPU ---------------------------

@pytest.mark.parametrize('case', K.SAT_CASES, ids=str)
def test_saturated_cases_keep_their_lead(case):
    """Every row of every step stays won by GAP_EXACT (exp(z - m) exactly 0 in fp32 for every
    loser), the first step starts GAP_START ahead, the 'all_won' client moves nothing and the
    fp32 oracle itself lands bitwise on the float64 reference rounded to fp32."""
    D, C, B = case
    Xs, ys, W0 = K.saturated_inputs(D, C, B)
    assert all(len(y) == B for y in ys) and B % 64 == 0 and B > 64
    z0 = np.concatenate(Xs).astype(np.float64) @ W0.astype(np.float64).T
    assert R._top2_gap(z0) >= R.GAP_START
    for chained in (False, True):
        torch.manual_seed(11)
        Wr, lr_, gap = R.train_chain_ref64(Xs, ys, W0, *K.saturated_args(B), chained)
        assert gap >= R.GAP_EXACT, (case, chained, gap)
        torch.manual_seed(11)
        Wf, lf = R.train_chain_f32(Xs, ys, W0, *K.saturated_args(B), chained)
        for j in range(4):
            assert np.array_equal(Wf[j], Wr[j].astype(np.float32)), (case, chained, j)
        j = K.ALL_WON_CLIENT
        # (float64 keeps the losers' exp(-200): residues far below fp32's reach)
        assert np.array_equal(Wf[j], Wf[j - 1] if chained else W0) and lf[j] == 0.0 and lr_[j] <= 1e-30


@pytest.mark.parametrize('case', K.MIXED_CASES, ids=str)
def test_mixed_cases_are_well_conditioned(case):
    """Rows at -128 are present, every batch spans two 64-row blocks with tails of 1, 7 and B - 3
    rows, and the fp32 oracle stays within a quarter of the GPU test's bound (2e-5)."""
    D, C, B, lr, on = case
    Xs, ys, W0 = K.mixed_inputs(D, C, B)
    assert sorted(len(y) % B for y in ys) == [1, 7, B - 3, B - 3] and 64 < B <= 128
    z0 = np.concatenate(Xs).astype(np.float64) @ W0.astype(np.float64).T
    assert (z0.max(axis=1) <= -104.0).any()                  # a padded class slot's 0 would win these rows
    for chained in (False, True):
        torch.manual_seed(11)
        Wr, lr_, _ = R.train_chain_ref64(Xs, ys, W0, *K.mixed_args(B, lr, on), chained)
        torch.manual_seed(11)
        Wf, lf = R.train_chain_f32(Xs, ys, W0, *K.mixed_args(B, lr, on), chained)
        for j in range(len(Xs)):
            assert np.abs(Wf[j] - Wr[j]).max() <= R.QUARTER * R.TOL * max(1.0, np.abs(Wr[j]).max()), (case, chained, j)
            assert abs(lf[j] - lr_[j]) <= R.QUARTER * R.TOL * max(1.0, abs(lr_[j])), (case, chained, j)


# ---- the library's host side (no device needed) ----------------------------------------------------

@pytest.fixture(scope='module')
def L():
    from fedamw_amd import _lib
    return _lib


def plan(L, N, C, B, E, ld, max_en, chained=0, want=0):
    g, ws = ctypes.c_int(want), ctypes.c_int64(-1)
    rc = L.lib().fs_local_train_plan(N, C, B, E, ld, max_en, chained, 0, ctypes.byref(g), ctypes.byref(ws))
    return rc, g.value, ws.value


def test_batch_size_zero_still_fails(L):
    one = ctypes.c_void_p(256)            # never dereferenced: validation comes first
    rc = L.lib().fs_local_train(one, 64, one, one, one, None, 1, 2, 0, 1, 0.5, 0.0, 0, 0.0, 0, 0, one, one, one, 1,
                                None, 0, None)
    assert rc != 0 and 'batch_size' in L.lib().fs_last_error().decode()


@pytest.mark.parametrize('B', [65, 4096])
def test_plan_answers_wide_above_64(L, B):
    assert L.G_WIDE == 2048 and L.LT_KERNELS[8] == 'wide'
    for chained in (0, 1):
        rc, g, ws = plan(L, 100, 10, B, 2, 2048, 2 * 700, chained)
        assert rc == 0 and g == 1 | L.G_WIDE and ws >= 256, (rc, g, ws)


def test_plan_workspace_is_host_arithmetic(L):
    """min(N, 512) slots (chained: one) of ceil64(min(B, max_en / E)) rows of 16 or 32 floats, then
    the 256-byte error block: bounded in N, and no larger than the largest client needs."""
    def ws(N, C, B, max_n, chained=0, E=2):
        rc, g, w = plan(L, N, C, B, E, 2048, E * max_n, chained)
        assert rc == 0 and g == 1 | L.G_WIDE
        return w
    assert ws(100, 10, 256, 700) == 100 * 256 * 16 * 4 + 256
    assert ws(100, 10, 65, 700) == 100 * 128 * 16 * 4 + 256
    assert ws(100, 17, 65, 700) == 100 * 128 * 32 * 4 + 256
    assert ws(100, 10, 2 ** 31 - 1, 700) == ws(100, 10, 700, 700) == 100 * 704 * 16 * 4 + 256
    assert ws(100, 10, 256, 700, chained=1) == 256 * 16 * 4 + 256
    assert ws(10 ** 6, 10, 256, 700) == ws(512, 10, 256, 700) == 512 * 256 * 16 * 4 + 256
    assert ws(100, 10, 256, 700, E=0) == 256


def test_plan_honours_a_wide_request_at_32(L):
    rc, g, ws = plan(L, 100, 10, 32, 2, 2048, 2 * 50, want=1 | L.G_WIDE)
    assert rc == 0 and g == 1 | L.G_WIDE and ws == 100 * 64 * 16 * 4 + 256
    # ... and nothing else changes at B <= 64: a request of 1 is still answered 1, without a workspace
    assert plan(L, 100, 10, 64, 2, 2048, 2 * 50, want=1) == (0, 1, 0)

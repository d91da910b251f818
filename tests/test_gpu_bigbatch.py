"""Batch sizes above 64: the wide form of fs_local_train (csrc/local_train_wide.hip, ABI 21,
G = 1 | G_WIDE -- one workgroup per client, the batch walked in 64-row blocks with the weights held
fixed and one update per batch) against the CPU oracle, the single form, the float64 reference
of tests/softmax_reference.py and, through the drop-ins, the reference's golden vectors
(tests/golden/make_golden_bigbatch.py; train_loop, functions/tools.py:177-215 of the reference).

Bounds: kernel level 2e-5 on W and the loss (the project's kernel bound; on this grid the fp32
oracle sits at most 4.8e-7 from a float64 run of itself, under a quarter of it); drop-ins
W_RTOL / LOSS_RTOL / one test sample (tests/fixtures.py).  Every case asserts that the wide form ran.
"""
import numpy as np
import pytest
import torch

from oracle import fedsim_oracle as O
from tests import bigbatch_cases as K
from tests import softmax_reference as R
from tests.fixtures import LOSS_RTOL, P_RTOL
from tests.softmax_reference import train_problem, train_ref64  # noqa: F401 (the exact-arithmetic inputs and reference)
from tests.test_bigbatch_oracle import ROUND_CASES, check_rounds, load_case, positional, split_clients
from tests.test_gpu_parity import _dl, _rand_clients, _train_via_abi, amd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 2e-5
SIZES = [1, 64, 65, 130, 257, 700]       # a 1-row client, exact and off-by-one blocks, tails of 1, 2 and 65 rows
E = 2


def _wide(amd, Xs, ys, W0, args, chained, seed=11, request=False):
    """One launch; ``request``: ask for the wide form (B <= 64), else the planner must choose it."""
    L = amd.lib
    W, loss = _train_via_abi(amd, Xs, ys, W0, *args, chained, seed=seed, split=(1 | L.G_WIDE) if request else None)
    assert L.lib().fs_local_train_last_kernel() == 8 and L.LT_KERNELS[8] == 'wide'      # FS_LT_WIDE
    assert _train_via_abi.last_G == 1 | L.G_WIDE
    return W, loss


_PROBLEMS = {}


def _problem(D, C):
    """The grid's clients and start, and per (B, terms) the oracle's result: computed once, shared."""
    if (D, C) not in _PROBLEMS:
        rs = np.random.RandomState(1000 * C + D)
        Xs, ys = _rand_clients(rs, SIZES, D, C)
        W0 = (rs.normal(size=(C, D)) * 0.1).astype(F32)
        _PROBLEMS[(D, C)] = (Xs, ys, W0, {})
    return _PROBLEMS[(D, C)]


def _oracle(D, C, args, chained, seed=11):
    Xs, ys, W0, memo = _problem(D, C)
    key = (args, chained, seed)
    if key not in memo:
        torch.manual_seed(seed)
        memo[key] = R.train_chain_f32(Xs, ys, W0, *args, chained)
    return memo[key]


def _terms(on):
    return (on, 0.05, on, 0.002)


def _check_vs_oracle(W, loss, Wr, lr_, what):
    for j in range(len(Wr)):
        eW = np.abs(W[j] - Wr[j]).max() / max(1.0, np.abs(Wr[j]).max())
        el = abs(loss[j] - lr_[j]) / max(1.0, abs(lr_[j]))
        assert eW <= TOL and el <= TOL, (what, j, eW, el)


@pytest.mark.parametrize('chained', [False, True], ids=['parallel', 'chained'])
@pytest.mark.parametrize('on', [False, True], ids=['none', 'prox+ridge'])
@pytest.mark.parametrize('B', [65, 96, 200, 256, 1024])
@pytest.mark.parametrize('D,C', [(64, 2), (200, 10), (1024, 16), (130, 26)])
def test_wide_vs_oracle(amd, D, C, B, on, chained):
    """Every client against O.train_client at 2e-5: clients below and above B, one and two class
    tiles, ld of 1, 4, 16 and 3 column tiles (waves without a tile; two tiles per wave); B = 1024
    on the 700-row client is a batch of two staged chunks."""
    Xs, ys, W0, _ = _problem(D, C)
    args = (0.5, E, B) + _terms(on)
    W, loss = _wide(amd, Xs, ys, W0, args, chained)
    Wr, lr_ = _oracle(D, C, args, chained)
    _check_vs_oracle(W, loss, Wr, lr_, (D, C, B, on, chained))


@pytest.mark.parametrize('D,C,B,sizes', [(8192, 10, 96, [97, 200, 1]), (4000, 17, 96, [97, 200, 1]),
                                         (2112, 10, 65, SIZES), (2112, 10, 200, SIZES), (1100, 26, 1024, SIZES)])
def test_wide_two_pass_vs_oracle(amd, D, C, B, sizes):
    """The grid above runs the one-pass instances (a wave holds the gradient of all its tiles: at
    most 4 tiles per wave at C <= 16, 2 above).  Wider rows take the two-pass instances, g through
    the workspace slot: D = 8192 (16 tiles per wave: four tile groups, weights in global memory),
    two class tiles at D = 4000 (global) and D = 1100 (3 tiles per wave; a 700-row batch spans two
    staged chunks), D = 2112 (5 tiles per wave, weights in LDS)."""
    rs = np.random.RandomState(D + C)
    Xs, ys = _rand_clients(rs, sizes, D, C)
    W0 = (rs.normal(size=(C, D)) * 0.1).astype(F32)
    for chained in (False, True):
        args = (0.5, E, B) + _terms(True)
        W, loss = _wide(amd, Xs, ys, W0, args, chained)
        torch.manual_seed(11)
        Wr, lr_ = R.train_chain_f32(Xs, ys, W0, *args, chained)
        _check_vs_oracle(W, loss, Wr, lr_, (D, C, chained))


@pytest.mark.parametrize('chained', [False, True], ids=['parallel', 'chained'])
@pytest.mark.parametrize('B', [16, 32, 33, 64])
def test_wide_on_request_matches_single(amd, B, chained):
    """The wide form where the single form also runs (a request of 1 | G_WIDE): the same inputs
    through both, within 2e-5 (one block per batch: the same sums in the same order, so in
    practice they agree far closer; the bound is the project's kernel bound)."""
    D, C = 200, 10
    Xs, ys, W0, _ = _problem(D, C)
    args = (0.5, E, B) + _terms(True)
    W, loss = _wide(amd, Xs, ys, W0, args, chained, request=True)
    Ws, ls = _train_via_abi(amd, Xs, ys, W0, *args, chained, seed=11, split=1)
    assert amd.lib.lib().fs_local_train_last_kernel() == 1
    _check_vs_oracle(W, loss, Ws, ls, (B, chained))


def test_effective_batch_and_repeatability(amd):
    """B = 700, 10^6 and 2^31 - 1 on clients of at most 700 rows train the same full batches:
    bitwise the same W and loss; two launches of one case are bitwise equal."""
    D, C = 200, 10
    Xs, ys, W0, _ = _problem(D, C)
    out = [_wide(amd, Xs, ys, W0, (0.5, E, B) + _terms(True), False) for B in (700, 10 ** 6, 2 ** 31 - 1, 700)]
    for W, loss in out[1:]:
        assert np.array_equal(W, out[0][0]) and np.array_equal(loss, out[0][1])
    Wr, lr_ = _oracle(D, C, (0.5, E, 700) + _terms(True), False)
    _check_vs_oracle(out[0][0], out[0][1], Wr, lr_, 'full batch')
    a = _wide(amd, Xs, ys, W0, (0.5, E, 96) + _terms(True), True)
    b = _wide(amd, Xs, ys, W0, (0.5, E, 96) + _terms(True), True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('case', K.SAT_CASES, ids=str)
def test_saturated_bitwise(amd, case):
    """Clients of exactly one batch of 128 or 256 saturated rows, lr = 2^-6: W bitwise the float64
    reference rounded to fp32, the loss within 2e-5; the 'all_won' client returns its start
    bitwise with loss 0.0 (the lead conditions: tests/test_bigbatch_oracle.py proves them, and they
    are asserted here as tests/test_gpu_softmax.py does)."""
    D, C, B = case
    Xs, ys, W0 = K.saturated_inputs(D, C, B)
    args = K.saturated_args(B)
    for chained in (False, True):
        W, loss = _wide(amd, Xs, ys, W0, args, chained)
        torch.manual_seed(11)
        Wr, lr_, gap = R.train_chain_ref64(Xs, ys, W0, *args, chained)
        assert gap >= R.GAP_EXACT
        for j in range(len(Xs)):
            assert np.array_equal(W[j], Wr[j].astype(F32)), (chained, j, np.abs(W[j] - Wr[j]).max())
            assert abs(loss[j] - lr_[j]) <= R.TOL * max(1.0, abs(lr_[j])), (chained, j, loss[j], lr_[j])
        j = K.ALL_WON_CLIENT
        assert np.array_equal(W[j], W[j - 1] if chained else W0) and loss[j] == 0.0
        assert not np.array_equal(W[j + 1], W[j] if chained else W0)        # ... and the next one moves


@pytest.mark.parametrize('case', K.MIXED_CASES, ids=str)
def test_mixed_rows_vs_float64(amd, case):
    """Saturated, tied and plain rows at offsets down to -128 (a padded class entering the maximum
    as 0 would underflow those rows) over batches of two 64-row blocks with ragged tails: within
    2e-5 of the float64 reference, everything finite."""
    D, C, B, lr, on = case
    Xs, ys, W0 = K.mixed_inputs(D, C, B)
    args = K.mixed_args(B, lr, on)
    for chained in (False, True):
        W, loss = _wide(amd, Xs, ys, W0, args, chained)
        assert np.isfinite(W).all() and np.isfinite(loss).all()
        torch.manual_seed(11)
        Wr, lr_, _ = R.train_chain_ref64(Xs, ys, W0, *args, chained)
        _check_vs_oracle(W, loss, Wr, lr_, (case, chained))


def test_more_workgroups_than_cus(amd):
    """300 parallel clients of 70 rows at B = 65 (a 65-row and a 5-row step per epoch): more
    workgroups than CUs; a sample of clients against the oracle, every client trained."""
    rs = np.random.RandomState(300)
    D, C, B, N = 128, 6, 65, 300
    Xs, ys = _rand_clients(rs, [70] * N, D, C)
    W0 = (rs.normal(size=(C, D)) * 0.1).astype(F32)
    args = (0.5, E, B) + _terms(False)
    W, loss = _wide(amd, Xs, ys, W0, args, False, seed=9)
    assert all(not np.array_equal(W[j], W0) for j in range(N)) and (loss > 0).all()
    torch.manual_seed(9)
    for j in range(N):
        if j % 37 == 0 or j == N - 1:
            Wr, lref = O.train_client(Xs[j], ys[j], W0, *args)
            assert np.abs(W[j] - Wr).max() <= TOL * max(1.0, np.abs(Wr).max()), j
            assert abs(loss[j] - lref) <= TOL * max(1.0, abs(lref)), j
        else:
            torch.empty(2 * E, dtype=torch.int64).random_()     # the oracle's draws for client j


def test_persistent_grid_walks(amd):
    """More clients than the grid's 512 workgroups: the workgroups walk d_order; the clients past
    the first 512 (in LPT order: the smallest) against the oracle."""
    rs = np.random.RandomState(600)
    D, C, B = 64, 3, 70
    sizes = [int(v) for v in rs.randint(1, 9, size=600)]
    sizes[5], sizes[599] = 150, 71
    Xs, ys = _rand_clients(rs, sizes, D, C)
    W0 = (rs.normal(size=(C, D)) * 0.1).astype(F32)
    args = (0.5, E, B) + _terms(True)
    W, loss = _wide(amd, Xs, ys, W0, args, False, seed=5)
    torch.manual_seed(5)
    Wr, lr_ = R.train_chain_f32(Xs, ys, W0, *args, False)
    _check_vs_oracle(W, loss, Wr, lr_, 'walk')


def test_chain_of_40_clients(amd):
    rs = np.random.RandomState(40)
    D, C, B = 128, 6, 100
    sizes = [int(v) for v in rs.randint(60, 160, size=40)]
    Xs, ys = _rand_clients(rs, sizes, D, C)
    W0 = (rs.normal(size=(C, D)) * 0.1).astype(F32)
    args = (0.2, E, B) + _terms(True)
    W, loss = _wide(amd, Xs, ys, W0, args, True, seed=4)
    torch.manual_seed(4)
    Wr, lr_ = R.train_chain_f32(Xs, ys, W0, *args, True)
    _check_vs_oracle(W, loss, Wr, lr_, 'chain')


# ---- the drop-ins, through the round plan (options['defer_eval'] is on by default) -------------------

def _tensors(d):
    Xs, ys = split_clients(d)
    return ([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys], torch.from_numpy(d['X_test']),
            torch.from_numpy(d['y_test']))


def _run_round_case(amd, d, stats):
    assert amd.tools.OPTIONS['defer_eval'] is True
    Xs, ys, Xt, yt = _tensors(d)
    mode = 'parallel' if str(d['mode']) == 'par' else 'sequential'
    torch.manual_seed(int(d['torch_seed']))
    if str(d['algo']) == 'fedamw':
        return amd.tools.FedAMW(Xs, ys, Xt, yt, _dl(d['X_val'], d['y_val'], int(d['Bv'])), *positional(d),
                                float(d['lr_p']), clients=mode, stats=stats, verbose=False)
    fn = amd.tools.FedAvg if str(d['algo']) == 'fedavg' else amd.tools.FedProx
    return fn(Xs, ys, Xt, yt, *positional(d), clients=mode, stats=stats, verbose=False)


@pytest.mark.parametrize('name', ROUND_CASES)
def test_dropin_rounds_match_reference(amd, name):
    """(These are the tests that fail without the feature: the parent raises NotImplementedError.)"""
    d = load_case(name)
    stats = {'trace': True}
    tr, tl, ta = _run_round_case(amd, d, stats)
    assert amd.lib.lib().fs_local_train_last_kernel() == 8
    ref = dict(d)
    p_ref = ref.pop('p', None)            # (the round plan keeps the last round's p only)
    check_rounds(name, ref, tr.numpy(), tl.numpy(), ta.numpy(), stats['W_rounds'])
    if p_ref is not None:
        assert np.abs(stats['p'].cpu().numpy() - p_ref[-1]).max() <= P_RTOL * np.abs(p_ref).max()
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), d['rng_after'])


def test_dropin_centralized_256_matches_reference(amd):
    d = load_case('bb_central_256')
    Xs, ys, Xt, yt = _tensors(d)
    stats = {'trace': True}
    torch.manual_seed(int(d['torch_seed']))
    tr, tl, ta = amd.tools.Centralized(Xs, ys, Xt, yt, *positional(d, rounds=False), stats=stats, verbose=False)
    assert amd.lib.lib().fs_local_train_last_kernel() == 8
    check_rounds('bb_central_256', d, tr, tl, ta, stats['W_global'].cpu().numpy()[None])
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), d['rng_after'])


def test_dropin_eval_stats_at_batch_100(amd):
    """stats['local_eval'] and stats['client_eval'] at batch_size = 100: the returns are bitwise
    those of the run without the keys, and the global model's loss on every client's own rows
    is the float64 cross-entropy of that round's model within LOSS_RTOL."""
    d = load_case('bb_fedavg_par')
    plain = {'trace': True}
    ref = _run_round_case(amd, d, plain)
    stats = {'trace': True, 'local_eval': ('global', 'own'), 'client_eval': 'test'}
    out = _run_round_case(amd, d, stats)
    assert amd.lib.lib().fs_local_train_last_kernel() == 8
    for a, b in zip(out, ref):
        assert torch.equal(a, b)
    assert np.array_equal(stats['W_rounds'], plain['W_rounds'])
    Rn, N = int(d['R']), len(d['sizes'])
    for key in ('local_global_loss', 'local_global_acc', 'local_own_loss', 'local_own_acc', 'client_test_loss',
                'client_test_acc'):
        assert tuple(stats[key].shape) == (Rn, N) and bool(torch.isfinite(stats[key]).all()), key
    Xs, ys = split_clients(d)
    for t in range(Rn):
        W = stats['W_rounds'][t].astype(np.float64)
        for j in range(N):
            z = Xs[j].astype(np.float64) @ W.T
            m = z.max(axis=1, keepdims=True)
            lse = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]
            ce = float((lse - z[np.arange(len(z)), ys[j]]).mean())
            assert abs(float(stats['local_global_loss'][t, j]) - ce) <= LOSS_RTOL * max(1.0, abs(ce)), (t, j)
            acc = 100.0 * float((z.argmax(axis=1) == ys[j]).mean())
            assert abs(float(stats['local_global_acc'][t, j]) - acc) <= 100.0 / len(z) + 1e-4, (t, j)


def test_regression_at_batch_65_still_raises(amd):
    X = [torch.rand(70, 8)]
    y = [torch.rand(70, 1)]
    with pytest.raises(NotImplementedError, match='regression'):
        amd.tools.FedAvg(X, y, torch.rand(9, 8), torch.rand(9, 1), 'regression', 1, 8, 0.1, 1, 65, False, 0.0, False, 0.0,
                         1, verbose=False)


def test_validation_batch_65_still_fails(amd):
    """The validation loader's batch keeps its limit of 64 (fs_mix_solve), whatever batch_size is."""
    d = load_case('bb_fedamw_par')
    Xs, ys, Xt, yt = _tensors(d)
    torch.manual_seed(1)
    with pytest.raises(amd.lib.FedsimError, match='valid batch size'):
        amd.tools.FedAMW(Xs, ys, Xt, yt, _dl(d['X_val'], d['y_val'], 65), *positional(d), float(d['lr_p']),
                         clients='parallel', verbose=False)

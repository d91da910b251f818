"""Partial client participation, host side (no GPU): the schedule maker, and the three
``part_*.npz`` reference fixtures held to the composition of the CPU oracle's functions."""
import numpy as np
import pytest
import torch

from oracle import fedsim_oracle as O
from tests.fixtures import LOSS_RTOL, W_RTOL, acc_tol, load, split_clients

PART_CASES = ['part_fedavg', 'part_fedprox_reg', 'part_fedavg_one']


@pytest.fixture(scope='module')
def P():
    import fedamw_amd  # noqa: F401
    from fedamw_amd.functions import participation
    return participation


def _stream(N, M, R, seed):
    """Item 8 of the semantics: one randperm per round on a private generator, sorted first M."""
    g = torch.Generator()
    g.manual_seed(seed)
    return [np.sort(torch.randperm(N, generator=g)[:M].numpy()) for _ in range(R)]


def test_schedule_is_the_randperm_stream_and_deterministic(P):
    a = P.make_schedule(25, 6, 0.3, 7)
    b = P.make_schedule(25, 6, 0.3, 7)
    ref = _stream(25, 8, 6, 7)
    assert len(a) == 6
    for x, y, r in zip(a, b, ref):
        assert x.dtype == np.int64 and np.array_equal(x, y) and np.array_equal(x, r)
        assert np.all(np.diff(x) > 0)
    assert any(not np.array_equal(x, y) for x, y in zip(a, P.make_schedule(25, 6, 0.3, 8)))
    c = P.make_schedule(25, 6, 8, 7)                 # an int is M itself
    assert all(np.array_equal(x, y) for x, y in zip(a, c))


@pytest.mark.parametrize('N,part,M', [(25, 0.1, 3), (10, 0.3, 3), (100, 0.29, 29), (3, 0.01, 1)])
def test_schedule_sample_size_rule(P, N, part, M):
    assert P.sample_size(N, part) == M
    assert all(len(S) == M for S in P.make_schedule(N, 3, part, 0))


def test_schedule_full_participation_is_every_client(P):
    for S in P.make_schedule(7, 3, 1.0, 5):
        assert np.array_equal(S, np.arange(7))


def test_schedule_leaves_the_global_generator_alone(P):
    torch.manual_seed(3)
    before = torch.get_rng_state().clone()
    P.make_schedule(50, 10, 0.2, 11)
    P.make_schedule(5, 2, [[0, 1], [4]], 11)
    assert torch.equal(torch.get_rng_state(), before)


def test_explicit_schedule_is_validated_and_sorted(P):
    s = P.make_schedule(6, 2, [[5, 0, 3], np.array([2])])
    assert np.array_equal(s[0], [0, 3, 5]) and np.array_equal(s[1], [2]) and s[0].dtype == np.int64
    for bad in ([[0, 6], [1]],          # out of range
                [[0, -1], [1]],
                [[0, 0], [1]],          # duplicate
                [[0, 1], []],           # empty round
                [[0, 1]],               # wrong R
                [[0, 1], [1], [2]]):
        with pytest.raises(ValueError):
            P.make_schedule(6, 2, bad)
    for bad in (0.0, 1.5, -0.1, 0, 7):
        with pytest.raises(ValueError):
            P.make_schedule(6, 2, bad)


def _oracle_run(d):
    """The round loop over the sampled clients as a composition of the oracle's functions."""
    Xs, ys = split_clients(d)
    C, D, R, E, B = int(d['C']), int(d['D']), int(d['R']), int(d['epoch']), int(d['batch_size'])
    lr = float(d['lr'])
    prox, mu, reg, lam = bool(d['prox']), float(d['mu']), bool(d['reg']), float(d['lam'])
    n = np.array([len(y) for y in ys])
    Wg = O.mlp_init(D, C)
    tr, tl, ta, Wt = [], [], [], []
    for t in range(R):
        lr = O.lr_schedule(t, lr, R)
        S = d['sched'][t]
        p = (n[S] / sum(n[S])).astype(np.float32)
        Ws, ls = [], []
        for i in S:
            W, l = O.train_client(Xs[i], ys[i], Wg, lr, E, B, prox, mu, reg, lam)
            Ws.append(W)
            ls.append(l)
        tr.append(np.sum(p * np.asarray(ls, np.float32), dtype=np.float32))
        Wg = O.aggregate(Ws, p)
        Wt.append(Wg.copy())
        a, b = O.test_eval(d['X_test'], d['y_test'], Wg, B)
        tl.append(a)
        ta.append(b)
    return np.array(tr), np.array(tl), np.array(ta), np.stack(Wt)


@pytest.mark.parametrize('name', PART_CASES)
def test_fixture_matches_the_oracle_composition(P, name):
    d = load(name)
    R, N = int(d['R']), len(d['sizes'])
    assert d['sched'].shape == (R, int(d['M']))
    for S, ref in zip(d['sched'], P.make_schedule(N, R, int(d['M']), int(d['sample_seed']))):
        assert np.array_equal(S, ref)
    torch.manual_seed(int(d['torch_seed']))
    tr, tl, ta, W = _oracle_run(d)
    rng_after = torch.empty(4, dtype=torch.int64).random_().numpy()
    assert W.shape == d['W'].shape
    for t in range(R):
        err = np.abs(W[t] - d['W'][t]).max()
        assert err <= W_RTOL * np.abs(d['W'][t]).max(), (name, t, err)
    np.testing.assert_allclose(tr, d['train_loss'], rtol=0, atol=LOSS_RTOL * max(1, np.abs(d['train_loss']).max()))
    np.testing.assert_allclose(tl, d['test_loss'], rtol=0, atol=LOSS_RTOL * max(1, np.abs(d['test_loss']).max()))
    assert np.abs(ta - d['test_acc']).max() <= acc_tol(d)
    np.testing.assert_array_equal(rng_after, d['rng_after'])

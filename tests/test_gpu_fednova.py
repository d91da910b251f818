"""FedNova on the GPU at drop-in level: ``tools.FedNova`` against the reference's own FedNova on
the four ``nova_*`` fixtures (bounds of fednova_drift.json), both variants with parallel clients and
under participation against the numpy restatement (tests/fednova_restatement.py; W within
2e-5 max|W|, losses within 1e-5 max(1, |l|): the kernel-level bounds of test_gpu_mse.py), and the
round plan's setting: mode 0 restores the plain aggregate bitwise, a deferred evaluation rides
across a nova AGGREGATE, mode 2 is refused on a chained plan."""
import numpy as np
import pytest
import torch

from tests import fednova_restatement as FR
from tests.fednova_fixtures import CASES, check_against, load, positional, split_clients

pytestmark = pytest.mark.gpu

W_TOL, LOSS_TOL = 2e-5, 1e-5


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine, rng
    from fedamw_amd.functions import participation, tools
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, rng=rng, tools=tools, participation=participation,
                                dev=torch.device('cuda')))


def _dropin(amd, d, **kw):
    Xs, ys = split_clients(d)
    Xs = [torch.from_numpy(x) for x in Xs]
    ys = [torch.from_numpy(y) for y in ys]
    stats = {'trace': True}
    torch.manual_seed(int(d['torch_seed']))
    out = amd.tools.FedNova(Xs, ys, torch.from_numpy(d['X_test']), torch.from_numpy(d['y_test']), *positional(d),
                            stats=stats, verbose=False, **kw)
    rng_after = torch.empty(4, dtype=torch.int64).random_().numpy()
    return [o.numpy() for o in out], stats, rng_after


@pytest.mark.parametrize('name', CASES)
def test_dropin_matches_the_references_fednova(amd, name):
    """The reference's call (chained clients, the reference form): W per round, the three returns,
    the final model and where the global generator is left."""
    d = load(name)
    (tr, tl, ta), stats, rng_after = _dropin(amd, d)
    check_against(name, d, tr, tl, ta, stats['W_rounds'])
    assert np.array_equal(stats['W_global'].cpu().numpy(), stats['W_rounds'][-1])
    np.testing.assert_array_equal(rng_after, d['rng_after'])


@pytest.fixture(scope='module')
def restated():
    """The restatement's runs, computed once per (case, variant, schedule)."""
    memo = {}

    def get(name, variant, sched=None):
        key = (name, variant, None if sched is None else tuple(tuple(int(j) for j in S) for S in sched))
        if key not in memo:
            tr, tl, ta, trace = FR.run_case(load(name), clients='parallel', variant=variant, sched=sched)
            memo[key] = (tr, tl, ta, trace['W'], torch.empty(4, dtype=torch.int64).random_().numpy())
        return memo[key]
    return get


def _check_restated(name, d, got, stats, rng_after, ref):
    tr, tl, ta = got
    check_against(name, d, tr, tl, ta, stats['W_rounds'], ref=ref[:4], rtol_W=W_TOL, rtol_loss=LOSS_TOL)
    np.testing.assert_array_equal(rng_after, ref[4])


@pytest.mark.parametrize('variant', ['reference', 'updates'])
@pytest.mark.parametrize('name', CASES)
def test_parallel_clients_match_the_restatement(amd, restated, name, variant):
    d = load(name)
    got, stats, rng_after = _dropin(amd, d, clients='parallel', variant=variant)
    _check_restated(name, d, got, stats, rng_after, restated(name, variant))


@pytest.mark.parametrize('variant', ['reference', 'updates'])
@pytest.mark.parametrize('name', ['nova_ce_ridge', 'nova_mse'])
def test_participation_matches_the_restatement(amd, restated, name, variant):
    """M = 3 sampled clients per round over R = 3 rounds (nova_ce_ridge: N = 6): the coefficients
    are taken over each round's sample in ascending id; only the sampled clients draw shuffles."""
    d = load(name)
    sched = amd.participation.make_schedule(len(d['sizes']), int(d['R']), 3, 3)
    assert all(len(S) == 3 for S in sched) and len({tuple(S) for S in sched}) > 1
    got, stats, rng_after = _dropin(amd, d, clients='parallel', variant=variant, participation=[S.copy() for S in sched])
    _check_restated(name, d, got, stats, rng_after, restated(name, variant, sched))
    assert all(np.array_equal(a, b) for a, b in zip(stats['participants'], sched))


def test_updates_differ_from_the_reference_form_and_from_fedavg(amd):
    """The three rules are three different models on unequal clients (none silently falls back)."""
    d = load('nova_ce')
    Wr = _dropin(amd, d, clients='parallel', variant='reference')[1]['W_rounds']
    Wu = _dropin(amd, d, clients='parallel', variant='updates')[1]['W_rounds']
    Xs, ys = split_clients(d)
    stats = {'trace': True}
    torch.manual_seed(int(d['torch_seed']))
    amd.tools.FedAvg([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys],
                     torch.from_numpy(d['X_test']), torch.from_numpy(d['y_test']), *positional(d), clients='parallel',
                     stats=stats, verbose=False)
    Wa = stats['W_rounds']
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()   # noqa: E731
    assert rel(Wr[0], Wa[0]) > 1e-2 and rel(Wu[0], Wa[0]) > 1e-3 and rel(Wr[0], Wu[0]) > 1e-2


# ---------------------------------------------------------------------------------------------
# plan level

def _clients(seed, N, D, C, lo=8, hi=40):
    rs = np.random.RandomState(seed)
    sizes = rs.randint(lo, hi + 1, size=N)
    Xs = [torch.from_numpy((np.cos(rs.normal(size=(n, D))) / np.sqrt(D)).astype(np.float32)) for n in sizes]
    ys = [torch.from_numpy(rs.randint(0, C, size=n).astype(np.int64)) for n in sizes]
    return Xs, ys


def _fed(amd, algo, clients, N=6, D=64, C=4, R=2, seed=31, **kw):
    Xs, ys = _clients(seed, N, D, C)
    Xt, yt = _clients(seed + 1, 1, D, C, lo=30, hi=30)
    torch.manual_seed(17)
    return amd.tools.Federation(algo, Xs, ys, Xt[0], yt[0], None, 'classification', C, D, 0.5, 2, 32, False, 0.0, False,
                                0.0, R, 1e-3, clients, verbose=False, **kw)


def test_mode_zero_restores_the_plain_aggregate(amd):
    """A FedAvg plan that ran one nova round, then fs_plan_set_nova(0): its next round, from the
    same round-start model, is bitwise the round of a plan that never had the setting."""
    opts = {'defer_eval': False, 'shuffle_chunk': 1}
    plain = _fed(amd, 'fedavg', 'parallel', options=opts)        # (each run seeds the generator: same shuffles)
    plain.round()
    W0 = plain.W_g.clone()
    plain.round()
    nova = _fed(amd, 'fedavg', 'parallel', options=opts)
    nova.plan.set_nova(amd.lib.NOVA_UPDATES)
    nova.round()
    torch.cuda.synchronize()
    assert not torch.equal(W0, nova.W_g)                         # (the nova round was a nova round:
    assert torch.equal(plain.loss_hist[0], nova.loss_hist[0])    #  same training, another aggregate)
    nova.plan.set_nova(0)
    nova.W_g.copy_(W0)
    nova.round()
    torch.cuda.synchronize()
    assert torch.isfinite(plain.W_g).all()
    assert torch.equal(plain.W_g, nova.W_g)
    assert torch.equal(plain.loss_hist[1], nova.loss_hist[1]) and torch.equal(plain.eval_hist[1], nova.eval_hist[1])


@pytest.mark.parametrize('variant', ['reference', 'updates'])
def test_deferred_evaluation_rides_across_a_nova_aggregate(amd, variant):
    """The split form at N = 10 leaves CUs idle: round t's evaluation fuses into round t+1's TRAIN
    launch and its finaliser rides on the nova aggregate.  Same models bitwise, the same
    eval_hist to the 1e-12 relative the header states for deferral."""
    tune = dict(train_form=1, split_mb=-1, split_dbuf=-1, split_pipe=-1, split_teams=-1)
    C, N, R, D, n_t = 10, 10, 3, 1024, 16 * 16 + 5
    Xs, ys = _clients(17, N, D, C)
    Xt, yt = _clients(18, 1, D, C, lo=n_t, hi=n_t)
    runs = {}
    with amd.lib.tuning(**tune):
        for defer in (False, True):
            stats = {'trace': True}
            torch.manual_seed(11)
            fed = amd.tools.Federation('fednova', Xs, ys, Xt[0], yt[0], None, 'classification', C, D, 0.5, 1, 32, False,
                                       0.0, False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False,
                                       options={'defer_eval': defer}, variant=variant)
            for _ in range(R):
                fed.round()
            fed.results()
            assert fed.plan.eval_blocks() > 0
            runs[defer] = (stats['W_rounds'], fed.eval_hist.cpu().numpy().copy())
    assert np.array_equal(runs[False][0], runs[True][0])
    assert np.isfinite(runs[True][1]).all()
    np.testing.assert_allclose(runs[True][1], runs[False][1], rtol=1e-12, atol=0)


def test_plan_setting_rejections(amd):
    U = amd.lib.FedsimError
    chained = _fed(amd, 'fedavg', 'sequential')
    with pytest.raises(U, match=r'\(-1\)'):                       # FS_EINVAL: mode 2 on a chained plan
        chained.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(U, match=r'\(-1\)'):                       # mode 1 without d_b
        chained.plan.set_nova(amd.lib.NOVA_REFERENCE)
    with pytest.raises(U, match=r'\(-1\)'):
        chained.plan.set_nova(3)
    b = torch.ones(6, device=amd.dev)
    chained.plan.set_nova(amd.lib.NOVA_REFERENCE, b, 1.0, 1.0)    # allowed: the reference chains its clients
    chained.plan.set_nova(0)
    with pytest.raises(ValueError, match='parallel'):
        _fed(amd, 'fednova', 'sequential', variant='updates')
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the experiment driver

def test_experiment_appends_fednova_only_when_asked(amd, tmp_path):
    """--algos ...,FedNova: a seventh row after the six default ones (exp.py:124's arguments, the
    reference form); the FedAvg row is that of a run without it (FedNova runs after the six, so it
    cannot move their draws)."""
    from fedamw_amd import experiment
    kw = dict(D=64, num_partitions=4, local_epoch=1, Round=3, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), save=False, synth=dict(n_train=700, n_test=120), verbose=False)
    six = experiment.run('a9a', algos=('FedAvg',), **kw)
    out = experiment.run('a9a', algos=('FedAvg', 'FedNova'), **kw)
    assert six['name'] == experiment.NAMES and six['test_acc'].shape == (6, 3, 1)
    assert out['name'] == experiment.NAMES + ['FedNova']
    for k in ('train_loss', 'test_loss', 'test_acc'):
        assert out[k].shape == (7, 3, 1) and np.isfinite(out[k][[3, 6]]).all() and np.isnan(out[k][[0, 1, 2, 4, 5]]).all()
        assert np.array_equal(out[k][3], six[k][3])
    assert not np.array_equal(out['test_loss'][6], out['test_loss'][3])
    with pytest.raises(ValueError, match='unknown algorithm'):
        experiment.run('a9a', algos=('FedAvg', 'FedNovaa'), **kw)

"""Partial client participation on the GPU: the gathered fold (fs_aggregate_sel), subset launches
of every training form, the FedAvg / FedProx drop-ins against the reference's ``part_*``
fixtures, full-participation equivalence, the deferred evaluation, stats, errors, regression.

Tolerances are tests/fixtures.py's (W_RTOL, LOSS_RTOL, acc_tol); everything else is bitwise."""
import numpy as np
import pytest
import torch

from oracle import fedsim_oracle as O
from tests.fixtures import LOSS_RTOL, W_RTOL, acc_tol, load, positional, split_clients

pytestmark = pytest.mark.gpu

PART_CASES = ['part_fedavg', 'part_fedprox_reg', 'part_fedavg_one']
SENTINEL = -7.25


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine, rng
    from fedamw_amd.functions import participation, tools
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, rng=rng, tools=tools, participation=participation,
                                dev=torch.device('cuda')))


# ---------------------------------------------------------------------------------------------
# (a) fs_aggregate_sel == fs_aggregate on the gathered copy, bitwise

def _agg_case(amd, N, M, length, chunks, seed):
    rs = np.random.RandomState(seed)
    sel = np.sort(rs.permutation(N)[:M]).astype(np.int32)
    W = np.full((N, length), np.nan, np.float32)          # rows outside sel: NaN, never to be read
    W[sel] = rs.normal(size=(M, length)).astype(np.float32)
    q = rs.rand(M).astype(np.float32)
    q /= q.sum()
    dev = amd.dev
    Wd, seld, qd = torch.from_numpy(W).to(dev), torch.from_numpy(sel).to(dev), torch.from_numpy(q).to(dev)
    agg = amd.engine.Aggregator(M, 1, length, dev, chunks=chunks)
    ref = agg.run(Wd[seld.long()].contiguous(), qd, torch.empty(length, device=dev)).cpu().numpy()
    got = agg.run_sel(Wd, seld, qd, torch.full((length,), np.nan, device=dev)).cpu().numpy()
    return W, sel, q, ref, got


@pytest.mark.parametrize('M', [1, 3, 15, 16, 40])
def test_aggregate_sel_one_launch_forms(amd, M):
    """len = 3 * 64, N = 40: one sub-range (M < 16: the reference's exact left fold) and several."""
    W, sel, q, ref, got = _agg_case(amd, 40, M, 3 * 64, 0, 100 + M)
    assert np.isfinite(got).all()
    assert np.array_equal(got, ref)
    if M < 16:
        assert np.array_equal(got, O.aggregate([W[j] for j in sel], q))


@pytest.mark.parametrize('chunks', [0, 1, 4])
def test_aggregate_sel_chunked_forms(amd, chunks):
    """M = 600 of N = 700, above the one-launch form's 512 clients: chunks plus the stage-2 fold."""
    W, sel, q, ref, got = _agg_case(amd, 700, 600, 64, chunks, 7 + chunks)
    assert np.isfinite(got).all()
    assert np.array_equal(got, ref)
    if chunks == 1:
        assert np.array_equal(got, O.aggregate([W[j] for j in sel], q))


def test_aggregate_sel_rejects_bad_arguments(amd):
    dev = amd.dev
    agg = amd.engine.Aggregator(4, 1, 64, dev)
    W = torch.zeros(4, 64, device=dev)
    q = torch.ones(2, device=dev)
    with pytest.raises(ValueError):
        agg.run_sel(W, torch.tensor([0, 4], dtype=torch.int32, device=dev), q, torch.empty(64, device=dev))
    with pytest.raises(ValueError):
        agg.run_sel(W, torch.tensor([0, 1], dtype=torch.int64, device=dev), q, torch.empty(64, device=dev))
    L = amd.lib.lib()
    assert L.fs_aggregate_sel(None, 64, None, None, 0, 64, None, None, 0, 1, None) == -1
    assert 'M' in L.fs_last_error().decode()


# ---------------------------------------------------------------------------------------------
# (b) every training form trains a subset in place

def _forms(amd):
    L = amd.lib
    off = dict(train_form=1, split_mb=-1, split_dbuf=-1, split_pipe=-1, split_teams=-1)
    return {
        # form: (fs_tuning, D = ld, trainer.G, FS_LT_*)
        'split': (off, 1024, 2, 2),
        'mb': (dict(off, split_mb=1), 1024, 2, 7),
        'dbuf': (dict(off, split_dbuf=1), 2048, 2, 3),
        'pair': (dict(off, train_form=2), 1024, 2 | L.G_PAIR, 4),
        'pipe': (dict(off, train_form=0, split_pipe=1), 2048, 2 | L.G_PIPE, 5),
        'teams': (dict(off, split_teams=1), 2048, 4 | L.G_TEAMS, 6),
    }


def _clients(seed, N, D, C, lo=8, hi=40, float_targets=False):
    rs = np.random.RandomState(seed)
    sizes = rs.randint(lo, hi + 1, size=N)
    Xs = [torch.from_numpy((np.cos(rs.normal(size=(n, D))) / np.sqrt(D)).astype(np.float32)) for n in sizes]
    if float_targets:
        ys = [torch.from_numpy(rs.normal(size=(n, 1)).astype(np.float32)) for n in sizes]
    else:
        ys = [torch.from_numpy(rs.randint(0, C, size=n).astype(np.int64)) for n in sizes]
    return Xs, ys


def _subset_safety(amd, D, C, B, E, G, kernel, loss='ce', seed=5, prox=True):
    """Train all 10 clients, then sel = {0, 3, 4, 9} and {7} into sentinel-filled buffers: the
    sampled rows and losses are bitwise the full launch's, everything else keeps the sentinel."""
    N = 10
    Xs, ys = _clients(seed, N, D, C, float_targets=loss == 'mse')
    feats = amd.engine.Features(Xs, ys, D, amd.dev, float_targets=loss == 'mse')
    tr = amd.engine.LocalTrainer(feats, C, B, E, prox=prox, loss=loss)
    if G is not None:
        assert tr.G == G, (tr.G, G)
    torch.manual_seed(3)
    tr.upload_perms(amd.rng.draw_pass_seeds(N * E))
    W0 = torch.zeros(C, feats.ld, device=amd.dev)
    W0[:, :D] = torch.from_numpy(O.mlp_init(D, C)).to(amd.dev)
    args = (W0, 0.3, prox, 0.01, prox, 0.001, False)      # (prox and ridge terms together, or neither)
    last = amd.lib.lib().fs_local_train_last_kernel
    W_full, l_full = tr.run(*args)
    if kernel is not None:
        assert last() == kernel
    W_full, l_full = W_full.clone(), l_full.clone()
    assert torch.isfinite(W_full).all() and torch.isfinite(l_full).all()
    for sel in ([0, 3, 4, 9], [7]):
        tr.W_out.fill_(SENTINEL)
        lo = torch.full((N,), SENTINEL, dtype=torch.float64, device=amd.dev)
        W_sub, l_sub = tr.run(*args, loss_out=lo, sel=sel)
        if kernel is not None:
            assert last() == kernel
        tr.check_errors()
        rest = [j for j in range(N) if j not in sel]
        assert torch.equal(W_sub[sel], W_full[sel]), sel
        assert torch.equal(l_sub[sel], l_full[sel]), sel
        assert bool((W_sub[rest] == SENTINEL).all()) and bool((l_sub[rest] == SENTINEL).all()), sel


@pytest.mark.parametrize('form', ['split', 'mb', 'dbuf', 'pair', 'pipe', 'teams'])
def test_subset_launch_per_exchanging_form(amd, form):
    """The six rows of test_gpu_eval's form table, plain FedAvg steps as there (the double-buffered
    instance is not chosen with a prox term)."""
    tune, D, G, kernel = _forms(amd)[form]
    with amd.lib.tuning(**tune):
        _subset_safety(amd, D, 10, 32, 2, G, kernel, prox=False)


def test_subset_launch_split_form_with_prox_and_ridge(amd):
    tune, D, G, kernel = _forms(amd)['split']
    with amd.lib.tuning(**tune):
        _subset_safety(amd, D, 10, 32, 2, G, kernel, prox=True)


def test_subset_launch_single_form(amd):
    _subset_safety(amd, 64, 10, 32, 2, 1, 1)


def test_subset_launch_wide_form(amd):
    _subset_safety(amd, 96, 10, 100, 2, 1 | amd.lib.G_WIDE, 8)


def test_subset_launch_mse(amd):
    _subset_safety(amd, 200, 1, 32, 2, None, None, loss='mse')


def test_subset_launch_validates_sel(amd):
    Xs, ys = _clients(1, 4, 64, 3)
    tr = amd.engine.LocalTrainer(amd.engine.Features(Xs, ys, 64, amd.dev), 3, 32, 1)
    for bad in ([], [0, 0], [4], [-1], [0, 1, 2, 3, 3]):
        with pytest.raises(ValueError):
            tr.sel_order(bad)
    assert tr.sel_order([3, 1]).dtype == np.int32


# ---------------------------------------------------------------------------------------------
# (c) the drop-ins against the reference's fixtures

def _dropin(amd, d, **kw):
    Xs, ys = split_clients(d)
    Xs = [torch.from_numpy(x) for x in Xs]
    ys = [torch.from_numpy(y) for y in ys]
    stats = {'trace': True}
    stats.update(kw.pop('stats', {}))
    torch.manual_seed(int(d['torch_seed']))
    fn = amd.tools.FedAvg if str(d['algo']) == 'fedavg' else amd.tools.FedProx
    out = fn(Xs, ys, torch.from_numpy(d['X_test']), torch.from_numpy(d['y_test']), *positional(d), clients='parallel',
             stats=stats, verbose=False, **kw)
    rng_after = torch.empty(4, dtype=torch.int64).random_().numpy()
    return out, stats, rng_after


def _check_against_fixture(d, out, stats, rng_after):
    tr, tl, ta = out
    W, Wref = stats['W_rounds'], d['W']
    assert W.shape == Wref.shape
    for t in range(len(Wref)):
        err = np.abs(W[t] - Wref[t]).max()
        print('round %d: max|W - W_ref| / max|W_ref| = %.2e' % (t, err / np.abs(Wref[t]).max()))
        assert err <= W_RTOL * np.abs(Wref[t]).max(), (t, err)
    np.testing.assert_allclose(tr.numpy(), d['train_loss'], rtol=0,
                               atol=LOSS_RTOL * max(1, np.abs(d['train_loss']).max()))
    np.testing.assert_allclose(tl.numpy(), d['test_loss'], rtol=0,
                               atol=LOSS_RTOL * max(1, np.abs(d['test_loss']).max()))
    assert np.abs(ta.numpy() - d['test_acc']).max() <= acc_tol(d)
    np.testing.assert_array_equal(rng_after, d['rng_after'])
    assert len(stats['participants']) == len(d['sched'])
    for S, ref in zip(stats['participants'], d['sched']):
        assert S.dtype == np.int64 and np.array_equal(S, ref)


@pytest.mark.parametrize('how', ['schedule', 'sampler'])
@pytest.mark.parametrize('name', PART_CASES)
def test_dropin_matches_reference_participation(amd, name, how):
    """An explicit schedule and the (M, sample_seed) sampler both reproduce the reference loop
    over the sampled clients: W per round, the three returns, where the generator is left."""
    d = load(name)
    kw = (dict(participation=list(d['sched'])) if how == 'schedule'
          else dict(participation=int(d['M']), sample_seed=int(d['sample_seed'])))
    out, stats, rng_after = _dropin(amd, d, **kw)
    _check_against_fixture(d, out, stats, rng_after)
    if name == 'part_fedavg_one':
        assert amd.lib.lib().fs_local_train_last_kernel() == 8          # the wide form (B = 100)


# ---------------------------------------------------------------------------------------------
# (d) full participation through the subset path == the path without the keyword

@pytest.mark.parametrize('how', ['fraction', 'schedule'])
def test_full_participation_is_bitwise_the_default_path(amd, how):
    d = load('fedprox_par')
    N, R = len(d['sizes']), int(d['R'])
    part = 1.0 if how == 'fraction' else [np.arange(N)] * R
    (tr0, tl0, ta0), s0, rng0 = _dropin(amd, d)
    (tr1, tl1, ta1), s1, rng1 = _dropin(amd, d, participation=part)
    assert 'participants' not in s0 and all(np.array_equal(S, np.arange(N)) for S in s1['participants'])
    assert np.array_equal(s0['W_rounds'], s1['W_rounds'])
    assert torch.equal(tr0, tr1) and torch.equal(tl0, tl1) and torch.equal(ta0, ta1)
    assert np.array_equal(rng0, rng1)


# ---------------------------------------------------------------------------------------------
# (e) the deferred evaluation rides on subset launches

def test_deferred_eval_under_participation(amd):
    tune, D, G, kernel = _forms(amd)['split']
    C, N, R, n_t = 10, 10, 3, 16 * 16 + 5
    Xs, ys = _clients(17, N, D, C)
    Xt, yt = _clients(18, 1, D, C, lo=n_t, hi=n_t)
    sched = amd.participation.make_schedule(N, R, 4, 3)
    runs = {}
    with amd.lib.tuning(**tune):
        for defer in (False, True):
            stats = {'trace': True}
            torch.manual_seed(11)
            fed = amd.tools.Federation('fedavg', Xs, ys, Xt[0], yt[0], None, 'classification', C, D, 0.5, 1, 32, False,
                                       0.0, False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False,
                                       options={'defer_eval': defer}, participation=sched)
            kernels = []
            for _ in range(R):
                fed.round()
                kernels.append(int(amd.lib.lib().fs_local_train_last_kernel()))
            fed.results()
            assert fed.trainer.G == G and kernels == [kernel] * R
            assert fed.plan.eval_blocks() > 0
            runs[defer] = (stats['W_rounds'], fed.eval_hist.cpu().numpy().copy())
    assert np.array_equal(runs[False][0], runs[True][0])
    assert np.isfinite(runs[True][1]).all()
    np.testing.assert_allclose(runs[True][1], runs[False][1], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------
# (f) stats of unsampled clients

def test_stats_of_unsampled_clients_are_nan(amd):
    """Round 0 of two runs whose round-0 samples share clients 0 and 1 (first in the draw order
    of both, so on the same shuffles and from the same W): their own-model and per-client rows
    agree bitwise; unsampled rows are NaN; local_global_* covers all N."""
    N, D, C, R = 6, 64, 4, 2
    Xs, ys = _clients(23, N, D, C)
    Xt, yt = _clients(24, 1, D, C, lo=50, hi=50)
    res = {}
    for key, sched in (('a', [[0, 1, 4], [2, 3]]), ('b', [[0, 1, 5], [0, 4]])):
        stats = {'local_eval': ('global', 'own'), 'client_eval': 'test'}
        torch.manual_seed(5)
        amd.tools.FedAvg(Xs, ys, Xt[0], yt[0], 'classification', C, D, 0.5, 2, 32, False, 0.0, False, 0.0, R,
                         clients='parallel', stats=stats, verbose=False, participation=sched)
        own = ('local_own_loss', 'local_own_acc', 'client_test_loss', 'client_test_acc')
        for t, S in enumerate(sched):
            rest = [j for j in range(N) if j not in S]
            for k in own:
                assert stats[k].shape == (R, N)
                assert bool(torch.isnan(stats[k][t, rest]).all()) and bool(torch.isfinite(stats[k][t, S]).all()), (k, t)
        for k in ('local_global_loss', 'local_global_acc', 'global_objective'):
            assert bool(torch.isfinite(stats[k]).all()), k
        res[key] = stats
    for k in own:
        assert torch.equal(res['a'][k][0, [0, 1]], res['b'][k][0, [0, 1]]), k


# ---------------------------------------------------------------------------------------------
# (g) errors

def _small_fed(amd, clients, R=4, **kw):
    Xs, ys = _clients(31, 5, 64, 3)
    Xt, yt = _clients(32, 1, 64, 3, lo=20, hi=20)
    return amd.tools.Federation('fedavg', Xs, ys, Xt[0], yt[0], None, 'classification', 3, 64, 0.5, 1, 32, False, 0.0,
                                False, 0.0, R, 1e-3, clients, verbose=False, **kw)


def _subset_args(amd, ids):
    dev = amd.dev
    sel = torch.tensor(ids, dtype=torch.int32, device=dev)
    return sel, sel.clone(), torch.full((len(ids),), 1.0 / len(ids), device=dev)


def test_participation_errors(amd):
    Xs, ys = _clients(31, 5, 64, 3)
    Xt, yt = _clients(32, 1, 64, 3, lo=20, hi=20)
    a = (Xs, ys, Xt[0], yt[0], 'classification', 3, 64, 0.5, 1, 32, False, 0.0, False, 0.0, 2)
    with pytest.raises(ValueError, match="clients='parallel'"):
        amd.tools.FedAvg(*a, clients='sequential', verbose=False, participation=0.5)
    with pytest.raises(ValueError, match="clients='parallel'"):
        amd.tools.FedProx(*a, verbose=False, participation=2)
    with pytest.raises(ValueError):
        amd.tools.FedAvg(*a, clients='parallel', verbose=False, participation=[[0, 9], [1]])
    vl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(Xt[0], yt[0]), batch_size=16, shuffle=True)
    with pytest.raises(TypeError):
        amd.tools.FedAMW(Xs, ys, Xt[0], yt[0], vl, 'classification', 3, 64, 0.5, 1, 32, False, 0.0, True, 0.01, 2, 1e-3,
                         clients='parallel', verbose=False, participation=0.5)


def test_plan_subset_rejections(amd):
    T, U = amd.lib.PHASE_TRAIN, amd.lib.FedsimError
    sel, order, q = _subset_args(amd, [0, 2])
    seeds = np.arange(2, dtype=np.int64)
    chained = _small_fed(amd, 'sequential')
    with pytest.raises(U, match=r'\(-3\)'):                       # FS_EUNSUPPORTED
        chained.plan.round_subset(0, 0.5, T, sel, order, q)
    with pytest.raises(U, match=r'\(-3\)'):
        chained.plan.shuffle_subset(seeds, [0, 2], 0)
    fed = _small_fed(amd, 'parallel', options={'shuffle_chunk': 1})
    for M in (0, 6):                                              # M = 0, M = N + 1
        big = _subset_args(amd, list(range(6)))
        with pytest.raises(U, match=r'\(-1\)'):
            fed.plan.round_subset(0, 0.5, T, *big, M=M)
    L = amd.lib.lib()
    ids = np.arange(6, dtype=np.int32)
    for M in (0, 6):
        assert L.fs_plan_shuffle_subset(fed.plan._h, np.zeros(6, np.int64).ctypes.data, ids.ctypes.data, M, 0) == -1
    bad = np.array([2, 0], np.int32)                              # not ascending
    assert L.fs_plan_shuffle_subset(fed.plan._h, seeds.ctypes.data, bad.ctypes.data, 2, 0) == -1
    assert L.fs_plan_round_subset(fed.plan._h, 0, 0.5, T, None, None, None, 2, None) == -1
    with pytest.raises(U, match=r'\(-1\)'):                       # round 0 was never prepared
        fed.plan.round_subset(0, 0.5, T, sel, order, q)
    fed.plan.shuffle(amd.rng.draw_pass_seeds(5), 0)               # prepared for all N: not for this sample
    with pytest.raises(U, match=r'\(-1\)'):
        fed.plan.round_subset(0, 0.5, T, sel, order, q)
    chunked = _small_fed(amd, 'parallel', options={'shuffle_chunk': 1})
    chunked.plan.set_chunk(4)
    with pytest.raises(U, match=r'\(-1\)'):                       # FS_EINVAL: per-round slots only
        chunked.plan.round_subset(0, 0.5, T, sel, order, q)
    with pytest.raises(U, match=r'\(-1\)'):
        chunked.plan.shuffle_subset(seeds, [0, 2], 0)
    torch.cuda.synchronize()


def test_subset_rounds_after_the_chunk_was_set_and_reset(amd):
    """fs_plan_set_shuffle_chunk(4) then (1), both before the first shuffle, reallocate the
    pinned seed slots: they must still hold a subset round's [3][P] layout (seeds and the pass
    table).  The run is bitwise the run of a plan whose chunk was never touched."""
    N, D, C, R = 40, 64, 4, 3
    Xs, ys = _clients(51, N, D, C)
    Xt, yt = _clients(52, 1, D, C, lo=30, hi=30)
    sched = amd.participation.make_schedule(N, R, 30, 2)
    Ws = []
    for reset in (False, True):
        stats = {'trace': True}
        torch.manual_seed(13)
        fed = amd.tools.Federation('fedavg', Xs, ys, Xt[0], yt[0], None, 'classification', C, D, 0.5, 2, 32, False, 0.0,
                                   False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False, participation=sched)
        if reset:
            fed.plan.set_chunk(4)
            fed.plan.set_chunk(1)
        for _ in range(R):
            fed.round()
        fed.results()
        Ws.append((stats['W_rounds'], fed.loss_hist.cpu().numpy()))
    assert np.isfinite(Ws[0][0]).all()
    assert np.array_equal(Ws[0][0], Ws[1][0])
    assert np.array_equal(Ws[0][1], Ws[1][1], equal_nan=True)


# ---------------------------------------------------------------------------------------------
# (h) the regression task, and the host shuffle replay

def _regression(amd, **kw):
    N, D, R = 5, 200, 3
    Xs, ys = _clients(41, N, D, 1, float_targets=True)
    Xt, yt = _clients(42, 1, D, 1, lo=30, hi=30, float_targets=True)
    stats = {'trace': True}
    torch.manual_seed(9)
    out = amd.tools.FedAvg(Xs, ys, Xt[0], yt[0], 'regression', 1, D, 0.2, 2, 32, False, 0.0, False, 0.0, R,
                           clients='parallel', stats=stats, verbose=False, **kw)
    return out, stats, torch.empty(4, dtype=torch.int64).random_().numpy()


def test_regression_under_participation(amd):
    N, R = 5, 3
    (tr0, tl0, ta0), s0, rng0 = _regression(amd)
    (tr1, tl1, ta1), s1, rng1 = _regression(amd, participation=[np.arange(N)] * R)
    assert np.array_equal(s0['W_rounds'], s1['W_rounds']) and np.array_equal(rng0, rng1)
    assert torch.equal(tr0, tr1) and torch.equal(tl0, tl1) and torch.equal(ta0, ta1)
    sched = [[1, 3], [0, 4], [1, 2]]
    Xs, ys = _clients(41, N, 200, 1, float_targets=True)
    Xt, yt = _clients(42, 1, 200, 1, lo=30, hi=30, float_targets=True)
    torch.manual_seed(9)
    fed = amd.tools.Federation('fedavg', Xs, ys, Xt[0], yt[0], None, 'regression', 1, 200, 0.2, 2, 32, False, 0.0,
                               False, 0.0, R, 1e-3, 'parallel', stats={'trace': True}, verbose=False,
                               participation=sched)
    for _ in range(R):
        fed.round()
    tr, tl, ta = fed.results()
    lh = fed.loss_hist.cpu().numpy()
    for t, S in enumerate(sched):
        rest = [j for j in range(N) if j not in S]
        assert np.isnan(lh[t, rest]).all() and np.isfinite(lh[t, S]).all()
    assert torch.isfinite(tr).all() and torch.isfinite(tl).all()
    W = fed.stats['W_rounds']
    assert np.isfinite(W).all() and not np.array_equal(W[0], s0['W_rounds'][0])


def test_host_shuffle_replay_matches_device_replay(amd):
    """shuffle_device=False: the host pool replays the sampled passes only; same bits."""
    d = load('part_fedavg')
    Xs, ys = split_clients(d)
    Xs, ys = [torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys]
    Ws = []
    for device in (True, False):
        stats = {'trace': True}
        torch.manual_seed(int(d['torch_seed']))
        fed = amd.tools.Federation(str(d['algo']), Xs, ys, torch.from_numpy(d['X_test']), torch.from_numpy(d['y_test']),
                                   None, *positional(d), 1e-3, 'parallel', stats=stats, verbose=False,
                                   shuffle_device=device, participation=list(d['sched']))
        for _ in range(fed.R):
            fed.round()
        fed.results()
        Ws.append(stats['W_rounds'])
    assert np.array_equal(Ws[0], Ws[1])

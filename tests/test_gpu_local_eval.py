"""Local evaluation at the engine and round level: engine.LocalEvaluator (fs_eval_clients) and
``stats['local_eval']`` through Federation, Distributed, FedAMW_OneShot and experiment.run.  Every
entry of the histories is held BITWISE to the existing single-model evaluation (engine.Evaluator:
fs_eval / fs_eval_mse) of the same model on the client's own rows -- contract A of
include/fedsim.h -- so no tolerance appears here; the kernel's own error against float64 is
bounded in tests/test_gpu_eval_clients.py."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.local_eval_reference import objective
from tests.test_gpu_dist import _free_port
from tests.test_gpu_parity import amd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

# eight ragged clients of 5 to 70 rows; D = 100 so ld = 128
SIZES, D, C, E, B, R, N_T, N_VAL, BV = (5, 70, 13, 22, 31, 16, 47, 9), 100, 3, 2, 8, 3, 33, 17, 4
N = len(SIZES)
LR, LR_P, MU, LAM = 0.5, 0.05, 0.02, 1e-3
SEED = 23
BOTH = ('global', 'own')


def _features(rs, n):
    return (rs.normal(size=(n, D)) / np.sqrt(D)).astype(np.float32)


def _problem(regression=False):
    rs = np.random.RandomState(SEED)
    Xs = [_features(rs, n) for n in SIZES]
    Xt, Xv = _features(rs, N_T), _features(rs, N_VAL)
    if regression:
        w = rs.normal(size=D)

        def tgt(X):
            y = (X @ w + 0.1 * rs.normal(size=len(X))).astype(np.float32).reshape(-1, 1)
            y[::4] = 0.0            # the degenerate accuracy counts exact zeros
            return y
    else:
        w = rs.normal(size=(D, C))

        def tgt(X):
            y = np.argmax(X @ w, axis=1)
            flip = rs.rand(len(X)) < 0.2
            y[flip] = rs.randint(0, C, size=int(flip.sum()))
            return y.astype(np.int64)
    return Xs, [tgt(X) for X in Xs], Xt, tgt(Xt), Xv, tgt(Xv)


def _loader(Xv, yv):
    T = torch.from_numpy
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(T(Xv), T(yv)), batch_size=BV, shuffle=True)


def _federation(tools, algo, clients, stats, regression=False, rounds=R):
    """(``defer_eval`` off, as tests/test_gpu_client_eval.py at this shape: B = 8 on ld = 128 leaves
    a parallel split launch no LDS room for the fused evaluation -- a scheduling option, no
    result bit depends on it.)"""
    Xs, ys, Xt, yt, Xv, yv = _problem(regression)
    T = torch.from_numpy
    torch.manual_seed(SEED)
    vl = _loader(Xv, yv) if algo == 'fedamw' else None
    return tools.Federation(algo, [T(x) for x in Xs], [T(y) for y in ys], T(Xt), T(yt), vl,
                            'regression' if regression else 'classification', 1 if regression else C, D,
                            0.05 if regression else LR, E, B, algo == 'fedprox', MU, algo == 'fedamw', LAM, rounds,
                            LR_P if algo == 'fedamw' else None, clients, stats=stats, verbose=False,
                            options={'defer_eval': False})


def _drive(tools, algo, clients, request, regression=False, rounds=R):
    """Run the rounds through Federation, cloning the clients x params buffer after every round.
    Returns (fed, stats, snapshots [R][n_mine, C, ld], results)."""
    stats = {'trace': True}
    if request is not None:
        stats['local_eval'] = request
    fed = _federation(tools, algo, clients, stats, regression, rounds)
    snaps = []
    for _ in range(rounds):
        fed.round()
        snaps.append(fed.trainer.W_out[:len(fed.mine)].clone())
    return fed, stats, snaps, fed.results()


class Slices:
    """One engine.Evaluator (fs_eval / fs_eval_mse) per client, on the client's own rows."""

    def __init__(self, engine, ld, regression=False):
        Xs, ys = _problem(regression)[:2]
        self.dev = torch.device('cuda')
        self.ld, self.Cc = ld, 1 if regression else C
        self.evs = [engine.Evaluator(torch.from_numpy(X), torch.from_numpy(y), D, self.Cc, self.dev, ld,
                                     loss='mse' if regression else 'ce') for X, y in zip(Xs, ys)]

    def pad(self, W):
        """numpy [..., D] -> device [..., ld]"""
        Wd = torch.zeros(W.shape[:-1] + (self.ld,), device=self.dev)
        Wd[..., :D] = torch.from_numpy(np.ascontiguousarray(W))
        return Wd

    def run(self, models):
        """models: device [C, ld] (one for every client) or [N, C, ld] -> numpy [N, 2]"""
        out = torch.empty(N, 2, dtype=torch.float64, device=self.dev)
        for j, ev in enumerate(self.evs):
            ev.run(models if models.dim() == 2 else models[j], out[j])
        return out.cpu().numpy()


def _hist(stats, which):
    return np.stack([stats['local_%s_loss' % which].numpy(), stats['local_%s_acc' % which].numpy()], axis=-1)


def _check_shapes(stats, rounds=R):
    for which in BOTH:
        for m in ('loss', 'acc'):
            v = stats['local_%s_%s' % (which, m)]
            assert v.shape == (rounds, N) and v.dtype == torch.float64 and not v.is_cuda, (which, m)
    g = stats['global_objective']
    assert g.shape == (rounds,) and g.dtype == torch.float64 and not g.is_cuda
    gl = stats['local_global_loss'].numpy()
    assert np.array_equal(g.numpy(), np.array([objective(gl[t], SIZES) for t in range(rounds)]))


@pytest.mark.parametrize('clients', ['parallel', 'sequential'])
@pytest.mark.parametrize('algo', ['fedavg', 'fedamw'])
def test_round_histories_are_fs_eval_on_the_slices(amd, algo, clients):
    """'global'[t]: fs_eval of W_rounds[t] (the model test_loss[t] scores) on each client's rows;
    'own'[t]: fs_eval of the W_out snapshot after round t's training.  Both bitwise."""
    fed, stats, snaps, out = _drive(amd.tools, algo, clients, BOTH)
    _check_shapes(stats)
    sl = Slices(amd.engine, fed.ld)
    gh, oh = _hist(stats, 'global'), _hist(stats, 'own')
    for t in range(R):
        assert np.array_equal(gh[t], sl.run(sl.pad(stats['W_rounds'][t]))), ('global', t)
        assert np.array_equal(oh[t], sl.run(snaps[t])), ('own', t)
    assert not np.array_equal(gh[0], gh[R - 1]) and not np.array_equal(oh[0], gh[0])
    # the last round's global model is W_global; it scores test_loss[R - 1] on the test rows
    assert np.array_equal(gh[R - 1], sl.run(sl.pad(stats['W_global'].cpu().numpy())))
    o2 = torch.empty(2, dtype=torch.float64, device=sl.dev)
    fed.evaluator.run(sl.pad(stats['W_rounds'][R - 1]), o2)
    assert np.float32(o2[0].item()) == out[1][R - 1].numpy()


def test_own_after_one_round(amd):
    """A one-round run: 'own' against fs_eval of the trainer's W_out as the run leaves it."""
    fed, stats, snaps, _ = _drive(amd.tools, 'fedavg', 'parallel', 'own', rounds=1)
    assert 'local_global_loss' not in stats and 'global_objective' not in stats
    assert stats['local_own_loss'].shape == (1, N)
    sl = Slices(amd.engine, fed.ld)
    assert np.array_equal(_hist(stats, 'own')[0], sl.run(fed.trainer.W_out[:N]))
    assert torch.equal(fed.trainer.W_out[:N], snaps[0])


@pytest.mark.parametrize('algo,clients', [('fedavg', 'parallel'), ('fedavg', 'sequential'), ('fedamw', 'parallel'),
                                          ('fedamw', 'sequential')])
def test_nothing_moves(amd, algo, clients):
    """With and without the key after a common reseed: the three returned tensors, W_global, the
    per-round models, p and the torch and numpy generator states afterwards are bitwise equal;
    without the key nothing is allocated."""
    runs = []
    for request in (None, BOTH):
        np.random.seed(SEED)
        fed, stats, _, out = _drive(amd.tools, algo, clients, request)
        runs.append((out, stats['W_global'].cpu(), stats['W_rounds'], stats['p'].cpu() if algo == 'fedamw' else None,
                     torch.get_rng_state(), np.random.get_state()))
        assert ('local_global_loss' in stats) == ('global_objective' in stats) == (request is not None)
        assert (fed.local_eval is not None) == bool(fed.local_hist) == (request is not None)
    (o0, W0, Wr0, p0, g0, n0), (o1, W1, Wr1, p1, g1, n1) = runs
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    assert torch.equal(W0, W1) and np.array_equal(Wr0, Wr1) and torch.equal(g0, g1)
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]
    if algo == 'fedamw':
        assert torch.equal(p0, p1)


def test_regression(amd):
    """type='regression' (C = 1) through FedAvg: bitwise fs_eval_mse on the slices."""
    fed, stats, snaps, _ = _drive(amd.tools, 'fedavg', 'parallel', BOTH, regression=True)
    _check_shapes(stats)
    sl = Slices(amd.engine, fed.ld, regression=True)
    gh, oh = _hist(stats, 'global'), _hist(stats, 'own')
    ys = _problem(True)[1]
    for t in range(R):
        assert np.array_equal(gh[t], sl.run(sl.pad(stats['W_rounds'][t]))), t
        assert np.array_equal(oh[t], sl.run(snaps[t])), t
        assert np.array_equal(gh[t, :, 1], [100.0 * float((y == 0).sum()) / len(y) for y in ys])
    assert (gh[:, :, 0] > 0).all()


def test_distributed_one_shot_and_centralized(amd):
    """Distributed: [N] and a 0-dim objective; FedAMW_OneShot: 'global' [R, N] against fs_eval of
    its W_rounds, 'own' [N]; both 'own' against the chained local models trained again from the
    same seed.  Centralized refuses the key: one pooled client."""
    tools, dev = amd.tools, torch.device('cuda')
    Xs, ys, Xt, yt, Xv, yv = _problem()
    T = torch.from_numpy
    args = ([T(x) for x in Xs], [T(y) for y in ys], T(Xt), T(yt))

    def chain(reg, lam):
        torch.manual_seed(SEED)
        W_init = tools.init_weights(D, C)
        _, trainer, W_out, _ = tools._chain_train(args[0], args[1], W_init, D, C, LR, 4, B, False, 0.0, reg, lam, dev)
        return trainer, W_out[:N]

    stats = {'local_eval': BOTH}
    torch.manual_seed(SEED)
    plain = tools.Distributed(*args, 'classification', C, D, LR, 4, B, False, 0.0, False, 0.0, stats=stats,
                              verbose=False)
    keep, W_out = chain(False, 0.0)
    sl = Slices(amd.engine, W_out.shape[2])
    for which in BOTH:
        assert stats['local_%s_loss' % which].shape == stats['local_%s_acc' % which].shape == (N,)
    assert np.array_equal(_hist(stats, 'own'), sl.run(W_out))
    assert np.array_equal(_hist(stats, 'global'), sl.run(sl.pad(stats['W_global'].cpu().numpy())))
    assert stats['global_objective'].shape == () and stats['global_objective'].dtype == torch.float64
    assert float(stats['global_objective']) == objective(stats['local_global_loss'].numpy(), SIZES)
    torch.manual_seed(SEED)
    again = tools.Distributed(*args, 'classification', C, D, LR, 4, B, False, 0.0, False, 0.0, verbose=False)
    assert float(plain[0]) == float(again[0]) and plain[1:] == again[1:]

    stats = {'local_eval': BOTH, 'trace': True}
    torch.manual_seed(SEED)
    tools.FedAMW_OneShot(*args, _loader(Xv, yv), 'classification', C, D, LR, 4, B, False, 0.0, True, LAM, 2, LR_P,
                         stats=stats, verbose=False)
    keep, W_out = chain(True, LAM)
    assert stats['local_global_loss'].shape == stats['local_global_acc'].shape == (2, N)
    assert stats['local_own_loss'].shape == stats['local_own_acc'].shape == (N,)
    assert stats['global_objective'].shape == (2,)
    gh = _hist(stats, 'global')
    for t in range(2):
        assert np.array_equal(gh[t], sl.run(sl.pad(stats['W_rounds'][t]))), t
        assert float(stats['global_objective'][t]) == objective(gh[t, :, 0], SIZES)
    assert np.array_equal(_hist(stats, 'own'), sl.run(W_out))

    with pytest.raises(ValueError, match='pooled'):
        tools.Centralized(*args, 'classification', C, D, LR, 4, B, False, 0.0, False, 0.0,
                          stats={'local_eval': 'global'}, verbose=False)


def test_request_errors(amd):
    with pytest.raises(ValueError, match='local_eval'):
        _federation(amd.tools, 'fedavg', 'parallel', {'local_eval': 'test'})
    with pytest.raises(ValueError, match='local_eval'):
        _federation(amd.tools, 'fedamw', 'sequential', {'local_eval': ('global', 'all')})
    Xs, ys, Xt, yt, _, _ = _problem()
    T = torch.from_numpy
    with pytest.raises(ValueError, match='local_eval'):
        amd.tools.Distributed([T(x) for x in Xs], [T(y) for y in ys], T(Xt), T(yt), 'classification', C, D, LR, 1, B,
                              stats={'local_eval': 'both'}, verbose=False)


def test_local_evaluator_argument_checks(amd):
    dev = torch.device('cuda')
    Xs, ys = _problem()[:2]
    f = amd.engine.Features([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys], D, dev)
    le = amd.engine.LocalEvaluator(f, C)
    assert le.N == N and le.ws.numel() == amd.lib.lib().fs_eval_clients_ws_doubles(sum(SIZES), N)
    out = torch.empty(N, 2, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match='W must'):
        le.run(torch.zeros(C, f.ld, device=dev), C * f.ld, out)             # one model, N asked for
    with pytest.raises(ValueError, match='out must'):
        le.run(torch.zeros(C, f.ld, device=dev), 0, out[:N - 1])
    with pytest.raises(ValueError, match='mse'):
        amd.engine.LocalEvaluator(f, 1, loss='mse')
    le.run(torch.zeros(C, f.ld, device=dev), 0, out)                        # all-zero model: log C, ties to class 0
    got = out.cpu().numpy()
    assert np.allclose(got[:, 0], np.log(C), rtol=1e-6)
    assert np.array_equal(got[:, 1], [100.0 * float((y == 0).sum()) / len(y) for y in ys])


def test_experiment_driver(tmp_path):
    """experiment.run(local_eval='both'): one list per metric, an entry per algorithm (None for
    CL); the reference's keys keep their shapes and values, and without the option no key is added."""
    import pickle

    from fedamw_amd import experiment
    kw = dict(D=64, num_partitions=4, local_epoch=1, Round=2, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), synth=dict(n_train=500, n_test=90), verbose=False)
    out = experiment.run('a9a', local_eval='both', **kw)
    with open(os.path.join(str(tmp_path), 'exp1_a9a.pkl'), 'rb') as f:
        saved = pickle.load(f)
    names = out['name']
    keys = ('local_global_loss', 'local_global_acc', 'local_own_loss', 'local_own_acc', 'global_objective')
    for key in keys:
        assert len(out[key]) == 6 and out[key][names.index('CL')] is None
        for name in ('FedAvg', 'FedProx', 'FedAMW', 'DL', 'FedAMW_OneShot'):
            v = out[key][names.index(name)]
            once = name == 'DL' or (name == 'FedAMW_OneShot' and 'own' in key)
            shape = (() if once else (2,)) if key == 'global_objective' else ((4,) if once else (2, 4))
            assert len(v) == 1 and v[0].shape == shape and v[0].dtype == np.float64, (key, name, v[0].shape)
            assert np.isfinite(v[0]).all()
            assert np.array_equal(saved[key][names.index(name)][0], v[0])
    assert out['test_loss'].shape == (6, 2, 1)
    plain = experiment.run('a9a', save=False, **kw)
    assert not [k for k in plain if k.startswith('local_') or k == 'global_objective']
    for k in ('train_loss', 'test_loss', 'test_acc'):                       # the same run with and without
        assert np.array_equal(plain[k], out[k], equal_nan=True), k
    with pytest.raises(ValueError, match='local_eval'):
        experiment.run('a9a', local_eval='all', **kw)


# --------------------------------------------------------------------------- #
# two ranks
# --------------------------------------------------------------------------- #
def _rank_run():
    from fedamw_amd.functions import tools
    fed, stats, snaps, _ = _drive(tools, 'fedavg', 'parallel', BOTH)
    res = {k: v.numpy() for k, v in stats.items() if k.startswith('local_') and k.endswith(('_loss', '_acc'))}
    res['global_objective'] = stats['global_objective'].numpy()
    return res, np.asarray(fed.mine), [s.cpu().numpy() for s in snaps], stats['W_rounds']


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    try:
        out[rank] = _rank_run()
    finally:
        torch.distributed.destroy_process_group()


def test_two_ranks(amd):
    """Two gloo ranks on the one GPU, parallel clients: each rank scores its own shard, and
    every rank returns the same [R, N] histories in the caller's client order.  Each entry equals
    BITWISE the single-process evaluation of the same model: 'global' fs_eval of that run's own
    W_rounds[t] (the sharded aggregate rounds differently from the single-process fold after round
    0, so the run's own models are the reference), 'own' fs_eval of the ranks' W_out snapshots put
    back in the caller's order."""
    mgr = mp.get_context('spawn').Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    (res0, mine0, snaps0, Wr0), (res1, mine1, snaps1, Wr1) = out[0], out[1]
    assert sorted(list(mine0) + list(mine1)) == list(range(N)) and len(mine0) and len(mine1)
    assert len(res0) == 5 and set(res0) == set(res1)
    for k in res0:
        assert res0[k].shape == ((R,) if k == 'global_objective' else (R, N)) and np.array_equal(res0[k], res1[k]), k
    assert np.array_equal(Wr0, Wr1)
    ld = snaps0[0].shape[2]
    sl = Slices(amd.engine, ld)
    for t in range(R):
        g = sl.run(sl.pad(Wr0[t]))
        assert np.array_equal(g[:, 0], res0['local_global_loss'][t]), t
        assert np.array_equal(g[:, 1], res0['local_global_acc'][t]), t
        assert res0['global_objective'][t] == objective(g[:, 0], SIZES)
        W = np.empty((N, C, ld), np.float32)
        W[mine0], W[mine1] = snaps0[t], snaps1[t]
        o = sl.run(torch.from_numpy(W).to(sl.dev))
        assert np.array_equal(o[:, 0], res0['local_own_loss'][t]), t
        assert np.array_equal(o[:, 1], res0['local_own_acc'][t]), t

"""Per-client evaluation at the engine and round level: engine.ClientEvaluator (fs_mix_z on row
chunks + fs_z_eval_*) and ``stats['client_eval']`` through Federation, Distributed and
FedAMW_OneShot, against the existing single-model evaluation (engine.Evaluator: fs_eval /
fs_eval_mse) on the same client models, and against the float64 reference of
tests/eval_reference.py.  Counts are compared exactly, losses within ``loss_bound`` (one kernel
against float64) or twice it (two kernels against each other)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.eval_reference import ce_acc_ref, dot_bound_rows, exact_problem, loss_bound
from tests.test_gpu_dist import _free_port
from tests.test_gpu_parity import amd  # noqa: F401 (fixture)
from tests.z_eval_reference import ZE_ROWS, ldn, mse_ref

pytestmark = pytest.mark.gpu

# the one small shape of every entry point: 5 ragged clients of 7 to 40 rows
SIZES, D, C, E, B, R, N_T, N_VAL, BV = (7, 40, 13, 22, 31), 100, 3, 2, 8, 3, 33, 17, 4
N = len(SIZES)
LR, LR_P, MU, LAM = 0.5, 0.05, 0.02, 1e-3
SEED = 21            # data and torch seed of the round-level tests


def _features(rs, n):
    return (rs.normal(size=(n, D)) / np.sqrt(D)).astype(np.float32)


def _problem(regression=False):
    """Unit-norm centred features; labels from a linear model with a fifth of them redrawn, so
    the trained models separate the classes and a row's top two logits are rarely close."""
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


def _federation(tools, algo, clients, stats, regression=False):
    """(``defer_eval`` off -- a scheduling option, no result bit depends on it: at this shape, B = 8
    on ld = 128, a parallel split launch has no LDS room for the fused evaluation and
    fs_plan_round refuses the deferred one, with or without client_eval.)"""
    Xs, ys, Xt, yt, Xv, yv = _problem(regression)
    T = torch.from_numpy
    torch.manual_seed(SEED)
    vl = _loader(Xv, yv) if algo == 'fedamw' else None
    return tools.Federation(algo, [T(x) for x in Xs], [T(y) for y in ys], T(Xt), T(yt), vl,
                            'regression' if regression else 'classification', 1 if regression else C, D,
                            0.05 if regression else LR, E, B, algo == 'fedprox', MU, algo == 'fedamw', LAM, R,
                            LR_P if algo == 'fedamw' else None, clients, stats=stats, verbose=False,
                            options={'defer_eval': False})


def _drive(tools, algo, clients, request, regression=False):
    """Run the R rounds through Federation, cloning the clients x params buffer after every
    round.  Returns (fed, stats, snapshots [R][n_mine, C, ld], results)."""
    stats = {} if request is None else {'client_eval': request}
    fed = _federation(tools, algo, clients, stats, regression)
    snaps = []
    for _ in range(R):
        fed.round()
        snaps.append(fed.trainer.W_out[:len(fed.mine)].clone())
    return fed, stats, snaps, fed.results()


def _each(ev, W_all):
    """engine.Evaluator.run on every model of W_all [N, C, ld] -> numpy [N, 2]."""
    out = torch.empty(W_all.shape[0], 2, dtype=torch.float64, device=W_all.device)
    for j in range(W_all.shape[0]):
        ev.run(W_all[j], out[j])
    return out.cpu().numpy()


def _check_against_evaluator(loss, acc, ev_res, X, y, W_all, tag):
    """Per-client (loss, acc %) against fs_eval's on the same models: counts exact -- rows whose
    top two float64 logits are closer than dot_bound_rows are dropped from the count comparison,
    at most 5 % of the rows -- and losses within twice loss_bound."""
    n = len(y)
    worst = 0.0
    for j in range(W_all.shape[0]):
        W = W_all[j, :, :X.shape[1]].cpu().numpy()
        ce, _, _ = ce_acc_ref(X, y, W)
        z = np.sort(X.astype(np.float64) @ W.astype(np.float64).T, axis=1)
        unsure = int((z[:, -1] - z[:, -2] < dot_bound_rows(X, W)).sum()) if z.shape[1] > 1 else 0
        assert unsure <= 0.05 * n, (tag, j, unsure)
        assert abs(round(acc[j] * n / 100.0) - round(ev_res[j, 1] * n / 100.0)) <= unsure, (tag, j)
        if unsure == 0:
            assert acc[j] == ev_res[j, 1], (tag, j, acc[j], ev_res[j, 1])
        frac = abs(loss[j] - ev_res[j, 0]) / (2.0 * loss_bound(z.shape[1], ce))
        worst = max(worst, frac)
        assert frac <= 1.0, (tag, j, loss[j], ev_res[j, 0], frac)
    print('%s: worst |dloss| / (2 loss_bound) = %.3f' % (tag, worst))


@pytest.mark.parametrize('D_', [27, 64, 100])
@pytest.mark.parametrize('C_', [3, 10])
def test_client_evaluator_on_exact_inputs(amd, D_, C_):
    """exact_problem with N * C class rows reshaped to [N, C, D]: logits exact in any summation
    order, so the GEMM's Z is the float64 Z.  Against ce_acc_ref per client: counts exact, loss
    within loss_bound; against fs_eval on each W_j: counts exact, loss within twice loss_bound;
    three chunks: bitwise the unchunked result."""
    n, dev = 33, torch.device('cuda')
    X, y, W, _ = exact_problem(np.random.RandomState(1000 * D_ + C_), n, D_, N * C_)
    y = y % C_
    W = W.reshape(N, C_, D_)
    ev = amd.engine.Evaluator(torch.from_numpy(X), torch.from_numpy(y), D_, C_, dev)
    Wd = torch.zeros(N, C_, ev.f.ld, device=dev)
    Wd[:, :, :D_] = torch.from_numpy(W)
    ce = amd.engine.ClientEvaluator(ev.f, C_, N)
    out = torch.full((N + 1, 2), -7.0, dtype=torch.float64, device=dev)
    ce.run(Wd, N, out)
    got = out.cpu().numpy()
    assert (got[N] == -7.0).all()
    ev_res = _each(ev, Wd)
    for j in range(N):
        rows, loss, correct = ce_acc_ref(X, y, W[j])
        assert got[j, 1] == 100.0 * correct / n == ev_res[j, 1], (j, got[j, 1], correct)
        b = loss_bound(C_, rows)
        assert abs(got[j, 0] - loss) <= b, (j, got[j, 0], loss, b)
        assert abs(got[j, 0] - ev_res[j, 0]) <= 2 * b, (j, got[j, 0], ev_res[j, 0], b)
    ce3 = amd.engine.ClientEvaluator(ev.f, C_, N, chunk_rows=ZE_ROWS)
    assert ce3.chunk_rows == ZE_ROWS and -(-n // ce3.chunk_rows) == 3
    out3 = torch.empty(N, 2, dtype=torch.float64, device=dev)
    ce3.run(Wd, N, out3)
    assert torch.equal(out3, out[:N])
    # fewer models than the evaluator was sized for: the same bits per model (column independence)
    out2 = torch.empty(2, 2, dtype=torch.float64, device=dev)
    ce.run(Wd[3:], 2, out2)
    assert torch.equal(out2, out[3:5])


def test_default_scratch_is_bounded(amd):
    """The scratch Z of ``run`` is capped at 256 MB by default, in whole row blocks."""
    dev = torch.device('cuda')
    n = 5000
    ev = amd.engine.Evaluator(torch.zeros(n, 64), torch.zeros(n, dtype=torch.int64), 64, 10, dev)
    ce = amd.engine.ClientEvaluator(ev.f, 10, 4000)
    assert ce.chunk_rows % ZE_ROWS == 0 and 0 < ce.chunk_rows < n
    assert 4 * ce.chunk_rows * 10 * 4000 <= 256 << 20 < 4 * (ce.chunk_rows + ZE_ROWS) * 10 * 4000
    assert ce.Z is None                                     # allocated by the first run
    small = amd.engine.ClientEvaluator(ev.f, 10, 5)
    assert small.chunk_rows == -(-n // ZE_ROWS) * ZE_ROWS


@pytest.mark.parametrize('clients', ['parallel', 'sequential'])
@pytest.mark.parametrize('algo', ['fedavg', 'fedprox', 'fedamw'])
def test_round_histories_match_the_evaluator(amd, algo, clients):
    """FedAvg / FedProx / FedAMW, parallel and chained: the [R, N] histories equal fs_eval on the
    snapshots of W_out taken after every round; FedAMW's 'val' history, from the p-solve's own Z,
    equals a ClientEvaluator on the validation rows bitwise."""
    request = ('test', 'val') if algo == 'fedamw' else 'test'
    fed, stats, snaps, _ = _drive(amd.tools, algo, clients, request)
    Xs, ys, Xt, yt, Xv, yv = _problem()
    tl, ta = stats['client_test_loss'], stats['client_test_acc']
    assert tl.shape == ta.shape == (R, N) and tl.dtype == ta.dtype == torch.float64 and not tl.is_cuda
    for t in range(R):
        _check_against_evaluator(tl[t].numpy(), ta[t].numpy(), _each(fed.evaluator, snaps[t]), Xt, yt, snaps[t],
                                 '%s %s test round %d' % (algo, clients, t))
    assert not torch.equal(tl[0], tl[R - 1])                # the models moved between the rounds
    if algo != 'fedamw':
        assert 'client_val_loss' not in stats
        return
    vl_, va = stats['client_val_loss'], stats['client_val_acc']
    assert vl_.shape == va.shape == (R, N)
    dev = snaps[0].device
    ev = amd.engine.Evaluator(torch.from_numpy(Xv), torch.from_numpy(yv), D, C, dev, fed.ld)
    ce = amd.engine.ClientEvaluator(fed.mixture.f, C, N)
    for t in range(R):
        out = torch.empty(N, 2, dtype=torch.float64, device=dev)
        ce.run(snaps[t], N, out)
        assert torch.equal(out[:, 0].cpu(), vl_[t]) and torch.equal(out[:, 1].cpu(), va[t]), t
        _check_against_evaluator(vl_[t].numpy(), va[t].numpy(), _each(ev, snaps[t]), Xv, yv, snaps[t],
                                 'fedamw %s val round %d' % (clients, t))


def _chain(tools, Xs, ys, epochs, reg, lam, dev):
    """The local models Distributed / FedAMW_OneShot train: their own first steps, replayed."""
    torch.manual_seed(SEED)
    W_init = tools.init_weights(D, C)
    T = torch.from_numpy
    _, trainer, W_out, _ = tools._chain_train([T(x) for x in Xs], [T(y) for y in ys], W_init, D, C, LR, epochs, B,
                                              False, 0.0, reg, lam, dev)
    return trainer, W_out[:N]


def test_distributed_and_one_shot(amd):
    """Distributed and FedAMW_OneShot return [N] tensors for their one set of local models:
    against fs_eval on those models (trained again from the same seed); FedAMW_OneShot's 'val'
    from its single Z equals a ClientEvaluator on the validation rows bitwise."""
    tools, dev = amd.tools, torch.device('cuda')
    Xs, ys, Xt, yt, Xv, yv = _problem()
    T = torch.from_numpy
    args = ([T(x) for x in Xs], [T(y) for y in ys], T(Xt), T(yt))
    stats = {'client_eval': 'test'}
    torch.manual_seed(SEED)
    tools.Distributed(*args, 'classification', C, D, LR, 4, B, False, 0.0, False, 0.0, stats=stats, verbose=False)
    keep, W_out = _chain(tools, Xs, ys, 4, False, 0.0, dev)
    ev = amd.engine.Evaluator(T(Xt), T(yt), D, C, dev, W_out.shape[2])
    assert stats['client_test_loss'].shape == stats['client_test_acc'].shape == (N,)
    _check_against_evaluator(stats['client_test_loss'].numpy(), stats['client_test_acc'].numpy(), _each(ev, W_out),
                             Xt, yt, W_out, 'Distributed')
    with pytest.raises(ValueError):
        tools.Distributed(*args, 'classification', C, D, LR, 4, B, False, 0.0, False, 0.0,
                          stats={'client_eval': 'val'}, verbose=False)

    stats = {'client_eval': ('test', 'val')}
    torch.manual_seed(SEED)
    tools.FedAMW_OneShot(*args, _loader(Xv, yv), 'classification', C, D, LR, 4, B, False, 0.0, True, LAM, 2, LR_P,
                         stats=stats, verbose=False)
    keep, W_out = _chain(tools, Xs, ys, 4, True, LAM, dev)
    _check_against_evaluator(stats['client_test_loss'].numpy(), stats['client_test_acc'].numpy(), _each(ev, W_out),
                             Xt, yt, W_out, 'FedAMW_OneShot test')
    evv = amd.engine.Evaluator(T(Xv), T(yv), D, C, dev, W_out.shape[2])
    _check_against_evaluator(stats['client_val_loss'].numpy(), stats['client_val_acc'].numpy(), _each(evv, W_out),
                             Xv, yv, W_out, 'FedAMW_OneShot val')
    out = torch.empty(N, 2, dtype=torch.float64, device=dev)
    amd.engine.ClientEvaluator(evv.f, C, N).run(W_out, N, out)
    assert torch.equal(out[:, 0].cpu(), stats['client_val_loss']) and torch.equal(out[:, 1].cpu(),
                                                                                  stats['client_val_acc'])


@pytest.mark.parametrize('algo', ['fedavg', 'fedamw'])
def test_regression_histories(amd, algo):
    """type='regression' ([n, 1] float targets, C = 1).  The last round against the float64
    reference from the SAME fp32 Z (the evaluator's scratch / the p-solve's Z) at the MSE bound
    2^-22 ref; every round against fs_eval_mse on the snapshots, where the two kernels' dot
    products differ by at most delta_v = dot_bound_rows per row, so the means by at most
    mean(2 |res_v| delta_v + delta_v^2) on top of the MSE bound; the accuracy value exact."""
    request = ('test', 'val') if algo == 'fedamw' else 'test'
    fed, stats, snaps, _ = _drive(amd.tools, algo, 'parallel', request, regression=True)
    Xs, ys, Xt, yt, Xv, yv = _problem(regression=True)
    sets = [('test', Xt, yt.reshape(-1), fed.client_eval['test'][0].Z)]
    if algo == 'fedamw':
        sets.append(('val', Xv, yv.reshape(-1), fed.mixture.Z))
    for which, X, y, Zdev in sets:
        loss, acc = stats['client_%s_loss' % which].numpy(), stats['client_%s_acc' % which].numpy()
        assert loss.shape == acc.shape == (R, N)
        n = len(y)
        Z = Zdev.reshape(-1)[:n * ldn(N)].reshape(n, ldn(N)).cpu().numpy()
        ref, racc = mse_ref(Z, y, N)
        assert (np.abs(loss[R - 1] - ref) <= 2.0 ** -22 * ref).all(), (which, loss[R - 1], ref)
        assert (acc == racc).all() and racc == 100.0 * float((y == 0).sum()) / n
        ev = fed.evaluator if which == 'test' else amd.engine.Evaluator(torch.from_numpy(X), torch.from_numpy(
            y.reshape(-1, 1)), D, 1, snaps[0].device, fed.ld, loss='mse')
        for t in range(R):
            res = _each(ev, snaps[t])
            for j in range(N):
                w = snaps[t][j, :, :D].cpu().numpy()
                delta = dot_bound_rows(X, w)
                r = np.abs(X.astype(np.float64) @ w[0].astype(np.float64) - y)
                tol = 2.0 ** -22 * res[j, 0] + float(np.mean(2.0 * r * delta + delta * delta))
                assert abs(loss[t, j] - res[j, 0]) <= tol, (which, t, j, loss[t, j], res[j, 0], tol)
                assert acc[t, j] == res[j, 1]


@pytest.mark.parametrize('algo,clients', [('fedavg', 'parallel'), ('fedamw', 'sequential')])
def test_nothing_moves(amd, algo, clients):
    """The same call with and without client_eval after a common reseed: the three returned
    tensors, W_global, p and the generator state afterwards are bitwise equal."""
    runs = []
    for request in (None, ('test', 'val') if algo == 'fedamw' else 'test'):
        fed, stats, _, out = _drive(amd.tools, algo, clients, request)
        runs.append((out, stats['W_global'].cpu(), stats['p'].cpu() if algo == 'fedamw' else None,
                     torch.get_rng_state()))
        assert ('client_test_loss' in stats) == (request is not None)
        assert bool(fed.client_eval) == (request is not None)
    (o0, W0, p0, g0), (o1, W1, p1, g1) = runs
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    assert torch.equal(W0, W1) and torch.equal(g0, g1)
    if algo == 'fedamw':
        assert torch.equal(p0, p1)


def test_request_errors(amd):
    with pytest.raises(ValueError, match='validloader'):
        _federation(amd.tools, 'fedavg', 'parallel', {'client_eval': 'val'})
    with pytest.raises(ValueError, match='client_eval'):
        _federation(amd.tools, 'fedavg', 'parallel', {'client_eval': 'train'})
    with pytest.raises(ValueError, match='client_eval'):
        _federation(amd.tools, 'fedamw', 'parallel', {'client_eval': ('test', 'all')})


def test_experiment_driver(tmp_path):
    """experiment.run(client_eval='both'): the results gain one list per metric, an entry per
    algorithm (None for CL; 'val' only where there is a validation set); the reference's keys
    keep their shapes, and without the option no key is added."""
    import pickle

    from fedamw_amd import experiment
    kw = dict(D=64, num_partitions=4, local_epoch=1, Round=2, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), synth=dict(n_train=500, n_test=90), verbose=False)
    out = experiment.run('a9a', client_eval='both', **kw)
    with open(os.path.join(str(tmp_path), 'exp1_a9a.pkl'), 'rb') as f:
        saved = pickle.load(f)
    names = out['name']
    for key in ('client_test_loss', 'client_test_acc', 'client_val_loss', 'client_val_acc'):
        assert len(out[key]) == 6 and out[key][names.index('CL')] is None
        for name in ('FedAvg', 'FedProx', 'FedAMW', 'DL', 'FedAMW_OneShot'):
            v = out[key][names.index(name)]
            if 'val' in key and name in ('FedAvg', 'FedProx', 'DL'):
                assert v is None
                continue
            assert len(v) == 1 and v[0].shape == ((4,) if name in ('DL', 'FedAMW_OneShot') else (2, 4)), (key, name)
            assert np.isfinite(v[0]).all()
            assert np.array_equal(saved[key][names.index(name)][0], v[0])
    assert out['test_loss'].shape == (6, 2, 1)
    plain = experiment.run('a9a', save=False, **kw)
    assert not [k for k in plain if k.startswith('client_')]
    for k in ('train_loss', 'test_loss', 'test_acc'):                       # the same run with and without
        assert np.array_equal(plain[k], out[k]), k


# --------------------------------------------------------------------------- #
# two ranks
# --------------------------------------------------------------------------- #
def _rank_run(algo):
    from fedamw_amd.functions import tools
    request = ('test', 'val') if algo == 'fedamw' else 'test'
    fed, stats, snaps, _ = _drive(tools, algo, 'parallel', request)
    res = {k: v.numpy() for k, v in stats.items() if k.startswith('client_') and k != 'client_eval'}
    return res, np.asarray(fed.mine), [s.cpu().numpy() for s in snaps]


def _worker(rank, world, port, algo, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    try:
        out[rank] = _rank_run(algo)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize('algo', ['fedavg', 'fedamw'])
def test_two_ranks(amd, algo):
    """Two gloo ranks on the one GPU, parallel clients.  Every rank returns the same [R, N]
    histories in the caller's client order, and they equal BITWISE a single process evaluating
    the same models -- the ranks' snapshots of W_out put back in the caller's order -- as
    clients 0..4 of 5: each rank scored them as clients of 3 or 2 (FedAMW 'val': as columns of
    its Z block of 4), so this is column independence across the shards.
    Against the single-process Federation run the histories agree to the tolerance of
    tests/test_gpu_dist.py only, from round 1 on: the sharded aggregate (one partial fold per
    rank, then an all-reduce) associates differently from the single-process left fold, so the
    global models, and every model trained from them, differ in their last bits.  Round 0 -- the
    same start -- is bitwise equal to it."""
    single_res, _, _ = _rank_run(algo)
    mgr = mp.get_context('spawn').Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), algo, out), nprocs=2, join=True)
    (res0, mine0, snaps0), (res1, mine1, snaps1) = out[0], out[1]
    assert sorted(list(mine0) + list(mine1)) == list(range(N))
    assert set(res0) == set(single_res) and len(res0) == (4 if algo == 'fedamw' else 2)
    for k in res0:
        assert res0[k].shape == (R, N) and np.array_equal(res0[k], res1[k]), k
    Xs, ys, Xt, yt, Xv, yv = _problem()
    dev = torch.device('cuda')
    ld = snaps0[0].shape[2]
    rows = {'test': (Xt, yt), 'val': (Xv, yv)}
    for which in ('test', 'val') if algo == 'fedamw' else ('test',):
        X, y = rows[which]
        ev = amd.engine.Evaluator(torch.from_numpy(X), torch.from_numpy(y), D, C, dev, ld)
        ce = amd.engine.ClientEvaluator(ev.f, C, N)
        for t in range(R):
            W = np.empty((N, C, ld), np.float32)
            W[mine0], W[mine1] = snaps0[t], snaps1[t]
            o = torch.empty(N, 2, dtype=torch.float64, device=dev)
            ce.run(torch.from_numpy(W).to(dev), N, o)
            o = o.cpu().numpy()
            assert np.array_equal(o[:, 0], res0['client_%s_loss' % which][t]), (which, t)
            assert np.array_equal(o[:, 1], res0['client_%s_acc' % which][t]), (which, t)
        # round 0 trains from the same start on every rank count: bitwise the single-process run
        for m in ('loss', 'acc'):
            assert np.array_equal(res0['client_%s_%s' % (which, m)][0], single_res['client_%s_%s' % (which, m)][0])
        np.testing.assert_allclose(res0['client_%s_loss' % which], single_res['client_%s_loss' % which], atol=1e-5)
        assert np.abs(res0['client_%s_acc' % which] - single_res['client_%s_acc' % which]).max() <= 100.0 / len(y) + 1e-4

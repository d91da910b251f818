"""RFA at drop-in level (the N = 14 ragged clients of the Krum and robust round tests, D = 32, C = 3 and C = 1
for regression, E = 2, B = 8, R = 3): ``tools.FedRFA`` against a replay of its rounds from engine pieces --
FedAvg's TRAIN phase, the corruption restated with torch, tests/rfa_restatement.py in numpy on the rows and
the round-start model as the aggregate saw them, the EVAL phase -- bit for bit in all three histories and
every round's global model; the attacks; the weightings; the plan setting and its rejections; the driver."""
import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO
from tests import krum_restatement as KR
from tests import rfa_restatement as RR

pytestmark = pytest.mark.gpu

N = len(KR.SIZES)
R = 3
OPTS = {'defer_eval': False, 'shuffle_chunk': 1}
F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    from fedamw_amd.functions import tools
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, tools=tools, dev=torch.device('cuda')))


def _data(regression=False):
    Xs, ys, Xt, yt = KR.case_data(regression)
    if regression:
        ys, yt = [y.reshape(-1, 1) for y in ys], yt.reshape(-1, 1)
    return ([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys], torch.from_numpy(Xt),
            torch.from_numpy(yt))


def _positional(regression=False, prox=False, batch=KR.B):
    return ('regression' if regression else 'classification', 1 if regression else KR.C, KR.D, KR.LR, KR.E, batch,
            prox, KR.MU, True, KR.LAM, R)


def _fed(amd, algo='fedavg', participation=None, opts=None, clients='parallel', regression=False, prox=False,
         batch=KR.B, **kw):
    torch.manual_seed(KR.TORCH_SEED)
    return amd.tools.Federation(algo, *_data(regression), None, *_positional(regression, prox, batch), 1e-3, clients,
                                verbose=False, options=opts, participation=participation,
                                sample_seed=KR.SAMPLE_SEED, **kw)


def _dropin(amd, iters=3, nu=1e-6, init='start', weighting='size', byzantine=None, participation=None,
            regression=False, prox=False, batch=KR.B, options=OPTS):
    stats = {'trace': True}
    torch.manual_seed(KR.TORCH_SEED)
    res = amd.tools.FedRFA(*_data(regression), *_positional(regression, prox, batch), iters=iters, nu=nu, init=init,
                           weighting=weighting, byzantine=byzantine, stats=stats, verbose=False, options=options,
                           participation=participation, sample_seed=KR.SAMPLE_SEED)
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return [r.numpy().copy() for r in res], stats, gen


def _replay(amd, iters, nu, init, weighting, byzantine, participation, regression, prox=False, batch=KR.B):
    """The drop-in's rounds from engine pieces on a FedAvg (FedProx) federation, the aggregate in numpy."""
    fed = _fed(amd, 'fedprox' if prox else 'fedavg', participation=participation, opts=OPTS, regression=regression,
               prox=prox, batch=batch)
    P = amd.lib.PHASE_TRAIN, amd.lib.PHASE_AGGREGATE, amd.lib.PHASE_EVAL
    bz = amd.tools.byzantine_plan(N, byzantine)
    rounds = []
    for t in range(R):
        if t == 0:
            fed._prepare_upto(1)
        fed.lr = amd.tools.update_learning_rate(t, fed.lr, fed.R)
        S = np.arange(N) if fed.sched is None else fed.sched[t]
        M = len(S)
        if fed.sched is None:
            fed.plan.round(t, fed.lr, P[0])
        else:
            fed.plan.round_subset(t, fed.lr, P[0], fed.sel_dev[t], fed.sel_order_dev[t], fed.q_dev[t], M)
        W = fed.trainer.W_out
        if bz is not None:
            ids, attack, scale, seed = bz
            rows = [int(k) for k in ids if k in set(S.tolist())]
            if rows and attack == 'sign_flip':
                for k in rows:
                    W[k] = fed.W_g - scale * (W[k] - fed.W_g)
            elif rows and attack == 'gaussian':
                z = amd.tools.byzantine_noise(seed, t, (len(rows), fed.C, KR.D)).to(amd.dev)
                for i, k in enumerate(rows):
                    W[k, :, :KR.D] = fed.W_g[:, :KR.D] + scale * z[i]
            elif rows:
                for k in rows:
                    W[k, :, :KR.D] = float('nan')
        rows32 = W.reshape(N, -1)[S].cpu().numpy().copy()
        x32 = fed.W_g.reshape(-1).cpu().numpy().copy()
        if weighting == 'uniform':
            alpha = np.full(M, F32(1.0 / M), F32)
        else:
            alpha = (fed.p_mine if fed.sched is None else fed.q_dev[t][:M]).cpu().numpy().astype(F32)
        ref = RR.chain(rows32, x32, alpha, iters, nu, init)
        fed.W_g.copy_(torch.from_numpy(ref['out']).reshape(fed.W_g.shape))
        rounds.append(dict(S=S, ref=ref, alpha=alpha, Wg=fed.W_g[:, :KR.D].cpu().numpy().copy()))
        if fed.sched is None:
            fed.plan.round(t, fed.lr, P[2])
        else:
            fed.plan.round_subset(t, fed.lr, P[2], fed.sel_dev[t], fed.sel_order_dev[t], fed.q_dev[t], M)
        fed.t += 1
        if fed.t < fed.R:
            fed._prepare_upto(fed.t + 1)
    res = [r.numpy().copy() for r in fed.results()]
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return res, rounds, gen


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype)
    ok = (got == ref) | (np.isnan(got) & np.isnan(ref))
    assert ok.all() and (np.signbit(got) == np.signbit(ref))[~np.isnan(got)].all(), (what, got, ref)


CASES = {
    'full': dict(),
    'full_t0': dict(iters=0),
    'mean_init': dict(init='mean', iters=2),
    'uniform_sampled': dict(weighting='uniform', participation=KR.PARTICIPATION),
    'sampled_flip': dict(participation=KR.PARTICIPATION, byzantine=dict(ids=[1, 4], attack='sign_flip', scale=4.0)),
    'gaussian': dict(byzantine=dict(fraction=0.2, attack='gaussian', scale=2.0, seed=3)),
    'nan': dict(byzantine=dict(fraction=0.2, attack='nan')),
    'nan_sampled_mean': dict(init='mean', participation=KR.PARTICIPATION, byzantine=dict(ids=[0, 5, 9], attack='nan')),
    'prox': dict(prox=True, nu=1e-3),
    'regression': dict(regression=True),
    'regression_flip_sampled': dict(regression=True, participation=KR.PARTICIPATION,
                                    byzantine=dict(ids=[0, 5], attack='sign_flip')),
    'large_batch': dict(batch=80, iters=1),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_dropin_is_the_replay_bit_for_bit(amd, name):
    k = dict(iters=3, nu=1e-6, init='start', weighting='size', byzantine=None, participation=None, regression=False,
             prox=False, batch=KR.B)
    k.update(CASES[name])
    res, stats, gen = _dropin(amd, **k)
    ref, rounds, gen2 = _replay(amd, **k)
    for what, a, b in zip(('train_loss', 'test_loss', 'test_acc'), res, ref):
        assert np.isfinite(a).all(), what
        _same(a, b, (name, what))
    T = k['iters']
    assert stats['rfa_weights'].shape == stats['rfa_dist'].shape == (R, N) and stats['rfa_weights'].dtype == F64
    assert stats['rfa_objective'].shape == (R, T + 2) and stats['rfa_objective'].dtype == F64
    for t, r in enumerate(rounds):
        S = r['S']
        _same(stats['W_rounds'][t], r['Wg'], (name, 'W_g', t))
        assert (np.isnan(stats['rfa_weights'][t]) == ~np.isin(np.arange(N), S)).all()
        _same(stats['rfa_weights'][t][S], r['ref']['b'].astype(F64), (name, 'weights', t))
        _same(stats['rfa_dist'][t][S], r['ref']['dist'], (name, 'dist', t))
        _same(stats['rfa_objective'][t], r['ref']['obj'], (name, 'objective', t))
    np.testing.assert_array_equal(gen, gen2)
    if k['byzantine'] is not None:
        ids = amd.tools.byzantine_plan(N, k['byzantine'])[0]
        assert np.array_equal(stats['byzantine_ids'], ids)
        if k['byzantine']['attack'] == 'nan':
            for t, r in enumerate(rounds):
                hit = np.intersect1d(ids, r['S'])
                assert (stats['rfa_weights'][t][hit] == 0).all()
    if not k['prox']:
        # the generator ends where FedAvg(clients='parallel') leaves it
        torch.manual_seed(KR.TORCH_SEED)
        amd.tools.FedAvg(*_data(k['regression']), *_positional(k['regression'], False, k['batch']), clients='parallel',
                         verbose=False, participation=k['participation'], sample_seed=KR.SAMPLE_SEED)
        np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), gen)


def test_default_options_change_no_number(amd):
    """The deferred evaluation and the chunked shuffles of the default options change no number."""
    bz = dict(ids=[2], attack='sign_flip')
    a = _dropin(amd, byzantine=bz)[0]
    b = _dropin(amd, byzantine=bz, options=None)[0]
    for x, y in zip(a, b):
        _same(x, y, 'default options')


def test_nan_attack_leaves_rfa_finite_and_the_mean_nan(amd):
    bz = dict(fraction=0.2, attack='nan')
    res, stats, _ = _dropin(amd, byzantine=bz)
    assert all(np.isfinite(r).all() for r in res) and np.isfinite(stats['W_rounds']).all()
    torch.manual_seed(KR.TORCH_SEED)
    mean = amd.tools.FedRobust(*_data(), *_positional(), rule='mean', byzantine=bz, verbose=False, options=OPTS)
    assert np.isnan(mean[2].numpy()).all() or np.isnan(mean[1].numpy()).all()


def test_weightings_differ(amd):
    a, sa, _ = _dropin(amd, weighting='size')
    b, sb, _ = _dropin(amd, weighting='uniform')
    assert not np.array_equal(sa['W_rounds'][-1], sb['W_rounds'][-1])
    assert not np.array_equal(sa['rfa_weights'], sb['rfa_weights'])
    assert not np.array_equal(a[1], b[1])


def test_off_restores_the_plain_aggregate(amd):
    """A FedAvg plan that ran one round with RFA set, then set_rfa(False): its next round, from the same
    round-start model, is bitwise the round of a plan that never had the setting."""
    plain = _fed(amd, 'fedavg', opts=OPTS)
    plain.round()
    W0 = plain.W_g.clone()
    plain.round()
    so = _fed(amd, 'fedavg', opts=OPTS)
    dist = torch.full((N,), -1.0, dtype=torch.float64, device=amd.dev)
    b = torch.full((N,), -1.0, device=amd.dev)
    obj = torch.full((5,), -1.0, dtype=torch.float64, device=amd.dev)
    so.plan.set_rfa(True, 3, 1e-6, 'start', False, dist, b, obj, so.agg.rfa_ws())
    so.round()
    torch.cuda.synchronize()
    assert not torch.equal(W0, so.W_g) and torch.isfinite(so.W_g).all()
    assert bool((b > 0).all()) and bool((dist > 0).all()) and bool(torch.isfinite(obj[:4]).all()) and bool(obj[4].isnan())
    so.plan.set_rfa(False)
    so.W_g.copy_(W0)
    so.round()
    torch.cuda.synchronize()
    assert torch.isfinite(plain.W_g).all() and torch.equal(plain.W_g, so.W_g)
    assert torch.equal(plain.loss_hist[1], so.loss_hist[1]) and torch.equal(plain.eval_hist[1], so.eval_hist[1])


def test_rejections(amd, monkeypatch):
    """The seven plan settings: RFA and each of the six others exclude each other in both directions with the
    documented messages; chained plans and bad arguments are refused."""
    E = amd.lib.FedsimError
    sc = FO.scalars(**FO.SERVER)
    dev = amd.dev
    dist = torch.zeros(N, dtype=torch.float64, device=dev)
    b = torch.zeros(N, device=dev)
    obj = torch.zeros(34, dtype=torch.float64, device=dev)
    chained = _fed(amd, 'fedavg', clients='sequential')
    with pytest.raises(E, match='parallel clients'):
        chained.plan.set_rfa(True, 3, 1e-6, 'start', False, dist, b, obj, chained.agg.rfa_ws())
    fed = _fed(amd, 'fedavg')
    ws = fed.agg.rfa_ws()
    rargs = (3, 1e-6, 'start', False, dist, b, obj, ws)
    for T in (-1, 33):
        with pytest.raises((E, ValueError), match=r'T must be in \[0, 32\]|set_rfa'):
            fed.plan.set_rfa(True, T, 1e-6, 'start', False, dist, b, torch.zeros(40, dtype=torch.float64, device=dev), ws)
    for nu in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(E, match='nu must be positive and finite'):
            fed.plan.set_rfa(True, 3, nu, 'start', False, dist, b, obj, ws)
    with pytest.raises(ValueError, match='init'):
        fed.plan.set_rfa(True, 3, 1e-6, 'median', False, dist, b, obj, ws)
    with pytest.raises(E, match='too small'):
        fed.plan.set_rfa(True, 3, 1e-6, 'start', False, dist, b, obj, ws[:ws.numel() - 8])
    with pytest.raises(ValueError, match='set_rfa'):
        fed.plan.set_rfa(True, 3, 1e-6, 'start', False, dist.to(torch.float32), b, obj, ws)
    with pytest.raises(ValueError, match='set_rfa'):
        fed.plan.set_rfa(True, 3, 1e-6, 'start', False, dist, b, obj[:4], ws)
    m, v = torch.zeros(fed.C, fed.ld, device=dev), torch.full((fed.C, fed.ld), 0.01, device=dev)
    c, ci, r = torch.zeros(fed.C, fed.ld, device=dev), torch.zeros(fed.N, fed.C, fed.ld, device=dev), \
        torch.ones(fed.N, device=dev)
    qf = dict(g=torch.zeros(fed.N, device=dev), S=torch.zeros(fed.C, fed.ld, device=dev),
              n=torch.zeros(fed.N, dtype=torch.float64, device=dev), hc=torch.zeros(2, dtype=torch.float64, device=dev),
              nws=fed.agg.qffl_ws())
    qargs = (qf['g'], 2.0, qf['S'], qf['n'], qf['hc'], qf['nws'])
    pick = torch.full((N,), -1, dtype=torch.int32, device=dev)
    score = torch.zeros(N, dtype=torch.float64, device=dev)
    kargs = (0.1, 0, pick, score, fed.agg.krum_ws())
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'RFA and a FedNova aggregate exclude each other'):
        fed.plan.set_rfa(True, *rargs)
    fed.plan.set_nova(0)
    fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'RFA and SCAFFOLD exclude each other'):
        fed.plan.set_rfa(True, *rargs)
    fed.plan.set_scaffold(False)
    fed.plan.set_server_opt('adam', m, v, *sc)
    with pytest.raises(E, match=r'RFA and a server optimizer exclude each other'):
        fed.plan.set_rfa(True, *rargs)
    fed.plan.set_server_opt(0)
    fed.plan.set_qffl(True, *qargs)
    with pytest.raises(E, match=r'RFA and q-FedAvg exclude each other'):
        fed.plan.set_rfa(True, *rargs)
    fed.plan.set_qffl(False)
    fed.plan.set_robust(True, 'median')
    with pytest.raises(E, match=r'RFA and a robust aggregate exclude each other'):
        fed.plan.set_rfa(True, *rargs)
    fed.plan.set_robust(False)
    fed.plan.set_krum(True, *kargs)
    with pytest.raises(E, match=r'RFA and Krum exclude each other'):
        fed.plan.set_rfa(True, *rargs)
    fed.plan.set_krum(False)
    fed.plan.set_rfa(True, *rargs)
    fed.plan.set_rfa(True, 1, 1e-3, 'mean', True, dist, b, obj, ws)            # callable again while on
    with pytest.raises(E, match=r'a FedNova aggregate and RFA exclude each other'):
        fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'SCAFFOLD and RFA exclude each other'):
        fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'a server optimizer and RFA exclude each other'):
        fed.plan.set_server_opt('adam', m, v, *sc)
    with pytest.raises(E, match=r'q-FedAvg and RFA exclude each other'):
        fed.plan.set_qffl(True, *qargs)
    with pytest.raises(E, match=r'a robust aggregate and RFA exclude each other'):
        fed.plan.set_robust(True, 'median')
    with pytest.raises(E, match=r'Krum and RFA exclude each other'):
        fed.plan.set_krum(True, *kargs)
    fed.plan.set_nova(0)                                                  # (turning the others off is not a change)
    fed.plan.set_server_opt(0)
    fed.plan.set_qffl(False)
    fed.plan.set_robust(False)
    fed.plan.set_krum(False)
    fed.plan.set_rfa(False)
    fed.plan.set_krum(True, *kargs)
    fed.plan.set_krum(False)
    with pytest.raises(ValueError, match='parallel'):
        _fed(amd, 'fedrfa', clients='sequential')
    with pytest.raises(ValueError, match='iters must be'):
        _fed(amd, 'fedrfa', rfa=dict(iters=33))
    monkeypatch.setattr(amd.tools.dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='rank'):
        amd.tools.FedRFA(*_data(), *_positional(), verbose=False)
    monkeypatch.undo()
    torch.cuda.synchronize()


def test_experiment_appends_the_row_in_order(amd, tmp_path):
    from fedamw_amd import experiment
    assert experiment.EXTRA_RFA == ['FedRFA']
    kw = dict(D=64, num_partitions=6, local_epoch=1, Round=3, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), save=False, synth=dict(n_train=900, n_test=120), verbose=False)
    out = experiment.run('a9a', algos=('FedRFA', 'FedAvg', 'MultiKrum'), **kw)
    assert out['name'] == experiment.NAMES + ['MultiKrum', 'FedRFA']
    for k in ('train_loss', 'test_loss', 'test_acc'):
        assert out[k].shape == (8, 3, 1) and np.isfinite(out[k][[3, 6, 7]]).all()
        assert np.isnan(out[k][[0, 1, 2, 4, 5]]).all()
    assert not np.array_equal(out['test_loss'][6], out['test_loss'][7])
    one = experiment.run('a9a', algos=('FedMedian', 'FedRFA'), rfa_iters=2, rfa_init='mean', rfa_weighting='uniform',
                         rfa_nu=1e-4, byzantine_fraction=0.2, byzantine_attack='nan', **kw)
    assert one['name'] == experiment.NAMES + ['FedMedian', 'FedRFA'] and np.isfinite(one['test_loss'][7]).all()
    part = experiment.run('a9a', algos=('FedRFA',), participation=0.7, **kw)
    assert part['name'] == experiment.NAMES + ['FedRFA'] and part['participants'][6] is not None


def test_smoke_still_passes():
    import __graft_entry__ as G
    G.smoke()

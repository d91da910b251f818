"""FedTopK at drop-in level (the N = 14 ragged clients of the Krum, robust and RFA round tests, D = 32, C = 3 and
C = 1 for regression, E = 2, B = 8, R = 3): ``tools.FedTopK(ratio=1.0)`` against ``tools.FedAvgM(server_lr=1.0,
beta1=0.0)`` -- whose q is p_k / sum_S p, FedAvg's -- bit for bit; at ``ratio=0.05`` against a replay of its
rounds from engine pieces with tests/topk_restatement.py in numpy as the aggregate, on the rows the engine
trained; the residual of an absent client; the stats; the plan setting and its rejections; the driver."""
import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO
from tests import krum_restatement as KR
from tests import topk_restatement as TK

pytestmark = pytest.mark.gpu

N = len(KR.SIZES)
R = 3
OPTS = {'defer_eval': False, 'shuffle_chunk': 1}
F32, F64 = np.float32, np.float64
PART = 0.5


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


def _dropin(amd, ratio=0.05, memory=True, participation=None, regression=False, prox=False, batch=KR.B,
            options=OPTS):
    stats = {'trace': True}
    torch.manual_seed(KR.TORCH_SEED)
    res = amd.tools.FedTopK(*_data(regression), *_positional(regression, prox, batch), ratio=ratio,
                            error_feedback=memory, stats=stats, verbose=False, options=options,
                            participation=participation, sample_seed=KR.SAMPLE_SEED)
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return [r.numpy().copy() for r in res], stats, gen


def _replay(amd, ratio, memory, participation, regression, prox=False, batch=KR.B):
    """The drop-in's rounds from engine pieces on a FedAvg (FedProx) federation, the aggregate in numpy."""
    fed = _fed(amd, 'fedprox' if prox else 'fedavg', participation=participation, opts=OPTS, regression=regression,
               prox=prox, batch=batch)
    P = amd.lib.PHASE_TRAIN, amd.lib.PHASE_AGGREGATE, amd.lib.PHASE_EVAL
    kc = TK.topk_count(ratio, fed.C, KR.D)
    L = fed.C * fed.ld
    e_all = np.zeros((N, L), F32) if memory else None
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
        rows32 = fed.trainer.W_out.reshape(N, -1)[S].cpu().numpy().copy()
        x32 = fed.W_g.reshape(-1).cpu().numpy().copy()
        q = (fed.p_mine if fed.sched is None else fed.q_dev[t][:M]).cpu().numpy().astype(F32)
        ref = TK.aggregate(rows32, x32, None if e_all is None else e_all[S], q, kc, 0, fed.agg.ws.numel() // L)
        if e_all is not None:
            e_all[S] = ref['e']
        fed.W_g.copy_(torch.from_numpy(ref['out']).reshape(fed.W_g.shape))
        rounds.append(dict(S=S, ref=ref, Wg=fed.W_g[:, :KR.D].cpu().numpy().copy(),
                           e=None if e_all is None else e_all.copy()))
        if fed.sched is None:
            fed.plan.round(t, fed.lr, P[2])
        else:
            fed.plan.round_subset(t, fed.lr, P[2], fed.sel_dev[t], fed.sel_order_dev[t], fed.q_dev[t], M)
        fed.t += 1
        if fed.t < fed.R:
            fed._prepare_upto(fed.t + 1)
    res = [r.numpy().copy() for r in fed.results()]
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return res, rounds, gen, (fed.C, fed.ld)


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype)
    ok = (got == ref) | (np.isnan(got) & np.isnan(ref))
    assert ok.all() and (np.signbit(got) == np.signbit(ref))[~np.isnan(got)].all(), (what, got, ref)


@pytest.mark.parametrize('participation', [None, PART])
@pytest.mark.parametrize('regression', [False, True])
def test_ratio_one_is_fedavgm_without_momentum(amd, participation, regression):
    """FedAvgM's q is FedAvg's p_k / sum_S p (tools.Federation: p_mine, or q_dev under participation)."""
    res, stats, gen = _dropin(amd, ratio=1.0, participation=participation, regression=regression)
    torch.manual_seed(KR.TORCH_SEED)
    st = {'trace': True}
    ref = amd.tools.FedAvgM(*_data(regression), *_positional(regression), server_lr=1.0, beta1=0.0, stats=st,
                            verbose=False, options=OPTS, participation=participation, sample_seed=KR.SAMPLE_SEED)
    gen2 = torch.empty(4, dtype=torch.int64).random_().numpy()
    for what, a, b in zip(('train_loss', 'test_loss', 'test_acc'), res, ref):
        assert np.isfinite(a).all(), what
        _same(a, b.numpy(), (what, participation, regression))
    _same(stats['W_rounds'], st['W_rounds'], 'W_rounds')
    np.testing.assert_array_equal(gen, gen2)
    assert float(stats['residual_norm'].max()) == 0.0 and not bool(stats['residual'].any())
    assert np.array_equal(stats['uplink_values'], stats['uplink_dense'])


CASES = {
    'memory': dict(),
    'no_memory': dict(memory=False),
    'memory_sampled': dict(participation=PART),
    'no_memory_sampled': dict(memory=False, participation=PART),
    'regression': dict(regression=True),
    'regression_no_memory': dict(regression=True, memory=False),
    'regression_sampled': dict(regression=True, participation=PART),
    'prox': dict(prox=True),
    'large_batch': dict(batch=80, ratio=0.1),
    'count': dict(ratio=7),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_dropin_is_the_replay_bit_for_bit(amd, name):
    k = dict(ratio=0.05, memory=True, participation=None, regression=False, prox=False, batch=KR.B)
    k.update(CASES[name])
    res, stats, gen = _dropin(amd, **k)
    ref, rounds, gen2, (C, ld) = _replay(amd, **k)
    for what, a, b in zip(('train_loss', 'test_loss', 'test_acc'), res, ref):
        assert np.isfinite(a).all(), what
        _same(a, b, (name, what))
    kc = TK.topk_count(k['ratio'], C, KR.D)
    assert amd.tools.topk_count(k['ratio'], C, KR.D) == kc
    for key in ('topk_kept', 'topk_tau'):
        assert stats[key].shape == (R, N) and stats[key].dtype == F64, key
    for key in ('uplink_values', 'uplink_dense', 'residual_norm'):
        assert stats[key].shape == (R,), key
    assert stats['uplink_values'].dtype == np.int64 and stats['residual_norm'].dtype == F64
    assert (stats['uplink_values'] <= stats['uplink_dense']).all()
    for t, r in enumerate(rounds):
        S = r['S']
        _same(stats['W_rounds'][t], r['Wg'], (name, 'W_g', t))
        assert (np.isnan(stats['topk_kept'][t]) == ~np.isin(np.arange(N), S)).all()
        assert (np.isnan(stats['topk_tau'][t]) == ~np.isin(np.arange(N), S)).all()
        _same(stats['topk_kept'][t][S], np.minimum(r['ref']['kept'], C * KR.D).astype(F64), (name, 'kept', t))
        _same(stats['topk_tau'][t][S], r['ref']['tau'].astype(F64), (name, 'tau', t))
        assert (stats['topk_kept'][t][S] >= kc).all()
        assert stats['uplink_values'][t] == int(stats['topk_kept'][t][S].sum())
        assert stats['uplink_dense'][t] == len(S) * C * KR.D
        if k['memory']:
            want = np.sqrt(np.sum(r['e'].astype(F64) ** 2))
            assert abs(stats['residual_norm'][t] - want) <= 1e-12 * max(1.0, want), (name, t)
        else:
            assert stats['residual_norm'][t] == 0.0
    if k['memory']:
        _same(stats['residual'].cpu().numpy(), rounds[-1]['e'].reshape(N, C, ld)[:, :, :KR.D], (name, 'residual'))
        assert stats['residual_norm'][-1] > 0
    else:
        assert 'residual' not in stats
    np.testing.assert_array_equal(gen, gen2)
    if not k['prox']:
        # the generator ends where FedAvg(clients='parallel') leaves it
        torch.manual_seed(KR.TORCH_SEED)
        amd.tools.FedAvg(*_data(k['regression']), *_positional(k['regression'], False, k['batch']), clients='parallel',
                         verbose=False, participation=k['participation'], sample_seed=KR.SAMPLE_SEED)
        np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), gen)


def test_memory_changes_the_result(amd):
    a, sa, _ = _dropin(amd, memory=True)
    b, sb, _ = _dropin(amd, memory=False)
    _same(sa['W_rounds'][0], sb['W_rounds'][0], 'round 0: no residual yet')
    assert not np.array_equal(sa['W_rounds'][-1], sb['W_rounds'][-1])


def test_absent_client_keeps_its_residual(amd):
    fed = _fed(amd, 'fedtopk', participation=PART, opts=OPTS, topk=dict(ratio=0.05, error_feedback=True))
    seen = np.zeros(N, bool)
    for t in range(R):
        before = fed.tk_e.clone()
        fed.round()
        torch.cuda.synchronize()
        S = fed.sched[t]
        absent = np.setdiff1d(np.arange(N), S)
        assert 0 < len(absent) < N
        a, b = before.cpu().numpy().view(np.uint32), fed.tk_e.cpu().numpy().view(np.uint32)
        assert np.array_equal(a[absent], b[absent]), t
        assert all(not np.array_equal(a[k], b[k]) for k in S), t
        seen[S] = True
        assert not b[~seen].any()                         # never sampled: still all +0
    fed.results()


def test_default_options_change_no_number(amd):
    """The deferred evaluation (its finaliser rides on the thresholded fold) and the chunked shuffles of the
    default options change no number."""
    a = _dropin(amd)[0]
    b = _dropin(amd, options=None)[0]
    for x, y in zip(a, b):
        _same(x, y, 'default options')


def test_off_restores_the_plain_aggregate(amd):
    plain = _fed(amd, 'fedavg', opts=OPTS)
    plain.round()
    W0 = plain.W_g.clone()
    plain.round()
    so = _fed(amd, 'fedavg', opts=OPTS)
    tau = torch.full((N,), -1.0, device=amd.dev)
    kept = torch.full((N,), -1, dtype=torch.int32, device=amd.dev)
    e = torch.zeros(N, so.C, so.ld, device=amd.dev)
    so.plan.set_topk(True, 5, e, tau, kept, so.agg.topk_ws())
    so.round()
    torch.cuda.synchronize()
    assert not torch.equal(W0, so.W_g) and torch.isfinite(so.W_g).all()
    assert bool((kept >= 5).all()) and bool((tau > 0).all()) and bool(e.any())
    so.plan.set_topk(False)
    so.W_g.copy_(W0)
    so.round()
    torch.cuda.synchronize()
    assert torch.isfinite(plain.W_g).all() and torch.equal(plain.W_g, so.W_g)
    assert torch.equal(plain.loss_hist[1], so.loss_hist[1]) and torch.equal(plain.eval_hist[1], so.eval_hist[1])


def test_rejections(amd, monkeypatch):
    """The eight plan settings: FedTopK and each of the seven others exclude each other in both directions
    with the documented messages; chained plans and bad arguments are refused."""
    E = amd.lib.FedsimError
    sc = FO.scalars(**FO.SERVER)
    dev = amd.dev
    tau = torch.zeros(N, device=dev)
    kept = torch.zeros(N, dtype=torch.int32, device=dev)
    chained = _fed(amd, 'fedavg', clients='sequential')
    with pytest.raises(E, match='parallel clients'):
        chained.plan.set_topk(True, 4, None, tau, kept, None)
    fed = _fed(amd, 'fedavg')
    e = torch.zeros(N, fed.C, fed.ld, device=dev)
    targs = (4, e, tau, kept, fed.agg.topk_ws())
    for kc in (0, -1, fed.C * fed.ld + 1):
        with pytest.raises(E, match=r'kcount must be in \[1, C \* ld\]'):
            fed.plan.set_topk(True, kc, e, tau, kept, None)
    with pytest.raises(E, match='d_e must not be d_W_g or d_W_out'):
        fed.plan.set_topk(True, 4, fed.W_g, tau, kept, None)
    with pytest.raises(E, match='d_e must not be d_W_g or d_W_out'):
        fed.plan.set_topk(True, 4, fed.trainer.W_out, tau, kept, None)
    with pytest.raises(ValueError, match='set_topk'):
        fed.plan.set_topk(True, 4, e, tau.to(torch.float64), kept, None)
    with pytest.raises(ValueError, match='set_topk'):
        fed.plan.set_topk(True, 4, e, tau, None, None)
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
    dist = torch.zeros(N, dtype=torch.float64, device=dev)
    b = torch.zeros(N, device=dev)
    obj = torch.zeros(34, dtype=torch.float64, device=dev)
    rargs = (3, 1e-6, 'start', False, dist, b, obj, fed.agg.rfa_ws())
    others = [
        ('a FedNova aggregate', lambda: fed.plan.set_nova(amd.lib.NOVA_UPDATES), lambda: fed.plan.set_nova(0)),
        ('SCAFFOLD', lambda: fed.plan.set_scaffold(True, c, ci, r), lambda: fed.plan.set_scaffold(False)),
        ('a server optimizer', lambda: fed.plan.set_server_opt('adam', m, v, *sc), lambda: fed.plan.set_server_opt(0)),
        ('q-FedAvg', lambda: fed.plan.set_qffl(True, *qargs), lambda: fed.plan.set_qffl(False)),
        ('a robust aggregate', lambda: fed.plan.set_robust(True, 'median'), lambda: fed.plan.set_robust(False)),
        ('Krum', lambda: fed.plan.set_krum(True, *kargs), lambda: fed.plan.set_krum(False)),
        ('RFA', lambda: fed.plan.set_rfa(True, *rargs), lambda: fed.plan.set_rfa(False)),
    ]
    for what, on, off in others:
        on()
        with pytest.raises(E, match=r'FedTopK and %s exclude each other' % what):
            fed.plan.set_topk(True, *targs)
        off()
    fed.plan.set_topk(True, *targs)
    fed.plan.set_topk(True, 9, None, tau, kept, None)                     # callable again while on
    for what, on, off in others:
        with pytest.raises(E, match=r'%s and FedTopK exclude each other' % what):
            on()
        off()                                                             # (turning the others off is not a change)
    fed.plan.set_topk(False)
    fed.plan.set_krum(True, *kargs)
    fed.plan.set_krum(False)
    with pytest.raises(ValueError, match='parallel'):
        _fed(amd, 'fedtopk', clients='sequential')
    with pytest.raises(ValueError, match='ratio'):
        _fed(amd, 'fedtopk', topk=dict(ratio=1.5))
    with pytest.raises(ValueError, match='error_feedback'):
        _fed(amd, 'fedtopk', topk=dict(error_feedback='yes'))
    monkeypatch.setattr(amd.tools.dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='rank'):
        amd.tools.FedTopK(*_data(), *_positional(), verbose=False)
    monkeypatch.undo()
    torch.cuda.synchronize()


def test_experiment_appends_the_row_in_order(amd, tmp_path):
    from fedamw_amd import experiment
    assert experiment.EXTRA_TOPK == ['FedTopK']
    kw = dict(D=64, num_partitions=6, local_epoch=1, Round=3, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), save=False, synth=dict(n_train=900, n_test=120), verbose=False)
    out = experiment.run('a9a', algos=('FedTopK', 'FedAvg', 'FedRFA'), topk_ratio=0.1, **kw)
    assert out['name'] == experiment.NAMES + ['FedRFA', 'FedTopK']
    for k in ('train_loss', 'test_loss', 'test_acc'):
        assert out[k].shape == (8, 3, 1) and np.isfinite(out[k][[3, 6, 7]]).all()
        assert np.isnan(out[k][[0, 1, 2, 4, 5]]).all()
    assert not np.array_equal(out['test_loss'][3], out['test_loss'][7])
    nomem = experiment.run('a9a', algos=('FedTopK',), topk_ratio=0.1, topk_memory=False, **kw)
    assert nomem['name'] == experiment.NAMES + ['FedTopK']
    assert not np.array_equal(nomem['test_loss'][6], out['test_loss'][7])
    part = experiment.run('a9a', algos=('FedTopK',), participation=0.7, **kw)
    assert part['name'] == experiment.NAMES + ['FedTopK'] and part['participants'][6] is not None


def test_smoke_still_passes():
    import __graft_entry__ as G
    G.smoke()

"""Krum and Multi-Krum at drop-in level (N = 14 ragged clients, D = 32, C = 3 and C = 1 for regression,
E = 2, B = 8, R = 2): ``tools.FedKrum`` against a replay of its rounds from engine pieces -- FedAvg's TRAIN
phase, the corruption restated with torch, ``Aggregator.run_krum`` with numpy's counts, the EVAL phase --
bit for bit in all three histories; the attacks, with the margin by which the attackers lose; the plan
setting and its rejections; the experiment driver."""
import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO
from tests import krum_restatement as KR

pytestmark = pytest.mark.gpu

N = len(KR.SIZES)
OPTS = {'defer_eval': False, 'shuffle_chunk': 1}
F64 = np.float64


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
            prox, KR.MU, True, KR.LAM, KR.R)


def _fed(amd, algo='fedavg', participation=None, opts=None, clients='parallel', regression=False, prox=False,
         batch=KR.B, **kw):
    torch.manual_seed(KR.TORCH_SEED)
    return amd.tools.Federation(algo, *_data(regression), None, *_positional(regression, prox, batch), 1e-3, clients,
                                verbose=False, options=opts, participation=participation,
                                sample_seed=KR.SAMPLE_SEED, **kw)


def _dropin(amd, f=0.1, m=None, byzantine=None, participation=None, regression=False, prox=False, batch=KR.B,
            options=OPTS):
    stats = {'trace': True}
    torch.manual_seed(KR.TORCH_SEED)
    res = amd.tools.FedKrum(*_data(regression), *_positional(regression, prox, batch), f=f, m=m, byzantine=byzantine,
                            stats=stats, verbose=False, options=options, participation=participation,
                            sample_seed=KR.SAMPLE_SEED)
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return [r.numpy().copy() for r in res], stats, gen


def _replay(amd, f, m, byzantine, participation, regression, prox=False, batch=KR.B):
    """The drop-in's rounds from engine pieces on a FedAvg (FedProx) federation; per round also the rows
    and the round-start model as the aggregate saw them."""
    fed = _fed(amd, 'fedprox' if prox else 'fedavg', participation=participation, opts=OPTS, regression=regression,
               prox=prox, batch=batch)
    P = amd.lib.PHASE_TRAIN, amd.lib.PHASE_AGGREGATE, amd.lib.PHASE_EVAL
    bz = amd.tools.byzantine_plan(N, byzantine)
    ws = fed.agg.krum_ws()
    rounds = []
    for t in range(KR.R):
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
        ft, mt = KR.counts(f, m, M)
        pick = torch.full((N,), -1, dtype=torch.int32, device=amd.dev)
        score = torch.full((N,), float('nan'), dtype=torch.float64, device=amd.dev)
        rows64 = W.reshape(N, -1)[S].cpu().numpy().copy()
        x64 = fed.W_g.reshape(-1).cpu().numpy().copy()
        fed.agg.run_krum(W, fed.W_g, ft, mt, fed.W_g, pick, score, ws,
                         sel=None if fed.sched is None else fed.sel_dev[t][:M].contiguous())
        full = np.full(N, np.nan)
        full[S] = score[:M].cpu().numpy()
        rounds.append(dict(f=ft, m=mt, S=S, selected=np.sort(pick[:mt].cpu().numpy().astype(np.int64)), scores=full,
                           rows=rows64, x=x64))
        if fed.sched is None:
            fed.plan.round(t, fed.lr, P[2])
        else:
            fed.plan.round_subset(t, fed.lr, P[2], fed.sel_dev[t], fed.sel_order_dev[t], fed.q_dev[t], M)
        fed.t += 1
        if fed.t < fed.R:
            fed._prepare_upto(fed.t + 1)
    res = [r.numpy().copy() for r in fed.results()]
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return res, rounds, fed.W_g[:, :KR.D].cpu().numpy(), gen


def _same(got, ref, what):
    assert np.asarray(got).tobytes() == np.asarray(ref).tobytes(), (what, got, ref)


CASES = {
    'multi_full': dict(),
    'krum_full': dict(m=1),
    'multi_sampled': dict(f=0.2, participation=KR.PARTICIPATION),
    'count_f_sampled_flip': dict(f=2, m=3, participation=KR.PARTICIPATION,
                                 byzantine=dict(ids=[1, 4], attack='sign_flip', scale=4.0)),
    'multi_gaussian': dict(f=0.25, byzantine=dict(fraction=0.2, attack='gaussian', scale=2.0, seed=3)),
    'multi_prox': dict(f=0.2, prox=True),
    'krum_regression': dict(m=1, regression=True),
    'multi_regression_flip': dict(f=0.2, regression=True, participation=KR.PARTICIPATION,
                                  byzantine=dict(ids=[0, 5], attack='sign_flip')),
    'multi_large_batch': dict(f=0.1, batch=80),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_dropin_is_the_replay_bit_for_bit(amd, name):
    k = dict(f=0.1, m=None, byzantine=None, participation=None, regression=False, prox=False, batch=KR.B)
    k.update(CASES[name])
    res, stats, gen = _dropin(amd, **k)
    ref, rounds, Wg, gen2 = _replay(amd, **k)
    for what, a, b in zip(('train_loss', 'test_loss', 'test_acc'), res, ref):
        assert np.isfinite(a).all(), what
        _same(a, b, (name, what))
    _same(stats['W_rounds'][-1], Wg, (name, 'W_g'))
    assert stats['krum_f'].dtype == np.int64 and stats['krum_f'].tolist() == [r['f'] for r in rounds]
    assert stats['krum_scores'].shape == (KR.R, N) and stats['krum_scores'].dtype == F64
    for t, r in enumerate(rounds):
        assert stats['krum_selected'][t].tolist() == r['selected'].tolist() and len(r['selected']) == r['m']
        assert set(r['selected'].tolist()) <= set(r['S'].tolist())
        assert (np.isnan(stats['krum_scores'][t]) == ~np.isin(np.arange(N), r['S'])).all()
        _same(stats['krum_scores'][t][r['S']], r['scores'][r['S']], (name, 'scores', t))
    np.testing.assert_array_equal(gen, gen2)
    if k['byzantine'] is not None:
        assert np.array_equal(stats['byzantine_ids'], amd.tools.byzantine_plan(N, k['byzantine'])[0])
    if not k['prox']:
        # the generator ends where FedAvg(clients='parallel') leaves it
        torch.manual_seed(KR.TORCH_SEED)
        amd.tools.FedAvg(*_data(k['regression']), *_positional(k['regression'], False, k['batch']), clients='parallel',
                         verbose=False, participation=k['participation'], sample_seed=KR.SAMPLE_SEED)
        np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), gen)


def test_default_options_and_thin_names(amd):
    """The deferred evaluation and the chunked shuffles of the default options change no number; Krum and
    MultiKrum are FedKrum with m = 1 and m = None."""
    bz = dict(ids=[2], attack='sign_flip')
    a = _dropin(amd, 0.1, None, byzantine=bz)[0]
    b = _dropin(amd, 0.1, None, byzantine=bz, options=None)[0]
    for x, y in zip(a, b):
        _same(x, y, 'default options')
    for fn, m in ((amd.tools.Krum, 1), (amd.tools.MultiKrum, None)):
        torch.manual_seed(KR.TORCH_SEED)
        st = {}
        got = fn(*_data(), *_positional(), f=0.2, stats=st, verbose=False, options=OPTS)
        ref, rst, _ = _dropin(amd, 0.2, m)
        for x, y in zip(got, ref):
            _same(x.numpy(), y, fn.__name__)
        assert [len(s) for s in st['krum_selected']] == [1 if m == 1 else N - 2] * KR.R


@pytest.mark.parametrize('attack', ['nan', 'sign_flip'])
@pytest.mark.parametrize('m', [1, None])
def test_attackers_are_never_selected(amd, attack, m):
    """attack='nan' and 'sign_flip' at scale 10 on 3 <= f clients (N = 14, f = floor(0.25 * 14) = 3): no
    corrupted id is selected, the histories are finite -- and not by luck: from the float64 scores of the
    rows the aggregate saw, the smallest attacker's score exceeds the largest selected score by more than
    1000 times what bound (b) allows the device's scores to be off by."""
    bz = dict(ids=[1, 6, 11], attack=attack, scale=10.0)
    res, stats, _ = _dropin(amd, 0.25, m, byzantine=bz)
    ref, rounds, _, _ = _replay(amd, 0.25, m, bz, None, False)
    for what, a, b in zip(('train_loss', 'test_loss', 'test_acc'), res, ref):
        assert np.isfinite(a).all(), what
        _same(a, b, (attack, what))
    assert np.isfinite(stats['W_rounds']).all()
    bad = np.array(bz['ids'])
    for t, r in enumerate(rounds):
        assert r['f'] == 3 and not set(stats['krum_selected'][t].tolist()) & set(bad.tolist())
        n = N - r['f'] - 2
        if attack == 'nan':
            assert np.isposinf(stats['krum_scores'][t][bad]).all()
            assert np.isfinite(np.delete(stats['krum_scores'][t], bad)).all()
            continue
        D64, n2 = KR.distances64(r['rows'], r['x'], gram=False)
        s64 = np.array([np.sort(np.delete(D64[a], a))[:n].sum() for a in range(N)])
        slack = n * KR.dist_bound(D64, n2, N, r['rows'].shape[1]).max()       # what n distances can be off by
        sel = stats['krum_selected'][t]
        margin = s64[bad].min() - s64[sel].max()
        print('round %d: attackers %.3g.., selected up to %.3g, margin / slack %.3g' % (t, s64[bad].min(),
                                                                                     s64[sel].max(), margin / slack))
        assert margin > 1000.0 * slack
        assert np.abs(stats['krum_scores'][t] - s64).max() <= slack


def test_off_restores_the_plain_aggregate(amd):
    """A FedAvg plan that ran one round with Krum set, then set_krum(False): its next round, from the same
    round-start model, is bitwise the round of a plan that never had the setting."""
    plain = _fed(amd, 'fedavg', opts=OPTS)
    plain.round()
    W0 = plain.W_g.clone()
    plain.round()
    so = _fed(amd, 'fedavg', opts=OPTS)
    pick = torch.full((N,), -1, dtype=torch.int32, device=amd.dev)
    score = torch.zeros(N, dtype=torch.float64, device=amd.dev)
    so.plan.set_krum(True, 0.1, 0, pick, score, so.agg.krum_ws())
    so.round()
    torch.cuda.synchronize()
    assert not torch.equal(W0, so.W_g) and torch.isfinite(so.W_g).all()
    assert int((pick >= 0).sum()) == N - 1 and bool((score > 0).all())
    so.plan.set_krum(False)
    so.W_g.copy_(W0)
    so.round()
    torch.cuda.synchronize()
    assert torch.isfinite(plain.W_g).all() and torch.equal(plain.W_g, so.W_g)
    assert torch.equal(plain.loss_hist[1], so.loss_hist[1]) and torch.equal(plain.eval_hist[1], so.eval_hist[1])


def test_rejections(amd, monkeypatch):
    """The six plan settings exclude each other with the documented messages; chained plans, small plans
    and bad arguments are refused."""
    E = amd.lib.FedsimError
    sc = FO.scalars(**FO.SERVER)
    dev = amd.dev
    pick = torch.full((N,), -1, dtype=torch.int32, device=dev)
    score = torch.zeros(N, dtype=torch.float64, device=dev)
    chained = _fed(amd, 'fedavg', clients='sequential')
    with pytest.raises(E, match='parallel clients'):
        chained.plan.set_krum(True, 0.1, 0, pick, score, chained.agg.krum_ws())
    fed = _fed(amd, 'fedavg')
    ws = fed.agg.krum_ws()
    kargs = (0.1, 0, pick, score, ws)
    for f in (-0.01, 0.5):
        with pytest.raises(E, match=r'f_frac must be in \[0, 0.5\)'):
            fed.plan.set_krum(True, f, 0, pick, score, ws)
    with pytest.raises(E, match='m_mode'):
        fed.plan.set_krum(True, 0.1, -1, pick, score, ws)
    with pytest.raises(E, match='too small'):
        fed.plan.set_krum(True, 0.1, 0, pick, score, ws[:ws.numel() - 8])
    with pytest.raises(ValueError, match='set_krum'):
        fed.plan.set_krum(True, 0.1, 0, pick.to(torch.int64), score, ws)
    m, v = torch.zeros(fed.C, fed.ld, device=dev), torch.full((fed.C, fed.ld), 0.01, device=dev)
    c, ci, r = torch.zeros(fed.C, fed.ld, device=dev), torch.zeros(fed.N, fed.C, fed.ld, device=dev), \
        torch.ones(fed.N, device=dev)
    qf = dict(g=torch.zeros(fed.N, device=dev), S=torch.zeros(fed.C, fed.ld, device=dev),
              n=torch.zeros(fed.N, dtype=torch.float64, device=dev), hc=torch.zeros(2, dtype=torch.float64, device=dev),
              nws=fed.agg.qffl_ws())
    qargs = (qf['g'], 2.0, qf['S'], qf['n'], qf['hc'], qf['nws'])
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'Krum and a FedNova aggregate exclude each other'):
        fed.plan.set_krum(True, *kargs)
    fed.plan.set_nova(0)
    fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'Krum and SCAFFOLD exclude each other'):
        fed.plan.set_krum(True, *kargs)
    fed.plan.set_scaffold(False)
    fed.plan.set_server_opt('adam', m, v, *sc)
    with pytest.raises(E, match=r'Krum and a server optimizer exclude each other'):
        fed.plan.set_krum(True, *kargs)
    fed.plan.set_server_opt(0)
    fed.plan.set_qffl(True, *qargs)
    with pytest.raises(E, match=r'Krum and q-FedAvg exclude each other'):
        fed.plan.set_krum(True, *kargs)
    fed.plan.set_qffl(False)
    fed.plan.set_robust(True, 'median')
    with pytest.raises(E, match=r'Krum and a robust aggregate exclude each other'):
        fed.plan.set_krum(True, *kargs)
    fed.plan.set_robust(False)
    fed.plan.set_krum(True, *kargs)
    fed.plan.set_krum(True, 0.2, 1, pick, score, ws)                      # callable again while on
    with pytest.raises(E, match=r'a FedNova aggregate and Krum exclude each other'):
        fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'SCAFFOLD and Krum exclude each other'):
        fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'a server optimizer and Krum exclude each other'):
        fed.plan.set_server_opt('adam', m, v, *sc)
    with pytest.raises(E, match=r'q-FedAvg and Krum exclude each other'):
        fed.plan.set_qffl(True, *qargs)
    with pytest.raises(E, match=r'a robust aggregate and Krum exclude each other'):
        fed.plan.set_robust(True, 'median')
    fed.plan.set_nova(0)                                                  # (turning the others off is not a change)
    fed.plan.set_server_opt(0)
    fed.plan.set_qffl(False)
    fed.plan.set_robust(False)
    fed.plan.set_krum(False)
    fed.plan.set_robust(True, 'median')
    fed.plan.set_robust(False)
    with pytest.raises(ValueError, match='parallel'):
        _fed(amd, 'fedkrum', clients='sequential')
    with pytest.raises(ValueError, match=r'M >= 2f \+ 3'):
        _fed(amd, 'fedkrum', krum=dict(f=6))
    monkeypatch.setattr(amd.tools.dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='rank'):
        amd.tools.MultiKrum(*_data(), *_positional(), verbose=False)
    monkeypatch.undo()
    torch.cuda.synchronize()


def test_small_plans_are_refused(amd):
    """N < 3: fs_plan_set_krum refuses the plan."""
    Xs, ys, Xt, yt = _data()
    torch.manual_seed(KR.TORCH_SEED)
    fed = amd.tools.Federation('fedavg', Xs[:2], ys[:2], Xt, yt, None, *_positional(), 1e-3, 'parallel', verbose=False)
    pick = torch.full((2,), -1, dtype=torch.int32, device=amd.dev)
    score = torch.zeros(2, dtype=torch.float64, device=amd.dev)
    with pytest.raises(amd.lib.FedsimError, match='N >= 3'):
        fed.plan.set_krum(True, 0.1, 0, pick, score, fed.agg.krum_ws(3))


def test_experiment_appends_the_two_rows_in_order(amd, tmp_path):
    from fedamw_amd import experiment
    assert experiment.EXTRA_KRUM == ['Krum', 'MultiKrum']
    kw = dict(D=64, num_partitions=6, local_epoch=1, Round=3, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), save=False, synth=dict(n_train=900, n_test=120), verbose=False)
    out = experiment.run('a9a', algos=('MultiKrum', 'FedAvg', 'Krum'), **kw)
    assert out['name'] == experiment.NAMES + ['Krum', 'MultiKrum']
    for k in ('train_loss', 'test_loss', 'test_acc'):
        assert out[k].shape == (8, 3, 1) and np.isfinite(out[k][[3, 6, 7]]).all()
        assert np.isnan(out[k][[0, 1, 2, 4, 5]]).all()
    assert not np.array_equal(out['test_loss'][6], out['test_loss'][7])
    one = experiment.run('a9a', algos=('FedMedian', 'MultiKrum'), krum_f=0.2, byzantine_fraction=0.2,
                         byzantine_attack='nan', **kw)
    assert one['name'] == experiment.NAMES + ['FedMedian', 'MultiKrum'] and np.isfinite(one['test_loss'][7]).all()
    part = experiment.run('a9a', algos=('Krum',), participation=0.7, krum_f=0.0, **kw)
    assert part['name'] == experiment.NAMES + ['Krum'] and part['participants'][6] is not None

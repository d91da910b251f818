"""Robust aggregation at drop-in level (N = 12 ragged clients, D = 32, C = 3 and C = 1 for regression,
E = 2, B = 8, R = 2): ``tools.FedRobust`` against a replay of its rounds from engine pieces -- FedAvg's
TRAIN phase, the corruption restated with torch, ``Aggregator.run_robust`` with numpy's trim count, the
EVAL phase -- bit for bit in all three histories; the NaN attack; the plan setting and its rejections;
the experiment driver."""
import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO
from tests import robust_restatement as RR

pytestmark = pytest.mark.gpu

N = len(RR.SIZES)
OPTS = {'defer_eval': False, 'shuffle_chunk': 1}


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    from fedamw_amd.functions import tools
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, tools=tools, dev=torch.device('cuda')))


def _data(regression=False):
    Xs, ys, Xt, yt = RR.case_data(regression)
    if regression:
        ys, yt = [y.reshape(-1, 1) for y in ys], yt.reshape(-1, 1)
    return ([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys], torch.from_numpy(Xt),
            torch.from_numpy(yt))


def _positional(regression=False):
    return ('regression' if regression else 'classification', 1 if regression else RR.C, RR.D, RR.LR, RR.E, RR.B,
            False, RR.MU, True, RR.LAM, RR.R)


def _fed(amd, algo='fedavg', participation=None, opts=None, clients='parallel', regression=False, **kw):
    torch.manual_seed(RR.TORCH_SEED)
    return amd.tools.Federation(algo, *_data(regression), None, *_positional(regression), 1e-3, clients,
                                verbose=False, options=opts, participation=participation,
                                sample_seed=RR.SAMPLE_SEED, **kw)


def _dropin(amd, rule, trim=0.1, byzantine=None, participation=None, regression=False, options=OPTS):
    stats = {'trace': True}
    torch.manual_seed(RR.TORCH_SEED)
    res = amd.tools.FedRobust(*_data(regression), *_positional(regression), rule=rule, trim=trim, byzantine=byzantine,
                              stats=stats, verbose=False, options=options, participation=participation,
                              sample_seed=RR.SAMPLE_SEED)
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return [r.numpy().copy() for r in res], stats, gen


def _replay(amd, rule, trim, byzantine, participation, regression, garbage=None):
    """The drop-in's rounds from engine pieces on a FedAvg federation.  ``garbage``: instead of the
    attack, (value for the rows) written into the corrupted rows."""
    fed = _fed(amd, 'fedavg', participation=participation, opts=OPTS, regression=regression)
    P = amd.lib.PHASE_TRAIN, amd.lib.PHASE_AGGREGATE, amd.lib.PHASE_EVAL
    bz = amd.tools.byzantine_plan(N, byzantine)
    bs = []
    for t in range(RR.R):
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
            if rows and garbage is not None:
                W[rows] = garbage
            elif rows and attack == 'sign_flip':
                for k in rows:
                    W[k] = fed.W_g - scale * (W[k] - fed.W_g)
            elif rows and attack == 'gaussian':
                z = amd.tools.byzantine_noise(seed, t, (len(rows), fed.C, RR.D)).to(amd.dev)
                for i, k in enumerate(rows):
                    W[k, :, :RR.D] = fed.W_g[:, :RR.D] + scale * z[i]
            elif rows:
                for k in rows:
                    W[k, :, :RR.D] = float('nan')
        b = RR.trim_count(rule, trim, M)
        bs.append(b)
        fed.agg.run_robust(W, b, fed.W_g, sel=None if fed.sched is None else fed.sel_dev[t][:M].contiguous())
        if fed.sched is None:
            fed.plan.round(t, fed.lr, P[2])
        else:
            fed.plan.round_subset(t, fed.lr, P[2], fed.sel_dev[t], fed.sel_order_dev[t], fed.q_dev[t], M)
        fed.t += 1
        if fed.t < fed.R:
            fed._prepare_upto(fed.t + 1)
    res = [r.numpy().copy() for r in fed.results()]
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return res, np.asarray(bs), fed.W_g[:, :RR.D].cpu().numpy(), gen


def _same(got, ref, what):
    assert RR.same_bits(got, ref), (what, got, ref)


CASES = {
    'median_full': dict(rule='median'),
    'median_sampled': dict(rule='median', participation=RR.PARTICIPATION),
    'trimmed_full': dict(rule='trimmed_mean', trim=0.2),
    'trimmed_sampled_flip': dict(rule='trimmed_mean', trim=0.2, participation=RR.PARTICIPATION,
                                 byzantine=dict(ids=[1, 4, 6, 9], attack='sign_flip', scale=4.0)),
    'median_gaussian': dict(rule='median', byzantine=dict(fraction=0.25, attack='gaussian', scale=2.0, seed=3)),
    'mean_full': dict(rule='mean'),
    'median_regression': dict(rule='median', regression=True),
    'trimmed_regression_flip': dict(rule='trimmed_mean', trim=0.25, regression=True, participation=RR.PARTICIPATION,
                                    byzantine=dict(ids=[0, 5], attack='sign_flip')),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_dropin_is_the_replay_bit_for_bit(amd, name):
    k = dict(rule='median', trim=0.1, byzantine=None, participation=None, regression=False)
    k.update(CASES[name])
    res, stats, gen = _dropin(amd, **k)
    ref, bs, Wg, gen2 = _replay(amd, **k)
    for what, a, b in zip(('train_loss', 'test_loss', 'test_acc'), res, ref):
        assert np.isfinite(a).all(), what
        _same(a, b, (name, what))
    _same(stats['W_rounds'][-1], Wg, (name, 'W_g'))
    assert stats['trim_count'].dtype == np.int64 and np.array_equal(stats['trim_count'], bs)
    np.testing.assert_array_equal(gen, gen2)
    if k['byzantine'] is not None:
        assert np.array_equal(stats['byzantine_ids'], amd.tools.byzantine_plan(N, k['byzantine'])[0])
    # the generator ends where FedAvg(clients='parallel') leaves it
    torch.manual_seed(RR.TORCH_SEED)
    amd.tools.FedAvg(*_data(k['regression']), *_positional(k['regression']), clients='parallel', verbose=False,
                     participation=k['participation'], sample_seed=RR.SAMPLE_SEED)
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), gen)


def test_default_options_give_the_same_histories(amd):
    """The deferred evaluation and the chunked shuffles of the default options change no number."""
    a = _dropin(amd, 'median', byzantine=dict(ids=[2], attack='sign_flip'))[0]
    b = _dropin(amd, 'median', byzantine=dict(ids=[2], attack='sign_flip'), options=None)[0]
    for x, y in zip(a, b):
        _same(x, y, 'default options')


def test_mean_rule_is_the_uniform_mean(amd):
    """rule='mean' against fs_aggregate with p = 1 / N on the same rows: the float64 sum rounded once
    against the float32 fold, within (N + 1) 2^-24 sum|W_k| / N."""
    fed = _fed(amd, 'fedavg', opts=OPTS)
    fed._prepare_upto(1)
    fed.lr = amd.tools.update_learning_rate(0, fed.lr, fed.R)
    fed.plan.round(0, fed.lr, amd.lib.PHASE_TRAIN)
    W = fed.trainer.W_out
    out = torch.zeros_like(fed.W_g)
    fed.agg.run_robust(W, 0, out)
    W64 = W.cpu().numpy().astype(np.float64)
    got = out.cpu().numpy()
    assert (np.abs(got - W64.mean(0)) <= 2.0 ** -24 * np.abs(W64.mean(0)) + N * 2.0 ** -52 * np.abs(W64).mean(0)
            + 2.0 ** -149).all()
    fold = fed.agg.run(W, torch.full((N,), 1.0 / N, device=amd.dev), torch.zeros_like(fed.W_g)).cpu().numpy()
    assert (np.abs(got - fold) <= (N + 1) * 2.0 ** -24 * np.abs(W64).sum(0) / N).all()


@pytest.mark.parametrize('rule,trim,ids', [('median', 0.1, [0, 3, 7, 8, 11]), ('trimmed_mean', 0.25, [2, 6, 10])])
def test_nan_attack_on_at_most_b_clients(amd, rule, trim, ids):
    """attack='nan' on f <= b clients (N = 12: the median's b = 5, trim 0.25's b = 3): the robust
    histories are finite and equal to the run where those rows hold any finite garbage of the same
    rank side (+3e38: NaN sorts to the top); rule='mean' is NaN."""
    bz = dict(ids=ids, attack='nan')
    assert len(ids) <= RR.trim_count(rule, trim, N)
    res, stats, _ = _dropin(amd, rule, trim=trim, byzantine=bz)
    ref = _replay(amd, rule, trim, bz, None, False, garbage=3e38)[0]
    for what, a, b in zip(('train_loss', 'test_loss', 'test_acc'), res, ref):
        assert np.isfinite(a).all(), what
        _same(a, b, (rule, what))
    assert np.isfinite(stats['W_rounds']).all()
    bad = _dropin(amd, 'mean', byzantine=bz)
    assert np.isnan(bad[0][1]).all() and np.isnan(bad[1]['W_rounds']).all()


def test_off_restores_the_plain_aggregate(amd):
    """A FedAvg plan that ran one round with the robust aggregate set, then set_robust(False): its next
    round, from the same round-start model, is bitwise the round of a plan that never had the setting."""
    plain = _fed(amd, 'fedavg', opts=OPTS)
    plain.round()
    W0 = plain.W_g.clone()
    plain.round()
    so = _fed(amd, 'fedavg', opts=OPTS)
    so.plan.set_robust(True, 'median')
    so.round()
    torch.cuda.synchronize()
    assert not torch.equal(W0, so.W_g) and torch.isfinite(so.W_g).all()
    so.plan.set_robust(False)
    so.W_g.copy_(W0)
    so.round()
    torch.cuda.synchronize()
    assert torch.isfinite(plain.W_g).all() and torch.equal(plain.W_g, so.W_g)
    assert torch.equal(plain.loss_hist[1], so.loss_hist[1]) and torch.equal(plain.eval_hist[1], so.eval_hist[1])


def test_rejections(amd, monkeypatch):
    """The five plan settings exclude each other with the documented messages; chained plans and bad
    arguments are refused."""
    E = amd.lib.FedsimError
    sc = FO.scalars(**FO.SERVER)
    chained = _fed(amd, 'fedavg', clients='sequential')
    with pytest.raises(E, match='parallel clients'):
        chained.plan.set_robust(True, 'median')
    fed = _fed(amd, 'fedavg')
    dev = amd.dev
    with pytest.raises(ValueError, match='mode'):
        fed.plan.set_robust(True, 'krum')
    for trim in (-0.01, 0.5):
        with pytest.raises(E, match=r'trim must be in \[0, 0.5\)'):
            fed.plan.set_robust(True, 'trimmed_mean', trim)
    fed.plan.set_robust(True, 'median', 0.9)                              # (the median ignores trim)
    fed.plan.set_robust(False)
    m, v = torch.zeros(fed.C, fed.ld, device=dev), torch.full((fed.C, fed.ld), 0.01, device=dev)
    c, ci, r = torch.zeros(fed.C, fed.ld, device=dev), torch.zeros(fed.N, fed.C, fed.ld, device=dev), \
        torch.ones(fed.N, device=dev)
    qf = dict(g=torch.zeros(fed.N, device=dev), S=torch.zeros(fed.C, fed.ld, device=dev),
              n=torch.zeros(fed.N, dtype=torch.float64, device=dev), hc=torch.zeros(2, dtype=torch.float64, device=dev),
              nws=fed.agg.qffl_ws())
    qargs = (qf['g'], 2.0, qf['S'], qf['n'], qf['hc'], qf['nws'])
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'a robust aggregate and a FedNova aggregate exclude each other'):
        fed.plan.set_robust(True, 'median')
    fed.plan.set_nova(0)
    fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'a robust aggregate and SCAFFOLD exclude each other'):
        fed.plan.set_robust(True, 'median')
    fed.plan.set_scaffold(False)
    fed.plan.set_server_opt('adam', m, v, *sc)
    with pytest.raises(E, match=r'a robust aggregate and a server optimizer exclude each other'):
        fed.plan.set_robust(True, 'median')
    fed.plan.set_server_opt(0)
    fed.plan.set_qffl(True, *qargs)
    with pytest.raises(E, match=r'a robust aggregate and q-FedAvg exclude each other'):
        fed.plan.set_robust(True, 'median')
    fed.plan.set_qffl(False)
    fed.plan.set_robust(True, 'trimmed_mean', 0.1)
    fed.plan.set_robust(True, 'median')                                   # callable again while on
    with pytest.raises(E, match=r'a FedNova aggregate and a robust aggregate exclude each other'):
        fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'SCAFFOLD and a robust aggregate exclude each other'):
        fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'a server optimizer and a robust aggregate exclude each other'):
        fed.plan.set_server_opt('adam', m, v, *sc)
    with pytest.raises(E, match=r'q-FedAvg and a robust aggregate exclude each other'):
        fed.plan.set_qffl(True, *qargs)
    fed.plan.set_nova(0)                                                  # (turning the others off is not a change)
    fed.plan.set_server_opt(0)
    fed.plan.set_qffl(False)
    fed.plan.set_robust(False)
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    fed.plan.set_nova(0)
    with pytest.raises(ValueError, match='parallel'):
        _fed(amd, 'fedrobust', clients='sequential')
    monkeypatch.setattr(amd.tools.dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='rank'):
        amd.tools.FedMedian(*_data(), *_positional(), verbose=False)
    monkeypatch.undo()
    torch.cuda.synchronize()


def test_prox_and_large_batches_train_as_fedavg(amd):
    """prox=True and a batch size above 64 (the wide form) run under the robust aggregate."""
    for bsz, prox in ((RR.B, True), (80, False)):
        st = {'trace': True}
        torch.manual_seed(RR.TORCH_SEED)
        amd.tools.FedTrimmedMean(*_data(), 'classification', RR.C, RR.D, RR.LR, RR.E, bsz, prox, RR.MU, True, RR.LAM,
                                 RR.R, trim=0.2, stats=st, verbose=False)
        assert np.isfinite(st['W_rounds']).all() and st['trim_count'].tolist() == [2, 2]


def test_experiment_appends_the_two_rows_in_order(amd, tmp_path):
    from fedamw_amd import experiment
    assert experiment.EXTRA_ROBUST == ['FedMedian', 'FedTrimmedMean']
    kw = dict(D=64, num_partitions=4, local_epoch=1, Round=3, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), save=False, synth=dict(n_train=700, n_test=120), verbose=False)
    out = experiment.run('a9a', algos=('FedTrimmedMean', 'FedAvg', 'FedMedian'), **kw)
    assert out['name'] == experiment.NAMES + ['FedMedian', 'FedTrimmedMean']
    for k in ('train_loss', 'test_loss', 'test_acc'):
        assert out[k].shape == (8, 3, 1) and np.isfinite(out[k][[3, 6, 7]]).all()
        assert np.isnan(out[k][[0, 1, 2, 4, 5]]).all()
    assert not np.array_equal(out['test_loss'][6], out['test_loss'][3])
    one = experiment.run('a9a', algos=('QFedAvg', 'FedMedian'), byzantine_fraction=0.25, byzantine_attack='nan', **kw)
    assert one['name'] == experiment.NAMES + ['QFedAvg', 'FedMedian'] and np.isfinite(one['test_loss'][7]).all()
    part = experiment.run('a9a', algos=('FedTrimmedMean',), participation=0.5, robust_trim=0.3, **kw)
    assert part['name'] == experiment.NAMES + ['FedTrimmedMean'] and part['participants'][6] is not None

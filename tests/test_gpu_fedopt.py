"""The FedOpt server optimizers at drop-in level (the SCAFFOLD drop-in test's scale: N = 6 unequal
clients, C = 3, D = 64, E = 2, B = 8, R = 3): the exact wiring of fs_aggregate_opt into the round on
the GPU's own buffers, ``tools.FedOpt`` against tests/fedopt_restatement.py on its eleven cases, the
plan setting and its rejections, and the experiment driver.

Tolerances of the restatement comparison: with tau = server_lr = 0.1 the server step is a contraction
in delta (tests/fedopt_restatement.py), so a round adds at most one training-kernel tolerance: W of
round t within max((t + 1) 2e-5 max|W|, 2 delta_W max|W|), the three returns within
max(1e-5 max(1, |.|), 2 delta_loss max(1, |.|)), the deltas recorded in
tests/golden/fedopt_drift.json (<= 2e-7, so the first terms hold)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_TOL, LOSS_TOL = 2e-5, 1e-5


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    from fedamw_amd.functions import tools
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, tools=tools, dev=torch.device('cuda')))


def _data(regression=False):
    Xs, ys, Xt, yt = FO.case_data(regression)
    if regression:
        ys, yt = [y.reshape(-1, 1) for y in ys], yt.reshape(-1, 1)
    return ([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys], torch.from_numpy(Xt),
            torch.from_numpy(yt))


def _positional(name=None):
    type, nc, bs, prox = FO.case_args(name) if name else ('classification', FO.C, FO.B, False)
    return (type, nc, FO.D, FO.LR, FO.E, bs, prox, FO.MU, True, FO.LAM, FO.R)


def _sched(sched):
    return None if sched is None else [s.copy() for s in sched]


def _fed(amd, algo='fedopt', rule='adam', sched=None, opts=None, clients='parallel', **kw):
    torch.manual_seed(FO.TORCH_SEED)
    if algo == 'fedopt':
        kw['server_opt'] = dict(rule=rule, **FO.SERVER)
    return amd.tools.Federation(algo, *_data(), None, *_positional(), 1e-3, clients, verbose=False, options=opts,
                                participation=_sched(sched), **kw)


def _same(got, ref, what):
    got, ref = got.reshape(-1), ref.reshape(-1)
    bad = np.flatnonzero(got != ref)
    assert got.tobytes() == ref.tobytes(), (what, len(bad), got[bad[:4]], ref[bad[:4]])


def _drive(amd, rule, sched, defer):
    """Federation.round() by hand: after every round the numpy step on the GPU's own W_out and the
    previous W_g / m / v, with that round's q, must be the new W_g / m / v bit for bit (M < 16: the
    left-fold regime).  Returns the evaluation history."""
    fed = _fed(amd, rule=rule, sched=sched, opts={'defer_eval': defer})
    sc = fed.opt_scalars[1:]
    assert sc == FO.scalars(**FO.SERVER)
    N = len(FO.SIZES)
    x, m, v = (a.cpu().numpy() for a in (fed.W_g, fed.opt_m, fed.opt_v))
    assert not m.any() and (v == np.float32(float(FO.SERVER['tau']) ** 2)).all()
    for t in range(FO.R):
        fed.round()
        torch.cuda.synchronize()
        S = np.arange(N) if sched is None else sched[t]
        q = (fed.p_mine if sched is None else fed.q_dev[t][:len(S)]).cpu().numpy()
        np.testing.assert_array_equal(q, (np.array(FO.SIZES)[S] / sum(np.array(FO.SIZES)[S])).astype(np.float32))
        W_out = fed.trainer.W_out.cpu().numpy().reshape(N, -1)
        ref = FO.server(rule, x.reshape(-1), m.reshape(-1), v.reshape(-1), [W_out[j] for j in S], q, sc)
        x2, m2, v2 = (a.cpu().numpy() for a in (fed.W_g, fed.opt_m, fed.opt_v))
        assert np.isfinite(x2).all() and not np.array_equal(x2, x)
        _same(x2, ref[0], (rule, t, 'W_g'))
        _same(m2, ref[1], (rule, t, 'm'))
        if rule == 'avgm':
            _same(v2, v, (rule, t, 'v untouched'))
        else:
            _same(v2, ref[2], (rule, t, 'v'))
        assert not x2[:, FO.D:].any()                                    # the padding columns: 0 / positive
        x, m, v = x2, m2, v2
    res = fed.results()
    return fed.eval_hist.cpu().numpy().copy(), [r.numpy().copy() for r in res], x


@pytest.mark.parametrize('rule', FO.RULES)
def test_exact_wiring_on_the_gpus_own_buffers(amd, rule):
    """All four rules, with participation = 3 over three distinct samples, and with defer_eval on,
    where the test metrics must be the undeferred run's exactly (the finaliser's path)."""
    _drive(amd, rule, FO.SCHED, False)
    plain = _drive(amd, rule, None, False)
    deferred = _drive(amd, rule, None, True)
    _same(deferred[2], plain[2], 'W_g')
    print(rule, 'eval_hist deferred - plain', np.abs(deferred[0] - plain[0]).max())
    assert np.isfinite(plain[0]).all()
    assert np.array_equal(deferred[0], plain[0])
    for a, b in zip(deferred[1], plain[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('rule', ['adam', 'avgm'])
def test_deferred_evaluation_rides_across_the_opt_aggregate(amd, rule):
    """The split form at N = 10 leaves CUs idle: round t's evaluation fuses into round t+1's TRAIN
    launch and its finaliser rides on fs_aggregate_opt.  Same models and moments bitwise, the same
    eval_hist to the 1e-12 relative the header states for a fused deferral."""
    tune = dict(train_form=1, split_mb=-1, split_dbuf=-1, split_pipe=-1, split_teams=-1)
    C, N, R, D, n_t = 10, 10, 3, 1024, 16 * 16 + 5
    rs = np.random.RandomState(17)
    sizes = rs.randint(8, 41, size=N)
    Xs = [torch.from_numpy((np.cos(rs.normal(size=(n, D))) / np.sqrt(D)).astype(np.float32)) for n in sizes]
    ys = [torch.from_numpy(rs.randint(0, C, size=n).astype(np.int64)) for n in sizes]
    Xt = torch.from_numpy((np.cos(rs.normal(size=(n_t, D))) / np.sqrt(D)).astype(np.float32))
    yt = torch.from_numpy(rs.randint(0, C, size=n_t).astype(np.int64))
    runs = {}
    with amd.lib.tuning(**tune):
        for defer in (False, True):
            stats = {'trace': True}
            torch.manual_seed(11)
            fed = amd.tools.Federation('fedopt', Xs, ys, Xt, yt, None, 'classification', C, D, 0.5, 1, 32, False, 0.0,
                                       False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False,
                                       options={'defer_eval': defer}, server_opt=dict(rule=rule, **FO.SERVER))
            for _ in range(R):
                fed.round()
            fed.results()
            assert fed.plan.eval_blocks() > 0
            runs[defer] = (stats['W_rounds'], stats['server_m_rounds'], stats['server_v_rounds'],
                           fed.eval_hist.cpu().numpy().copy())
    for k in range(3):
        assert np.array_equal(runs[False][k], runs[True][k])
    assert np.isfinite(runs[True][3]).all()
    np.testing.assert_allclose(runs[True][3], runs[False][3], rtol=1e-12, atol=0)


def _bounds(name):
    with open(os.path.join(ROOT, 'tests', 'golden', 'fedopt_drift.json')) as f:
        d = json.load(f)[name]
    return d['delta_W'], max(LOSS_TOL, 2 * d['delta_loss'])


@pytest.mark.parametrize('name', sorted(FO.CASES))
def test_dropin_matches_the_restatement(amd, name):
    k = FO.CASES[name]
    reg = k.get('type') == 'regression'
    ref = FO.run_case(name)
    rng_ref = torch.empty(4, dtype=torch.int64).random_().numpy()
    stats = {'trace': True}
    torch.manual_seed(FO.TORCH_SEED)
    tr, tl, ta = amd.tools.FedOpt(*_data(reg), *_positional(name), server_opt=k['rule'], stats=stats, verbose=False,
                                  participation=_sched(k['sched']), **FO.SERVER)
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), rng_ref)
    dW, ltol = _bounds(name)
    C = 1 if reg else FO.C
    W = stats['W_rounds']
    assert W.shape == ref[3]['W'].shape == (FO.R, C, FO.D)
    for key in ('server_m', 'server_v'):
        assert tuple(stats[key].shape) == (C, FO.D) and stats[key + '_rounds'].shape == W.shape
        assert np.array_equal(stats[key].cpu().numpy(), stats[key + '_rounds'][-1])
    assert np.isfinite(stats['server_m_rounds']).all() and stats['server_m_rounds'].any()
    assert (stats['server_v_rounds'] > 0).all()
    for t in range(FO.R):
        Wr = ref[3]['W'][t]
        err = np.abs(W[t] - Wr).max()
        bound = max((t + 1) * W_TOL, 2 * dW) * np.abs(Wr).max()
        print('%s round %d: W err %.3g of %.3g' % (name, t, err, bound))
        assert err <= bound
    for what, got, want in (('train_loss', tr, ref[0]), ('test_loss', tl, ref[1]), ('test_acc', ta, ref[2])):
        err = np.abs(got.numpy() - want)
        print('%s %s: max err %.3g' % (name, what, (err / np.maximum(1.0, np.abs(want))).max()))
        assert (err <= ltol * np.maximum(1.0, np.abs(want))).all(), what
    if k['sched'] is not None:
        assert all(np.array_equal(a, b) for a, b in zip(stats['participants'], FO.SCHED))


def test_train_loss_and_generator_are_fedavgs(amd):
    """The same training launch: round 0 trains from the same model, so its train_loss is bitwise
    FedAvg's with parallel clients, under participation too; and the generator ends where FedAvg
    leaves it."""
    for sched in (None, FO.SCHED):
        torch.manual_seed(FO.TORCH_SEED)
        a = amd.tools.FedAvg(*_data(), *_positional(), clients='parallel', verbose=False, participation=_sched(sched))
        ra = torch.empty(4, dtype=torch.int64).random_().numpy()
        torch.manual_seed(FO.TORCH_SEED)
        b = amd.tools.FedYogi(*_data(), *_positional(), verbose=False, participation=_sched(sched), **FO.SERVER)
        rb = torch.empty(4, dtype=torch.int64).random_().numpy()
        np.testing.assert_array_equal(ra, rb)
        assert float(a[0][0]) == float(b[0][0]) and not np.array_equal(a[1].numpy(), b[1].numpy())


def test_rule_zero_restores_the_plain_aggregate(amd):
    """A FedAvg plan that ran one round with a rule set, then set_server_opt(0): its next round, from
    the same round-start model, is bitwise the round of a plan that never had the setting."""
    opts = {'defer_eval': False, 'shuffle_chunk': 1}
    plain = _fed(amd, 'fedavg', opts=opts)
    plain.round()
    W0 = plain.W_g.clone()
    plain.round()
    so = _fed(amd, 'fedavg', opts=opts)
    m = torch.zeros(FO.C, so.ld, device=amd.dev)
    v = torch.full((FO.C, so.ld), 0.01, device=amd.dev)
    so.plan.set_server_opt('adam', m, v, *FO.scalars(**FO.SERVER))
    so.round()
    torch.cuda.synchronize()
    assert not torch.equal(W0, so.W_g) and bool(m.any()) and not bool((v == 0.01).all())
    so.plan.set_server_opt(0)
    so.W_g.copy_(W0)
    so.round()
    torch.cuda.synchronize()
    assert torch.isfinite(plain.W_g).all() and torch.equal(plain.W_g, so.W_g)
    assert torch.equal(plain.loss_hist[1], so.loss_hist[1]) and torch.equal(plain.eval_hist[1], so.eval_hist[1])


def test_rejections(amd, monkeypatch):
    E = amd.lib.FedsimError
    sc = FO.scalars(**FO.SERVER)

    def bufs(fed):
        return torch.zeros(fed.C, fed.ld, device=amd.dev), torch.full((fed.C, fed.ld), 0.01, device=amd.dev)

    chained = _fed(amd, 'fedavg', clients='sequential')
    with pytest.raises(E, match=r'\(-1\)'):
        chained.plan.set_server_opt('adam', *bufs(chained), *sc)
    fed = _fed(amd, 'fedavg')
    m, v = bufs(fed)
    for args in ((None, v), (m, None), (m, m), (fed.W_g, v)):
        with pytest.raises(E, match=r'\(-1\)'):
            fed.plan.set_server_opt('yogi', *args, *sc)
    with pytest.raises(E, match=r'\(-1\)'):
        fed.plan.set_server_opt(5, m, v, *sc)
    with pytest.raises(E, match=r'\(-1\)'):
        fed.plan.set_server_opt('adam', m, v, *sc[:5], 0.0)              # tau
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'\(-1\)'):                              # a nova mode other than 0
        fed.plan.set_server_opt('adam', m, v, *sc)
    fed.plan.set_nova(0)
    N = fed.N
    c, ci, r = torch.zeros(fed.C, fed.ld, device=amd.dev), torch.zeros(N, fed.C, fed.ld, device=amd.dev), \
        torch.ones(N, device=amd.dev)
    fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'\(-1\)'):                              # SCAFFOLD on
        fed.plan.set_server_opt('adam', m, v, *sc)
    fed.plan.set_scaffold(False)
    fed.plan.set_server_opt('avgm', m, None, *sc)                        # (avgm has no second moment)
    fed.plan.set_server_opt('adam', m, v, *sc)
    with pytest.raises(E, match=r'\(-1\)'):                              # and the other two refuse in turn
        fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'\(-1\)'):
        fed.plan.set_scaffold(True, c, ci, r)
    fed.plan.set_nova(0)                                                 # (turning nova off is not a change)
    fed.plan.set_server_opt(0)
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    fed.plan.set_nova(0)
    # prox, loss = 1 and B > 64 are allowed: they are the point
    for kw in (dict(name='adam_prox'), dict(name='yogi_regression'), dict(name='adam_wide')):
        name = kw['name']
        reg = FO.CASES[name].get('type') == 'regression'
        torch.manual_seed(3)
        f2 = amd.tools.Federation('fedprox' if name == 'adam_prox' else 'fedavg', *_data(reg), None, *_positional(name),
                                  1e-3, 'parallel', verbose=False)
        f2.plan.set_server_opt('adam', *bufs(f2), *sc)
    with pytest.raises(ValueError, match='parallel'):
        _fed(amd, 'fedopt', clients='sequential')
    monkeypatch.setattr(amd.tools.dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='rank'):
        amd.tools.FedAdam(*_data(), *_positional(), verbose=False)
    monkeypatch.undo()
    torch.cuda.synchronize()


def test_experiment_appends_fedadam_only_when_asked(amd, tmp_path):
    from fedamw_amd import experiment
    assert experiment.EXTRA == ['FedNova', 'Scaffold', 'FedAvgM', 'FedAdagrad', 'FedAdam', 'FedYogi']
    kw = dict(D=64, num_partitions=4, local_epoch=1, Round=3, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), save=False, synth=dict(n_train=700, n_test=120), verbose=False)
    six = experiment.run('a9a', algos=('FedAvg',), **kw)
    out = experiment.run('a9a', algos=('FedAvg', 'FedAdam'), **kw)
    assert six['name'] == experiment.NAMES and out['name'] == experiment.NAMES + ['FedAdam']
    for k in ('train_loss', 'test_loss', 'test_acc'):
        assert out[k].shape == (7, 3, 1) and np.isfinite(out[k][[3, 6]]).all() and np.isnan(out[k][[0, 1, 2, 4, 5]]).all()
        assert np.array_equal(out[k][3], six[k][3])
    assert not np.array_equal(out['test_loss'][6], out['test_loss'][3])
    slow = experiment.run('a9a', algos=('FedAdam',), server_lr=1e-3, server_beta1=0.5, server_beta2=0.9, server_tau=0.1,
                          **kw)
    assert not np.array_equal(slow['test_loss'][6], out['test_loss'][6])
    ap = experiment.main.__code__.co_consts
    assert all(flag in ap for flag in ('--server-lr', '--server-beta1', '--server-beta2', '--server-tau'))

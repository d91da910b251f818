"""SCAFFOLD at drop-in level: ``tools.Scaffold`` against tests/scaffold_restatement.py on its eight
cases (N = 6 unequal clients, D = 64, C = 4, R = 3, E = 2, B = 8, lr = 0.5, ridge on; all clients and
M = 3 of 6 with three distinct samples; both weightings; server_lr 1.0 and 0.5), against FedAvg in
rounds 0 and 1, the variates' invariant on the GPU, the plan setting, the experiment driver and the
Python rejections.

Tolerances: W per round 2e-5 max|W|; c per round 2e-5 max|c| + 2e-5 max|W| / (K_min lr) -- c is a
difference of models divided by K lr, so the model tolerance reaches it with that factor; the three
returns 1e-5 max(1, |.|).  The recorded float32 drift (tests/golden/scaffold_drift.json: <= 2e-7 in
W, <= 5e-8 in c in the same normalisation, <= 1.3e-7 in the losses) is far below half of each, so
max(bound, 2 delta) is the bound itself."""
import json
import os

import numpy as np
import pytest
import torch

from tests import scaffold_restatement as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_TOL, LOSS_TOL = 2e-5, 1e-5
U = 2.0 ** -24


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    from fedamw_amd.functions import tools
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, tools=tools, dev=torch.device('cuda')))


def _data():
    Xs, ys, Xt, yt = SR.case_data()
    return ([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys], torch.from_numpy(Xt),
            torch.from_numpy(yt))


def _positional():
    return ('classification', SR.C, SR.D, SR.LR, SR.E, SR.B, False, 0.0, True, SR.LAM, SR.R)


def _kw(name):
    k = SR.CASES[name]
    return dict(server_lr=k['server_lr'], weighting=k['weighting'],
                participation=None if k['sched'] is None else [s.copy() for s in k['sched']])


def _bounds(name):
    with open(os.path.join(ROOT, 'tests', 'golden', 'scaffold_drift.json')) as f:
        d = json.load(f)[name]
    return max(W_TOL, 2 * d['delta_W']), max(W_TOL, 2 * d['delta_c']), max(LOSS_TOL, 2 * d['delta_loss'])


@pytest.mark.parametrize('name', sorted(SR.CASES))
def test_dropin_matches_the_restatement(amd, name):
    ref = SR.run_case(name)
    rng_ref = torch.empty(4, dtype=torch.int64).random_().numpy()
    stats = {'trace': True}
    torch.manual_seed(SR.TORCH_SEED)
    tr, tl, ta = amd.tools.Scaffold(*_data(), *_positional(), stats=stats, verbose=False, **_kw(name))
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), rng_ref)
    wtol, ctol, ltol = _bounds(name)
    assert (wtol, ctol, ltol) == (W_TOL, W_TOL, LOSS_TOL)
    W, c = stats['W_rounds'], stats['c_rounds']
    assert W.shape == ref[3]['W'].shape == (SR.R, SR.C, SR.D) and c.shape == W.shape
    assert tuple(stats['c_global'].shape) == (SR.C, SR.D)
    assert np.array_equal(stats['c_global'].cpu().numpy(), c[-1])
    kmin = float(SR.steps(SR.SIZES, SR.E, SR.B).min())
    lr = SR.LR
    for t in range(SR.R):
        lr = SR.O.lr_schedule(t, lr, SR.R)
        Wr, cr = ref[3]['W'][t], ref[3]['c'][t]
        eW, ec = np.abs(W[t] - Wr).max(), np.abs(c[t] - cr).max()
        bW = wtol * np.abs(Wr).max()
        bc = ctol * np.abs(cr).max() + ctol * np.abs(Wr).max() / (kmin * lr)
        print('%s round %d: W err %.3g of %.3g, c err %.3g of %.3g' % (name, t, eW, bW, ec, bc))
        assert eW <= bW and ec <= bc
        assert np.abs(cr).max() > 0
    for got, want in ((tr, ref[0]), (tl, ref[1])):
        assert (np.abs(got.numpy() - want) <= ltol * np.maximum(1.0, np.abs(want))).all()
    assert np.abs(ta.numpy() - ref[2]).max() <= 100.0 / 40 + 1e-4          # one test sample of 40
    if SR.CASES[name]['sched'] is not None:
        assert all(np.array_equal(a, b) for a, b in zip(stats['participants'], SR.SCHED))


def test_rounds_0_and_1_against_fedavg(amd):
    """All variates are zero in round 0, so the round-0 model is FedAvg's (parallel clients) within
    the W tolerance; from round 1 on the correction is there: more than 1e-3 relative away."""
    sa, ss = {'trace': True}, {'trace': True}
    torch.manual_seed(SR.TORCH_SEED)
    amd.tools.FedAvg(*_data(), *_positional(), clients='parallel', stats=sa, verbose=False)
    torch.manual_seed(SR.TORCH_SEED)
    amd.tools.Scaffold(*_data(), *_positional(), stats=ss, verbose=False)
    Wa, Ws = sa['W_rounds'], ss['W_rounds']
    assert np.abs(Ws[0] - Wa[0]).max() <= W_TOL * np.abs(Wa[0]).max()
    assert np.abs(Ws[1] - Wa[1]).max() > 1e-3 * np.abs(Wa[1]).max()


def _fed(amd, algo='scaffold', sched=None, opts=None, **kw):
    torch.manual_seed(SR.TORCH_SEED)
    return amd.tools.Federation(algo, *_data(), None, *_positional(), 1e-3, 'parallel', verbose=False, options=opts,
                                participation=None if sched is None else [s.copy() for s in sched], **kw)


@pytest.mark.parametrize('sched', [None, SR.SCHED], ids=['full', 'sampled'])
@pytest.mark.parametrize('weighting', ['size', 'uniform'])
def test_variates_invariant_on_the_gpu(amd, sched, weighting):
    """|c - sum_j p_j c_j| <= (t+1)(N+4) 2^-24 (|c| + sum_j p_j |c_j|) elementwise on the GPU's own c
    and c_i after every round; clients that sat a round out keep their c_i bit for bit."""
    fed = _fed(amd, sched=sched, weighting=weighting)
    N = len(SR.SIZES)
    p = SR.weights(SR.SIZES, weighting)
    prev = fed.ci_var.cpu().numpy()
    assert not prev.any() and not fed.c_var.cpu().numpy().any()
    for t in range(SR.R):
        fed.round()
        torch.cuda.synchronize()
        c, ci = fed.c_var.cpu().numpy().astype(np.float64), fed.ci_var.cpu().numpy()
        mean = np.tensordot(p, ci.astype(np.float64), 1)
        bound = (t + 1) * (N + 4) * U * (np.abs(c) + np.tensordot(p, np.abs(ci.astype(np.float64)), 1))
        assert np.abs(c).max() > 0 and (np.abs(c - mean) <= bound).all(), (t, (np.abs(c - mean) / bound.max()).max())
        S = np.arange(N) if sched is None else sched[t]
        for j in range(N):
            if j in S:
                assert not np.array_equal(ci[j], prev[j])
            else:
                assert ci[j].tobytes() == prev[j].tobytes()
        prev = ci
    fed.results()


def test_set_scaffold_off_restores_fedavg(amd):
    """A FedAvg plan that ran one SCAFFOLD round, then set_scaffold(0): its next round, from the same
    round-start model, is bitwise the round of a plan that never had the setting."""
    opts = {'defer_eval': False, 'shuffle_chunk': 1}
    plain = _fed(amd, 'fedavg', opts=opts)
    plain.round()
    W0 = plain.W_g.clone()
    plain.round()
    sc = _fed(amd, 'fedavg', opts=opts)
    N, ld = len(SR.SIZES), sc.ld
    c = torch.full((SR.C, ld), 0.05, device=amd.dev)
    ci = torch.zeros(N, SR.C, ld, device=amd.dev)
    q, r, cs, _ = amd.tools.scaffold_round_coefficients(np.array(SR.SIZES), np.arange(N), SR.E, SR.B, SR.LR)
    sc.plan.set_scaffold(True, c, ci, torch.from_numpy(r).to(amd.dev), cs)
    sc.round()
    torch.cuda.synchronize()
    assert not torch.equal(W0, sc.W_g) and bool(ci.any()) and not bool((c == 0.05).all())
    sc.plan.set_scaffold(False)
    sc.W_g.copy_(W0)
    sc.round()
    torch.cuda.synchronize()
    assert torch.isfinite(plain.W_g).all() and torch.equal(plain.W_g, sc.W_g)
    assert torch.equal(plain.loss_hist[1], sc.loss_hist[1]) and torch.equal(plain.eval_hist[1], sc.eval_hist[1])


def test_deferred_evaluation_is_never_fused(amd):
    """A plan whose training form leaves CUs idle (the split form at N = 10) would fuse a deferred
    evaluation; with SCAFFOLD on it runs as a launch of its own before the next TRAIN: the same
    models bitwise and the same eval_hist to the 1e-12 relative the header states for deferral."""
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
            fed = amd.tools.Federation('scaffold', Xs, ys, Xt, yt, None, 'classification', C, D, 0.5, 1, 32, False, 0.0,
                                       False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False,
                                       options={'defer_eval': defer})
            for _ in range(R):
                fed.round()
            fed.results()
            assert fed.plan.eval_blocks() > 0                      # the plan itself could fuse
            runs[defer] = (stats['W_rounds'], stats['c_rounds'], fed.eval_hist.cpu().numpy().copy())
    assert np.array_equal(runs[False][0], runs[True][0]) and np.array_equal(runs[False][1], runs[True][1])
    assert np.isfinite(runs[True][2]).all()
    np.testing.assert_allclose(runs[True][2], runs[False][2], rtol=1e-12, atol=0)


def test_plan_setting_rejections(amd):
    E = amd.lib.FedsimError
    dev = amd.dev

    def bufs(fed):
        N, C, ld = fed.N, fed.C, fed.ld
        return (torch.zeros(C, ld, device=dev), torch.zeros(N, C, ld, device=dev), torch.ones(N, device=dev))

    def fed_of(clients='parallel', prox=False, B=SR.B, type='classification', opts=None):
        torch.manual_seed(3)
        Xs, ys, Xt, yt = _data()
        C = SR.C
        if type == 'regression':
            ys, yt, C = [y.float().reshape(-1, 1) for y in ys], yt.float().reshape(-1, 1), 1
        return amd.tools.Federation('fedprox' if prox else 'fedavg', Xs, ys, Xt, yt, None, type, C, SR.D, 0.1, 1, B,
                                    prox, 0.1, False, 0.0, 2, 1e-3, clients, verbose=False, options=opts)

    for kw in (dict(clients='sequential'), dict(type='regression'), dict(B=65), dict(prox=True)):
        fed = fed_of(**kw)
        with pytest.raises(E, match=r'\(-1\)'):
            fed.plan.set_scaffold(True, *bufs(fed))
    fed = fed_of()
    c, ci, r = bufs(fed)
    for args in ((None, ci, r), (c, None, r), (c, ci, None)):
        with pytest.raises(E, match=r'\(-1\)'):
            fed.plan.set_scaffold(True, *args)
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'\(-1\)'):                         # a nova mode other than 0
        fed.plan.set_scaffold(True, c, ci, r)
    fed.plan.set_nova(0)
    fed.plan.set_scaffold(True, c, ci, r)
    fed.plan.set_scaffold(True, c, ci, r, 0.5)                      # again while on: a round's new r and cs
    fed.plan.set_scaffold(False)
    # a plan that still holds a pending evaluation: the caller flushes first (the MSE plan's and the
    # fused plan's deferral; here a classification plan whose launch leaves CUs idle)
    tune = dict(train_form=1, split_mb=-1, split_dbuf=-1, split_pipe=-1, split_teams=-1)
    rs = np.random.RandomState(5)
    Xs = [torch.from_numpy(rs.normal(size=(20, 1024)).astype(np.float32) / 32) for _ in range(4)]
    ys = [torch.from_numpy(rs.randint(0, 4, size=20).astype(np.int64)) for _ in range(4)]
    with amd.lib.tuning(**tune):
        torch.manual_seed(3)
        pend = amd.tools.Federation('fedavg', Xs, ys, Xs[0], ys[0], None, 'classification', 4, 1024, 0.1, 1, 32, False,
                                    0.0, False, 0.0, 2, 1e-3, 'parallel', verbose=False, options={'defer_eval': True})
        assert pend.plan.eval_blocks() > 0
        pend.round()                                                # round 0's evaluation is now deferred
        c, ci, r = bufs(pend)
        with pytest.raises(E, match=r'\(-1\)'):
            pend.plan.set_scaffold(True, c, ci, r)
        pend.plan.eval_flush()
        pend.plan.set_scaffold(True, c, ci, r)
        pend.plan.set_scaffold(False)
        pend.round()
        pend.results()
    torch.cuda.synchronize()


def test_experiment_appends_scaffold_only_when_asked(amd, tmp_path):
    from fedamw_amd import experiment
    kw = dict(D=64, num_partitions=4, local_epoch=1, Round=3, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), save=False, synth=dict(n_train=700, n_test=120), verbose=False)
    six = experiment.run('a9a', algos=('FedAvg',), **kw)
    out = experiment.run('a9a', algos=('FedAvg', 'Scaffold'), **kw)
    assert six['name'] == experiment.NAMES and out['name'] == experiment.NAMES + ['Scaffold']
    for k in ('train_loss', 'test_loss', 'test_acc'):
        assert out[k].shape == (7, 3, 1) and np.isfinite(out[k][[3, 6]]).all() and np.isnan(out[k][[0, 1, 2, 4, 5]]).all()
        assert np.array_equal(out[k][3], six[k][3])
    assert not np.array_equal(out['test_loss'][6], out['test_loss'][3])
    both = experiment.run('a9a', algos=('FedAvg', 'FedNova', 'Scaffold'), **kw)
    assert both['name'] == experiment.NAMES + ['FedNova', 'Scaffold']
    for k in ('train_loss', 'test_loss', 'test_acc'):         # (Scaffold runs last: it cannot move the others' draws)
        assert both[k].shape == (8, 3, 1) and np.array_equal(both[k][3], six[k][3]) and np.isfinite(both[k][[6, 7]]).all()


def test_python_rejections(amd):
    a = _data()
    with pytest.raises(ValueError, match='prox'):
        amd.tools.Scaffold(*a, 'classification', SR.C, SR.D, 0.5, 2, 8, True, 0.1, False, 0.0, 2, verbose=False)
    ya = ([y.float().reshape(-1, 1) for y in a[1]], a[3].float().reshape(-1, 1))
    with pytest.raises(ValueError, match='classification'):
        amd.tools.Scaffold(a[0], ya[0], a[2], ya[1], 'regression', 1, SR.D, 0.5, 2, 8, False, 0.1, False, 0.0, 2,
                           verbose=False)
    with pytest.raises(ValueError, match='batch_size'):
        amd.tools.Scaffold(*a, 'classification', SR.C, SR.D, 0.5, 2, 128, False, 0.1, False, 0.0, 2, verbose=False)

"""q-FedAvg at drop-in level (the FedOpt drop-in test's federation: N = 6 ragged clients, D = 64, C = 3 and
C = 1 for regression, E = 2, B = 8, R = 3): the exact wiring of the local evaluation, fs_qffl_coef and
fs_aggregate_qffl into the round on the GPU's own buffers, ``tools.QFedAvg`` against
tests/qffl_restatement.py on its eight cases and against ``FedAvg`` at q = 0, the plan setting and its
rejections, and the experiment driver.

Tolerances of the restatement comparison are tests/test_gpu_fedopt.py's: the q-FFL step is no longer
than the longest client update (H >= L U), so a round adds at most one training-kernel tolerance: W of
round t within max((t + 1) 2e-5 max|W|, 2 delta_W max|W|), the three returns and the clients' losses
within max(1e-5 max(1, |.|), 2 delta max(1, |.|)), the deltas recorded in tests/golden/qffl_drift.json
(<= 3e-7, so the first terms hold)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO
from tests import qffl_restatement as QR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_TOL, LOSS_TOL = 2e-5, 1e-5
U = 2.0 ** -24
N = len(QR.SIZES)


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    from fedamw_amd.functions import tools
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, tools=tools, dev=torch.device('cuda')))


def _data(regression=False):
    Xs, ys, Xt, yt = QR.case_data(regression)
    if regression:
        ys, yt = [y.reshape(-1, 1) for y in ys], yt.reshape(-1, 1)
    return ([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys], torch.from_numpy(Xt),
            torch.from_numpy(yt))


def _positional(name=None):
    type, nc, bs, prox = QR.case_args(name) if name else ('classification', QR.C, QR.B, False)
    return (type, nc, QR.D, QR.LR, QR.E, bs, prox, QR.MU, True, QR.LAM, QR.R)


def _fed(amd, algo='qfedavg', q=1.0, weighting='size', participation=None, opts=None, clients='parallel', name=None):
    torch.manual_seed(QR.TORCH_SEED)
    kw = dict(weighting=weighting, qffl=dict(q=q)) if algo == 'qfedavg' else {}
    reg = name is not None and QR.CASES[name].get('type') == 'regression'
    return amd.tools.Federation(algo, *_data(reg), None, *_positional(name), 1e-3, clients, verbose=False, options=opts,
                                participation=participation, sample_seed=QR.SAMPLE_SEED, **kw)


def _same(got, ref, what):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    bad = np.flatnonzero(got != ref)
    assert got.tobytes() == ref.tobytes(), (what, len(bad), got[bad[:4]], ref[bad[:4]])


def _drive(amd, q, weighting, participation, defer):
    """Federation.round() by hand.  After every round, from the GPU's own buffers: F is bitwise
    LocalEvaluator.run on the round's starting model; u and g are numpy's from that F within 2^-22;
    S is bitwise the numpy left fold of W_out with the GPU's u (M < 16); n within 16 * 2^-24 of the
    exact norms; and the numpy finish on the GPU's n, S, u, g is hc and the new W_g bit for bit."""
    fed = _fed(amd, q=q, weighting=weighting, participation=participation, opts={'defer_eval': defer})
    p32 = QR.client_weights(QR.SIZES, weighting)
    Ls = QR.lipschitz_schedule(QR.LR, QR.R)
    le = amd.engine.LocalEvaluator(fed.feats, fed.C)
    for t in range(QR.R):
        x_dev = fed.W_g.clone()
        x = x_dev.cpu().numpy()
        fed.round()
        torch.cuda.synchronize()
        S_ids = np.arange(N) if fed.sched is None else fed.sched[t]
        M = len(S_ids)
        F = fed.qf_F[t].cpu().numpy()
        _same(F, le.run(x_dev, 0, torch.empty(N, 2, dtype=torch.float64, device=amd.dev)).cpu().numpy(), (t, 'F'))
        assert np.isfinite(F).all() and (F[:, 0] > 0).all()
        u, g = fed.qf_u[:M].cpu().numpy(), fed.qf_g[:M].cpu().numpy()
        ru, rg = QR.coefficients(F[S_ids, 0], p32[S_ids], q, Ls[t], np.float64)
        if q == 0:
            _same(u, p32[S_ids], (t, 'u = p'))
            assert not g.any()
        else:
            assert (np.abs(u - ru) <= 2.0 ** -22 * ru).all() and (np.abs(g - rg) <= 2.0 ** -22 * rg).all()
        W_out = fed.trainer.W_out.cpu().numpy().reshape(N, -1)
        rows = [W_out[j] for j in S_ids]
        Sg, ng, hc = fed.qf_S.cpu().numpy(), fed.qf_n[t][:M].cpu().numpy(), fed.qf_hc[t].cpu().numpy()
        _same(Sg, FO.delta(rows, u, x.reshape(-1)), (t, 'S'))
        d = (np.stack(rows) - x.reshape(-1)).astype(np.float32).astype(np.float64)
        exact = (d * d).sum(1)
        assert (np.abs(ng - exact) <= 16 * U * exact).all() and (exact > 0).all()
        ref, H, coef = QR.finish(Sg.reshape(-1), ng, u, g, Ls[t], x.reshape(-1))
        assert hc[0] == H and hc[1] == float(coef) and coef > 0
        x2 = fed.W_g.cpu().numpy()
        _same(x2, ref, (t, 'W_g'))
        assert np.isfinite(x2).all() and not np.array_equal(x2, x) and not x2[:, QR.D:].any()
    res = fed.results()
    return fed.eval_hist.cpu().numpy().copy(), [r.numpy().copy() for r in res], fed.W_g.cpu().numpy(), fed


@pytest.mark.parametrize('q,weighting', [(0.0, 'size'), (1.0, 'uniform'), (5.0, 'size')])
def test_exact_wiring_on_the_gpus_own_buffers(amd, q, weighting):
    """With participation = 0.5, and with defer_eval on, where the test metrics must be the undeferred
    run's exactly (the finaliser's path)."""
    _drive(amd, q, weighting, QR.PARTICIPATION, False)
    plain = _drive(amd, q, weighting, None, False)
    deferred = _drive(amd, q, weighting, None, True)
    _same(deferred[2], plain[2], 'W_g')
    assert np.isfinite(plain[0]).all() and np.array_equal(deferred[0], plain[0])
    for a, b in zip(deferred[1], plain[1]):
        assert np.array_equal(a, b)


def test_stats(amd):
    """client_loss [R, N] is the F of each round's starting model (bitwise the device history),
    update_norms [R, N] is NaN exactly where a client was not sampled, qffl_coef [R, 2] = (H, coef)."""
    stats = {}
    torch.manual_seed(QR.TORCH_SEED)
    amd.tools.QFedAvg(*_data(), *_positional(), q=1.0, stats=stats, verbose=False, participation=QR.PARTICIPATION,
                      sample_seed=QR.SAMPLE_SEED)
    cl, un, hc = stats['client_loss'], stats['update_norms'], stats['qffl_coef']
    assert cl.shape == (QR.R, N) and cl.dtype == np.float64 and np.isfinite(cl).all() and (cl > 0).all()
    assert un.shape == (QR.R, N) and hc.shape == (QR.R, 2) and (hc > 0).all()
    sched = QR.case_sched('q1_uniform_sampled')
    for t, S in enumerate(stats['participants']):
        assert np.array_equal(S, sched[t]) and len(S) == 3
        keep = np.zeros(N, bool)
        keep[S] = True
        assert np.isfinite(un[t][keep]).all() and (un[t][keep] > 0).all() and np.isnan(un[t][~keep]).all()


def _bounds(name):
    with open(os.path.join(ROOT, 'tests', 'golden', 'qffl_drift.json')) as f:
        d = json.load(f)[name]
    return d['delta_W'], max(LOSS_TOL, 2 * d['delta_loss']), max(LOSS_TOL, 2 * d['delta_F'])


@pytest.mark.parametrize('name', sorted(QR.CASES))
def test_dropin_matches_the_restatement(amd, name):
    k = QR.CASES[name]
    reg = k.get('type') == 'regression'
    ref = QR.run_case(name)
    rng_ref = torch.empty(4, dtype=torch.int64).random_().numpy()
    stats = {'trace': True}
    torch.manual_seed(QR.TORCH_SEED)
    tr, tl, ta = amd.tools.QFedAvg(*_data(reg), *_positional(name), q=k['q'], weighting=k['weighting'], stats=stats,
                                   verbose=False, participation=QR.PARTICIPATION if k['sampled'] else None,
                                   sample_seed=QR.SAMPLE_SEED)
    np.testing.assert_array_equal(torch.empty(4, dtype=torch.int64).random_().numpy(), rng_ref)
    dW, ltol, ftol = _bounds(name)
    C = 1 if reg else QR.C
    W = stats['W_rounds']
    assert W.shape == ref[3]['W'].shape == (QR.R, C, QR.D)
    for t in range(QR.R):
        Wr = ref[3]['W'][t]
        err = np.abs(W[t] - Wr).max()
        bound = max((t + 1) * W_TOL, 2 * dW) * np.abs(Wr).max()
        print('%s round %d: W err %.3g of %.3g' % (name, t, err, bound))
        assert err <= bound
    for what, got, want in (('train_loss', tr, ref[0]), ('test_loss', tl, ref[1]), ('test_acc', ta, ref[2])):
        err = np.abs(got.numpy() - want)
        print('%s %s: max err %.3g' % (name, what, (err / np.maximum(1.0, np.abs(want))).max()))
        assert (err <= ltol * np.maximum(1.0, np.abs(want))).all(), what
    errF = np.abs(stats['client_loss'] - ref[3]['F']) / np.maximum(1.0, np.abs(ref[3]['F']))
    print('%s client_loss: max err %.3g; H rel err %.3g' % (
        name, errF.max(), (np.abs(stats['qffl_coef'][:, 0] - ref[3]['hc'][:, 0]) / ref[3]['hc'][:, 0]).max()))
    assert (errF <= ftol).all()
    assert np.array_equal(np.isnan(stats['update_norms']), np.isnan(ref[3]['n']))
    if k['sampled']:
        assert all(np.array_equal(a, b) for a, b in zip(stats['participants'], QR.case_sched(name)))


@pytest.mark.parametrize('participation', [None, QR.PARTICIPATION])
def test_q0_is_fedavg(amd, participation):
    """QFedAvg(q=0) against FedAvg(clients='parallel'), the same seeds and the same participation: per
    round within the restatement cases' bound; round 0 trains from the same model, so its train_loss
    is FedAvg's bitwise; and the generator ends where FedAvg leaves it."""
    sa, sb = {'trace': True}, {'trace': True}
    torch.manual_seed(QR.TORCH_SEED)
    a = amd.tools.FedAvg(*_data(), *_positional(), clients='parallel', stats=sa, verbose=False,
                         participation=participation, sample_seed=QR.SAMPLE_SEED)
    ra = torch.empty(4, dtype=torch.int64).random_().numpy()
    torch.manual_seed(QR.TORCH_SEED)
    b = amd.tools.QFedAvg(*_data(), *_positional(), q=0.0, stats=sb, verbose=False, participation=participation,
                          sample_seed=QR.SAMPLE_SEED)
    rb = torch.empty(4, dtype=torch.int64).random_().numpy()
    np.testing.assert_array_equal(ra, rb)
    assert float(a[0][0]) == float(b[0][0])
    dW = _bounds('q0_size_full' if participation is None else 'q0_size_sampled')[0]
    for t in range(QR.R):
        Wr = sa['W_rounds'][t]
        err = np.abs(sb['W_rounds'][t] - Wr).max()
        bound = max((t + 1) * W_TOL, 2 * dW) * np.abs(Wr).max()
        print('q = 0 vs FedAvg round %d: W err %.3g of %.3g' % (t, err, bound))
        assert err <= bound
    for x, y in zip(a, b):
        assert (np.abs(x.numpy() - y.numpy()) <= LOSS_TOL * np.maximum(1.0, np.abs(x.numpy()))).all()


def test_deferred_evaluation_rides_across_the_qffl_aggregate(amd):
    """The split form at N = 10 leaves CUs idle: round t's evaluation fuses into round t+1's TRAIN
    launch and its finaliser rides on fs_aggregate_qffl's pass.  Same models and coefficients bitwise,
    the same eval_hist to the 1e-12 relative the header states for a fused deferral."""
    tune = dict(train_form=1, split_mb=-1, split_dbuf=-1, split_pipe=-1, split_teams=-1)
    C, Nc, R, D, n_t = 10, 10, 3, 1024, 16 * 16 + 5
    rs = np.random.RandomState(17)
    sizes = rs.randint(8, 41, size=Nc)
    Xs = [torch.from_numpy((np.cos(rs.normal(size=(n, D))) / np.sqrt(D)).astype(np.float32)) for n in sizes]
    ys = [torch.from_numpy(rs.randint(0, C, size=n).astype(np.int64)) for n in sizes]
    Xt = torch.from_numpy((np.cos(rs.normal(size=(n_t, D))) / np.sqrt(D)).astype(np.float32))
    yt = torch.from_numpy(rs.randint(0, C, size=n_t).astype(np.int64))
    runs = {}
    with amd.lib.tuning(**tune):
        for defer in (False, True):
            stats = {'trace': True}
            torch.manual_seed(11)
            fed = amd.tools.Federation('qfedavg', Xs, ys, Xt, yt, None, 'classification', C, D, 0.5, 1, 32, False, 0.0,
                                       False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False,
                                       options={'defer_eval': defer}, qffl=dict(q=2.0))
            for _ in range(R):
                fed.round()
            fed.results()
            assert fed.plan.eval_blocks() > 0
            runs[defer] = (stats['W_rounds'], stats['qffl_coef'], stats['update_norms'], stats['client_loss'],
                           fed.eval_hist.cpu().numpy().copy())
    for k in range(4):
        assert np.array_equal(runs[False][k], runs[True][k])
    assert np.isfinite(runs[True][4]).all()
    np.testing.assert_allclose(runs[True][4], runs[False][4], rtol=1e-12, atol=0)


def _qffl_bufs(amd, fed):
    dev = amd.dev
    return dict(g=torch.zeros(fed.N, device=dev), S=torch.zeros(fed.C, fed.ld, device=dev),
                n=torch.zeros(fed.N, dtype=torch.float64, device=dev), hc=torch.zeros(2, dtype=torch.float64, device=dev),
                nws=fed.agg.qffl_ws())


def test_off_restores_the_plain_aggregate(amd):
    """A FedAvg plan that ran one round with q-FedAvg set, then set_qffl(False): its next round, from
    the same round-start model, is bitwise the round of a plan that never had the setting."""
    opts = {'defer_eval': False, 'shuffle_chunk': 1}
    plain = _fed(amd, 'fedavg', opts=opts)
    plain.round()
    W0 = plain.W_g.clone()
    plain.round()
    so = _fed(amd, 'fedavg', opts=opts)
    b = _qffl_bufs(amd, so)
    b['g'].fill_(0.3)
    so.plan.set_qffl(True, b['g'], 2.0, b['S'], b['n'], b['hc'], b['nws'])
    so.round()
    torch.cuda.synchronize()
    assert not torch.equal(W0, so.W_g) and bool(b['S'].any()) and bool((b['n'] > 0).all()) and bool((b['hc'] > 0).all())
    so.plan.set_qffl(False)
    so.W_g.copy_(W0)
    so.round()
    torch.cuda.synchronize()
    assert torch.isfinite(plain.W_g).all() and torch.equal(plain.W_g, so.W_g)
    assert torch.equal(plain.loss_hist[1], so.loss_hist[1]) and torch.equal(plain.eval_hist[1], so.eval_hist[1])


def test_rejections(amd, monkeypatch):
    """The four plan settings exclude each other; chained plans and bad arguments are refused; prox,
    regression and large batches are allowed."""
    E = amd.lib.FedsimError
    sc = FO.scalars(**FO.SERVER)
    chained = _fed(amd, 'fedavg', clients='sequential')
    b = _qffl_bufs(amd, chained)
    with pytest.raises(E, match=r'\(-1\)'):
        chained.plan.set_qffl(True, b['g'], 2.0, b['S'], b['n'], b['hc'], b['nws'])
    fed = _fed(amd, 'fedavg')
    b = _qffl_bufs(amd, fed)
    args = lambda **kw: [{**b, 'Lc': 2.0, **kw}[k] for k in ('g', 'Lc', 'S', 'n', 'hc', 'nws')]   # noqa: E731
    for kw in (dict(g=None), dict(S=None), dict(n=None), dict(hc=None), dict(nws=None), dict(Lc=0.0), dict(Lc=-1.0),
               dict(Lc=float('inf')), dict(S=fed.W_g), dict(nws=b['nws'][:max(1, b['nws'].numel() // 2 - 1)])):
        with pytest.raises(E, match=r'\(-1\)'):
            fed.plan.set_qffl(True, *args(**kw))
    m, v = torch.zeros(fed.C, fed.ld, device=amd.dev), torch.full((fed.C, fed.ld), 0.01, device=amd.dev)
    c, ci, r = torch.zeros(fed.C, fed.ld, device=amd.dev), torch.zeros(fed.N, fed.C, fed.ld, device=amd.dev), \
        torch.ones(fed.N, device=amd.dev)
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'\(-1\)'):                              # a nova mode other than 0
        fed.plan.set_qffl(True, *args())
    fed.plan.set_nova(0)
    fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'\(-1\)'):                              # SCAFFOLD on
        fed.plan.set_qffl(True, *args())
    fed.plan.set_scaffold(False)
    fed.plan.set_server_opt('adam', m, v, *sc)
    with pytest.raises(E, match=r'\(-1\)'):                              # a server-optimizer rule
        fed.plan.set_qffl(True, *args())
    fed.plan.set_server_opt(0)
    fed.plan.set_qffl(True, *args())
    fed.plan.set_qffl(True, *args(Lc=20.0))                              # callable again while on
    with pytest.raises(E, match=r'\(-1\)'):                              # and the other three refuse in turn
        fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    with pytest.raises(E, match=r'\(-1\)'):
        fed.plan.set_scaffold(True, c, ci, r)
    with pytest.raises(E, match=r'\(-1\)'):
        fed.plan.set_server_opt('adam', m, v, *sc)
    fed.plan.set_nova(0)                                                 # (turning the others off is not a change)
    fed.plan.set_server_opt(0)
    fed.plan.set_qffl(False)
    fed.plan.set_nova(amd.lib.NOVA_UPDATES)
    fed.plan.set_nova(0)
    fed.plan.set_server_opt('adam', m, v, *sc)
    fed.plan.set_server_opt(0)
    with pytest.raises(ValueError, match='parallel'):
        _fed(amd, 'qfedavg', clients='sequential')
    for kw in (dict(q=-1.0), dict(lipschitz=0.0), dict(weighting='loss')):
        with pytest.raises(ValueError):
            amd.tools.QFedAvg(*_data(), *_positional(), verbose=False, **kw)
    monkeypatch.setattr(amd.tools.dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='rank'):
        amd.tools.QFedAvg(*_data(), *_positional(), verbose=False)
    monkeypatch.undo()
    torch.cuda.synchronize()


def test_lipschitz_keyword_and_large_batches(amd):
    """A given Lipschitz estimate replaces 1 / lr_t (a larger L with q > 0 shortens the step), and a
    batch size above 64 trains on the wide form as FedAvg's."""
    out = {}
    for lip in (None, 50.0):
        st = {'trace': True}
        torch.manual_seed(QR.TORCH_SEED)
        amd.tools.QFedAvg(*_data(), 'classification', QR.C, QR.D, QR.LR, QR.E, 80, False, QR.MU, True, QR.LAM, QR.R,
                          q=2.0, lipschitz=lip, stats=st, verbose=False)
        out[lip] = st
        assert np.isfinite(st['W_rounds']).all() and (st['qffl_coef'] > 0).all()
    assert np.array_equal(out[None]['client_loss'][0], out[50.0]['client_loss'][0])
    assert np.array_equal(out[None]['update_norms'][0], out[50.0]['update_norms'][0])
    assert out[50.0]['qffl_coef'][0, 1] < out[None]['qffl_coef'][0, 1]


def test_experiment_appends_qfedavg_only_when_asked(amd, tmp_path):
    from fedamw_amd import experiment
    assert experiment.EXTRA_FAIR == ['QFedAvg']
    kw = dict(D=64, num_partitions=4, local_epoch=1, Round=3, n_repeats=1, alpha_Dirk=0.5, data_dir='/nonexistent/',
              result_dir=str(tmp_path), save=False, synth=dict(n_train=700, n_test=120), verbose=False)
    six = experiment.run('a9a', algos=('FedAvg',), **kw)
    out = experiment.run('a9a', algos=('FedAvg', 'QFedAvg'), **kw)
    assert six['name'] == experiment.NAMES and out['name'] == experiment.NAMES + ['QFedAvg']
    for k in ('train_loss', 'test_loss', 'test_acc'):
        assert out[k].shape == (7, 3, 1) and np.isfinite(out[k][[3, 6]]).all() and np.isnan(out[k][[0, 1, 2, 4, 5]]).all()
        assert np.array_equal(out[k][3], six[k][3])
    assert not np.array_equal(out['test_loss'][6], out['test_loss'][3])
    fair = experiment.run('a9a', algos=('QFedAvg',), qffl_q=5.0, qffl_weighting='uniform', **kw)
    assert not np.array_equal(fair['test_loss'][6], out['test_loss'][6])
    both = experiment.run('a9a', algos=('FedAdam', 'QFedAvg'), participation=0.5, **kw)
    assert both['name'] == experiment.NAMES + ['FedAdam', 'QFedAvg'] and both['participants'][7] is not None

"""DPFedAvg at drop-in level (the N = 14 ragged clients of the Krum, robust, RFA and top-k round tests, D = 32,
C = 3 and C = 1 for regression, E = 2, B = 8, R = 3): ``clip=inf, noise_multiplier=0`` against
``tools.FedAvgM(server_lr=1.0, beta1=0.0)`` bit for bit; the clip as a bound on every round's step under a
sign-flip attack and the dropped NaN rows; the noise's reproducibility and its exact form after one round; the
adaptive clip's trajectory against tests/dp_restatement.py on the device's own norms; the stats."""
import numpy as np
import pytest
import torch

from tests import dp_restatement as DP
from tests import krum_restatement as KR

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


def _positional(regression=False, prox=False, batch=KR.B, rounds=R):
    return ('regression' if regression else 'classification', 1 if regression else KR.C, KR.D, KR.LR, KR.E, batch,
            prox, KR.MU, True, KR.LAM, rounds)


def _dropin(amd, regression=False, participation=None, rounds=R, prox=False, batch=KR.B, options=OPTS, **kw):
    stats = {'trace': True}
    torch.manual_seed(KR.TORCH_SEED)
    res = amd.tools.DPFedAvg(*_data(regression), *_positional(regression, prox, batch, rounds), stats=stats,
                             verbose=False, options=options, participation=participation,
                             sample_seed=KR.SAMPLE_SEED, **kw)
    gen = torch.empty(4, dtype=torch.int64).random_().numpy()
    return [r.numpy().copy() for r in res], stats, gen


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype)
    ok = (got == ref) | (np.isnan(got) & np.isnan(ref))
    assert ok.all() and (np.signbit(got) == np.signbit(ref))[~np.isnan(got)].all(), (what, got, ref)


def _W(stats):
    return stats['W_global'].cpu().numpy()


def _initial_model(amd):
    """x_0 [C, D]: what a federation of the same seed starts from."""
    torch.manual_seed(KR.TORCH_SEED)
    fed = amd.tools.Federation('fedavg', *_data(), None, *_positional(), 1e-3, 'parallel', verbose=False, options=OPTS)
    return fed.W_g[:, :KR.D].cpu().numpy().copy()


@pytest.mark.parametrize('participation', [None, PART])
@pytest.mark.parametrize('regression', [False, True])
def test_no_clip_no_noise_is_fedavgm_without_momentum(amd, participation, regression):
    res, stats, gen = _dropin(amd, regression=regression, participation=participation, clip=float('inf'),
                              noise_multiplier=0.0, weighting='size')
    torch.manual_seed(KR.TORCH_SEED)
    st = {'trace': True}
    ref = amd.tools.FedAvgM(*_data(regression), *_positional(regression), server_lr=1.0, beta1=0.0, stats=st,
                            verbose=False, options=OPTS, participation=participation, sample_seed=KR.SAMPLE_SEED)
    gen2 = torch.empty(4, dtype=torch.int64).random_().numpy()
    _same(_W(stats), _W(st), 'W_global')
    for a, b, what in zip(res, ref, ('train_loss', 'test_loss', 'test_acc')):
        _same(a, b.numpy(), what)
    assert np.array_equal(gen, gen2)                     # the global generator is consumed alike
    assert (stats['dp_clip'] == np.inf).all() and (stats['dp_sigma'] == 0).all()
    assert (stats['dp_clipped'] == 0).all() and (stats['dp_dropped'] == 0).all()


def test_clip_bounds_every_round_step_under_sign_flip(amd):
    S = 0.05
    byz = dict(fraction=0.2, attack='sign_flip', scale=100)
    _, stats, _ = _dropin(amd, clip=S, noise_multiplier=0.0, byzantine=byz)
    hist = stats['W_rounds'].astype(F64)                 # [R, C, D]: the model after every round
    assert hist.shape[0] == R
    prev = _initial_model(amd).astype(F64)
    for t in range(R):
        step = np.sqrt(np.sum((hist[t] - prev) ** 2))
        assert step <= S * (1 + 1e-5), (t, step)
        prev = hist[t]
    # the bound was at work: at the first round's learning rate the corrupted updates, at least, are clipped
    # (the rate falls by 10 and by 1000 in rounds 1 and 2, and the updates with it)
    assert len(stats['byzantine_ids']) == 2 and stats['dp_clipped'][0] >= 2
    assert (stats['dp_norms'][0, stats['byzantine_ids']] > S).all()


def test_nan_attack_is_dropped(amd):
    byz = dict(fraction=0.2, attack='nan')
    res, stats, _ = _dropin(amd, clip=0.5, noise_multiplier=0.0, byzantine=byz)
    assert np.isfinite(_W(stats)).all() and all(np.isfinite(r).all() for r in res)
    assert (stats['dp_dropped'] == len(stats['byzantine_ids'])).all() and len(stats['byzantine_ids']) == 2
    assert np.isnan(stats['dp_norms'][:, stats['byzantine_ids']]).all()


def test_noise_is_reproducible_and_seeded(amd):
    kw = dict(clip=0.5, noise_multiplier=1.0)
    a, sa, _ = _dropin(amd, noise_seed=3, **kw)
    b, sb, _ = _dropin(amd, noise_seed=3, **kw)
    c, sc, _ = _dropin(amd, noise_seed=4, **kw)
    _same(_W(sa), _W(sb), 'the same seed')
    for u, v in zip(a, b):
        _same(u, v, 'the same seed')
    assert not np.array_equal(_W(sa), _W(sc))
    assert (sa['dp_sigma'] == 1.0 * 0.5 * float(F32(1.0 / N))).all()


@pytest.mark.parametrize('regression', [False, True])
def test_one_round_of_noise_is_the_field_added_once(amd, regression):
    S, z, seed = 0.5, 0.8, 2 ** 32 + 5
    _, s0, _ = _dropin(amd, regression=regression, rounds=1, clip=S, noise_multiplier=0.0)
    _, s1, _ = _dropin(amd, regression=regression, rounds=1, clip=S, noise_multiplier=z, noise_seed=seed)
    x0, x1 = _W(s0), _W(s1)                              # [C, D]
    C, D = x0.shape
    ld = amd.engine.pad_ld(D)
    g = torch.empty(C * ld, device=amd.dev)
    amd.engine.Aggregator(1, C, ld, amd.dev).dp_noise(seed, 0, g)
    g = g.cpu().numpy().reshape(C, ld)[:, :D]
    sigma = s1['dp_sigma'][0]
    assert sigma == (z * S) * float(F32(1.0 / N))
    _same(x1, (x0 + (F32(sigma) * g).astype(F32)).astype(F32), 'x_1(z) = fl(x_1(0) + fl(sigma g))')
    # and the restatement's field is the device's, to the neighbouring float
    ref = DP.noise(seed, 0, C * ld).reshape(C, ld)[:, :D]
    assert (np.abs(g.astype(F64) - ref) <= np.spacing(np.abs(ref))).all()


@pytest.mark.parametrize('participation', [None, PART])
def test_adaptive_clip_follows_the_restatement(amd, participation):
    ad = dict(quantile=0.5, lr=0.4, count_noise=0.5)
    S0, seed = 0.02, 9
    _, stats, _ = _dropin(amd, participation=participation, clip=S0, noise_multiplier=0.3, noise_seed=seed,
                          adaptive=ad)
    clip = stats['dp_clip']
    assert clip[0] == S0 and len(set(clip)) == R
    for t in range(R - 1):
        r = stats['dp_norms'][t]
        r = r[~np.isnan(r)]
        b = float(np.sum(r <= clip[t]))
        assert stats['dp_clipped'][t] == len(r) - b
        nxt = DP.clip_next(clip[t], b, len(r), ad, seed, t)
        ulp = abs(int(np.array(nxt).view(np.int64)) - int(np.array(clip[t + 1]).view(np.int64)))
        assert ulp <= 4, (t, nxt, clip[t + 1])
    assert (stats['dp_sigma'] == (0.3 * clip) * float(F32(1.0 / len(r)))).all()


def test_participation_norms_are_nan_off_the_sample(amd):
    _, stats, _ = _dropin(amd, participation=PART, clip=0.5, noise_multiplier=0.5)
    part = stats['participants']
    assert len(part) == R
    for t in range(R):
        on = np.zeros(N, bool)
        on[np.asarray(part[t])] = True
        assert np.isnan(stats['dp_norms'][t][~on]).all() and np.isfinite(stats['dp_norms'][t][on]).all(), t
        assert 0 < on.sum() < N


@pytest.mark.parametrize('kw', [dict(), dict(prox=True), dict(batch=80), dict(regression=True, weighting='size')])
def test_stats_shapes_and_dtypes(amd, kw):
    res, stats, _ = _dropin(amd, clip=0.3, noise_multiplier=0.5, **kw)
    for key, shape in (('dp_clip', (R,)), ('dp_sigma', (R,)), ('dp_norms', (R, N)), ('dp_clipped', (R,)),
                       ('dp_dropped', (R,))):
        a = stats[key]
        assert isinstance(a, np.ndarray) and a.dtype == F64 and a.shape == shape, (key, a.dtype, a.shape)
    assert (stats['dp_clip'] == 0.3).all() and np.isfinite(stats['dp_norms']).all()
    assert ((stats['dp_clipped'] >= 0) & (stats['dp_clipped'] <= N)).all() and (stats['dp_dropped'] == 0).all()
    assert all(np.isfinite(r).all() and r.shape == (R,) for r in res)


def test_plan_setting_excludes_the_other_aggregates(amd):
    torch.manual_seed(KR.TORCH_SEED)
    fed = amd.tools.Federation('fedavg', *_data(), None, *_positional(), 1e-3, 'parallel', verbose=False,
                               options=OPTS)
    dev = amd.dev
    c = torch.zeros(N, device=dev)
    r = torch.zeros(N, dtype=torch.float64, device=dev)
    st = torch.zeros(amd.engine.DP_STATE, dtype=torch.float64, device=dev)
    ws = fed.agg.dp_ws()
    fed.plan.set_dp(True, 1.0, 1.0, 0, True, None, None, c, r, st, ws, cols=KR.D)
    with pytest.raises(RuntimeError, match='DP-FedAvg'):
        fed.plan.set_topk(True, 4, None, torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match='DP-FedAvg'):
        fed.plan.set_robust(True, 'median', 0.0)
    fed.plan.set_dp(False)
    fed.plan.set_topk(True, 4, None, torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match='FedTopK'):
        fed.plan.set_dp(True, 1.0, 1.0, 0, True, None, None, c, r, st, ws, cols=KR.D)
    fed.plan.set_topk(False)
    for bad in (dict(clip=0.0), dict(clip=float('nan')), dict(z=-1.0), dict(z=float('inf')),
                dict(clip=float('inf')), dict(cols=0), dict(cols=fed.ld + 1)):
        a = dict(clip=1.0, z=1.0, cols=KR.D)
        a.update(bad)
        with pytest.raises(RuntimeError):
            fed.plan.set_dp(True, a['clip'], a['z'], 0, True, None, None, c, r, st, ws, cols=a['cols'])

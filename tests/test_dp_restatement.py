"""tests/dp_restatement.py on the CPU: Philox4x32-10's known answers, the moments of the noise field, the
properties of DP-FedAvg's rule, the adaptive clip's fixed point, DPFedAvg's keyword checks and the driver's flags.
No GPU."""
import numpy as np
import pytest

from tests import dp_restatement as DP
from tests import fedopt_restatement as FO

F32 = np.float32
F64 = np.float64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def rows(M, L, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(L).astype(F32)
    W = (x[None, :] + scale * rs.standard_normal((M, L))).astype(F32)
    q = rs.dirichlet(np.full(M, 2.0)).astype(F32)
    return W, x, q


# ---- Philox4x32-10: the Random123 known-answer vectors -------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize('counter,key,want', KAT)
def test_philox_known_answers(counter, key, want):
    got = DP.philox4x32_10(counter, key)
    assert tuple(int(w[0]) for w in got) == want


def test_philox_is_vectorised_over_the_counter():
    j = np.arange(7, dtype=np.uint64)
    w = DP.philox4x32_10((j, 5, 0, 0), (9, 1))
    for i in range(7):
        one = DP.philox4x32_10((i, 5, 0, 0), (9, 1))
        assert [int(a[i]) for a in w] == [int(a[0]) for a in one]


def test_seed_key_split():
    assert DP.seed_key(0) == (0, 0) and DP.seed_key(2 ** 32 + 5) == (5, 1) and DP.seed_key(2 ** 64 - 1) == (2 ** 32 - 1,) * 2


# ---- the field g ---------------------------------------------------------------------------------------------
def test_noise_moments():
    n = 1 << 20
    g = DP.noise(0, 0, n).astype(F64)
    assert g.dtype == F64 and len(g) == n
    mean, var = g.mean(), g.var()
    assert abs(mean) <= 5.0 / np.sqrt(n), mean
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n), var
    assert np.abs(g).max() <= 6.77 and DP.G_MAX <= 6.77


def test_noise_extremes_are_finite():
    # u = (w + 0.5) 2^-32 is never 0 or 1: the smallest and the largest word give finite normals
    lo, hi = np.array([0], np.uint32), np.array([0xffffffff], np.uint32)
    for w0 in (lo, hi):
        for w1 in (lo, hi):
            a, b = DP.pair(w0, w1)
            assert np.isfinite(a).all() and np.isfinite(b).all() and abs(a[0]) <= 6.77 and abs(b[0]) <= 6.77
    assert abs(DP.pair(lo, lo)[0][0] - DP.G_MAX) < 1e-6


def test_noise_field_does_not_depend_on_the_length():
    a, b = DP.noise(3, 7, 64), DP.noise(3, 7, 4096)
    assert np.array_equal(bits(a), bits(b[:64]))


def test_noise_differs_by_round_seed_and_stream():
    base = DP.noise(1, 2, 256)
    for other in (DP.noise(1, 3, 256), DP.noise(2, 2, 256), DP.noise(1, 2, 256, stream=1), DP.noise(2 ** 32 + 1, 2, 256)):
        assert not np.array_equal(bits(base), bits(other))
    assert np.array_equal(bits(base), bits(DP.noise(1, 2, 256)))
    # the count noise of the adaptive clip is the first normal of stream 1's first block
    assert DP.count_normal(1, 2) == DP.noise(1, 2, 4, stream=1)[0]


# ---- the rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,L', [(1, 4), (3, 36), (7, 132), (15, 64)])
def test_clipped_updates_are_bounded(M, L):
    W, x, q = rows(M, L, 10 * M + L, scale=3.0)
    S = 0.5 * float(np.sqrt(DP.norms_exact(W, x)).min())        # every row is clipped
    c, r, st = DP.coef(DP.norms(W, x), q, S, 0.0)
    assert st['b'] == 0 and st['dropped'] == 0 and (r > S).all()
    d = DP.updates(W, x)
    for k in range(M):
        term = (c[k] * d[k]).astype(F32).astype(F64)
        assert np.sqrt(np.sum(term * term)) <= float(q[k]) * S * (1 + 2.0 ** -22), k
    # and a generous clip changes nothing: c = q
    c2, _, st2 = DP.coef(DP.norms(W, x), q, 1e6, 0.0)
    assert np.array_equal(bits(c2), bits(q)) and st2['b'] == M


@pytest.mark.parametrize('M', [1, 2, 3, 8, 15])
def test_no_clip_no_noise_is_the_avgm_step(M):
    L = 36
    W, x, q = rows(M, L, 77 + M)
    got = DP.aggregate(W, x, q, np.inf, 0.0)
    sc = FO.scalars(1.0, 0.0, 0.99, 1e-3)
    ref, _, _ = FO.server('avgm', x, np.zeros(L, F32), None, list(W), q, sc)
    assert np.array_equal(bits(got['out']), bits(ref))
    assert np.array_equal(bits(got['c']), bits(q)) and got['state']['sigma'] == 0.0
    # the fold through fedopt_restatement's delta with the coefficients c
    assert np.array_equal(bits(DP.fold(W, x, got['c'])), bits(DP.fold_left(W, x, got['c'])))


@pytest.mark.parametrize('bad', ['nan', 'inf', '-inf', 'overflow'])
def test_a_nonfinite_row_changes_nothing_but_the_dropped_count(bad):
    M, L = 6, 36
    W, x, q = rows(M, L, 5)
    S, z = 0.8 * float(np.sqrt(np.median(DP.norms_exact(W, x)))), 1.3
    W2 = W.copy()
    W2[2, 7] = {'nan': np.nan, 'inf': np.inf, '-inf': -np.inf, 'overflow': 3e38}[bad]
    keep = [0, 1, 3, 4, 5]
    a = DP.aggregate(W2, x, q, S, z, seed=4, t=2)
    b = DP.aggregate(W[keep], x, q[keep], S, z, seed=4, t=2)
    assert a['state']['dropped'] == 1 and b['state']['dropped'] == 0
    assert a['c'][2] == 0 and np.array_equal(bits(a['c'][keep]), bits(b['c']))
    # (the left fold: the dropped row's +0 term leaves every partial sum as it is, except a -0 first term)
    assert np.array_equal(bits(a['out']), bits(b['out']))
    assert np.isfinite(a['out']).all()
    assert a['state']['sigma'] == b['state']['sigma'] and a['state']['b'] == b['state']['b']
    assert np.array_equal(bits(DP.fold(W2, x, a['c'])), bits(DP.fold_left(W2, x, a['c'])))


def test_special_norms():
    S = 2.0
    n = np.array([0.0, S * S, np.inf, np.nan, 4.0 * S * S], F64)
    q = np.full(5, F32(0.2))
    c, r, st = DP.coef(n, q, S, 0.5)
    assert r[0] == 0 and r[1] == S and np.isinf(r[2]) and np.isnan(r[3])
    assert c[0] == q[0] and c[1] == q[1] and c[2] == 0 and c[3] == 0 and c[4] == F32(F64(q[4]) * 0.5)
    assert st['b'] == 2 and st['dropped'] == 2 and st['sigma'] == (0.5 * S) * float(q[0]) and st['clip_next'] == S
    # an all-dropped round leaves x + noise
    W = np.full((2, 8), np.nan, F32)
    x = np.arange(8, dtype=F32)
    out = DP.aggregate(W, x, None, 1.0, 1.0, seed=1, t=0)
    assert out['state']['dropped'] == 2
    assert np.array_equal(bits(out['out']), bits((x + (F32(0.5) * DP.noise(1, 0, 8)).astype(F32)).astype(F32)))


def test_uniform_weights_and_sigma():
    c, _, st = DP.coef(np.ones(10), None, 3.0, 1.1)
    assert (c == F32(0.1)).all() and st['sigma'] == (1.1 * 3.0) * float(F32(0.1))
    assert DP.coef(np.ones(10), None, np.inf, 0.0)[2]['sigma'] == 0.0


def test_padding_columns_take_no_noise():
    x = np.zeros(2 * 8, F32)
    out = DP.finish(x, np.zeros_like(x), 1.0, DP.noise(0, 0, 16), 1.0, cols=(8, 5))
    out = out.reshape(2, 8)
    assert (out[:, 5:] == 0).all() and (out[:, :5] != 0).all()


def test_adaptive_clip_converges_to_the_quantile():
    rs = np.random.RandomState(3)
    M, gamma = 200, 0.7
    r = np.exp(rs.normal(0.0, 0.5, M))
    target = np.quantile(r, gamma)
    ad = dict(quantile=gamma, lr=0.2, count_noise=0.0)
    S = DP.adaptive_trajectory([r] * 400, 10.0, M, ad)
    assert abs(np.mean(r <= S[-1]) - gamma) <= 1.5 / M
    assert abs(S[-1] - target) <= 0.02 * target
    # from below as well, and with count noise the time average settles at the same place
    S = DP.adaptive_trajectory([r] * 400, 0.05, M, ad)
    assert abs(S[-1] - target) <= 0.02 * target
    S = DP.adaptive_trajectory([r] * 600, 10.0, M, dict(quantile=gamma, lr=0.2, count_noise=2.0), seed=5)
    assert abs(np.mean(S[300:]) - target) <= 0.05 * target
    # one step, written out
    b = float(np.sum(r <= 1.0))
    assert DP.clip_next(1.0, b, M, ad) == 1.0 * np.exp(-(0.2 * (b / M - gamma)))
    assert DP.clip_next(1.0, b, M, None) == 1.0


# ---- the public call's keyword checks and the driver's flags --------------------------------------------------
def test_dpfedavg_argument_errors_need_no_gpu():
    import fedamw_amd  # noqa: F401
    from fedamw_amd.functions import tools
    X = [np.zeros((4, 3), F32)] * 2
    y = [np.zeros(4, np.int64)] * 2
    args = (X, y, X[0], y[0], 'classification', 2, 8, 0.01, 1, 4, False, 0.1, False, 0.01, 2)
    for bad in (0.0, -1.0, float('nan'), 'one', None, True):
        with pytest.raises(ValueError, match='clip'):
            tools.DPFedAvg(*args, clip=bad, verbose=False)
    for bad in (-0.1, float('inf'), float('nan'), 'one', None, True):
        with pytest.raises(ValueError, match='noise_multiplier'):
            tools.DPFedAvg(*args, noise_multiplier=bad, verbose=False)
    with pytest.raises(ValueError, match='finite clip'):
        tools.DPFedAvg(*args, clip=float('inf'), noise_multiplier=1.0, verbose=False)
    for bad in (-1, 2 ** 64, 1.5, None, True):
        with pytest.raises(ValueError, match='noise_seed'):
            tools.DPFedAvg(*args, noise_seed=bad, verbose=False)
    with pytest.raises(ValueError, match='weighting'):
        tools.DPFedAvg(*args, weighting='loss', verbose=False)
    for bad in (0.5, dict(quantile=0.5), dict(lr=0.2), dict(quantile=1.5, lr=0.2), dict(quantile=0.5, lr=-1.0),
                dict(quantile=0.5, lr=0.2, count_noise=-1.0), dict(quantile=0.5, lr=0.2, momentum=0.9),
                dict(quantile='half', lr=0.2), dict(quantile=0.5, lr=float('inf'))):
        with pytest.raises(ValueError, match='adaptive'):
            tools.DPFedAvg(*args, adaptive=bad, verbose=False)
    with pytest.raises(ValueError, match='adaptive'):
        tools.DPFedAvg(*args, clip=float('inf'), noise_multiplier=0.0, adaptive=dict(quantile=0.5, lr=0.2), verbose=False)
    with pytest.raises(ValueError, match='byzantine'):
        tools.DPFedAvg(*args, byzantine=dict(fraction=2.0), verbose=False)
    with pytest.raises(ValueError, match='parallel'):
        tools._check_dp(1.0, 1.0, 0, 'uniform', None, 'sequential')
    tools._check_dp(float('inf'), 0.0, 2 ** 64 - 1, 'size', None)
    tools._check_dp(np.float32(1.0), np.int64(0), np.int64(3), 'uniform', dict(quantile=0.5, lr=0.2, count_noise=1.0))


def test_driver_accepts_the_flags(monkeypatch):
    import fedamw_amd  # noqa: F401
    from fedamw_amd import experiment
    seen = {}

    def fake_run(*pos, **kw):
        seen.update(kw, algos=pos[12])
        return dict(name=[], test_acc=np.zeros((0, 1, 1)), heterogeneity=0.0, seconds={})
    monkeypatch.setattr(experiment, 'run', fake_run)
    experiment.main(['--algos', 'FedAvg,FedTopK,DPFedAvg', '--dp-clip', '0.5', '--dp-noise-multiplier', '0.7',
                     '--dp-noise-seed', '11', '--dp-weighting', 'size', '--dp-adaptive-quantile', '0.6',
                     '--dp-adaptive-lr', '0.3', '--byzantine-fraction', '0.2'])
    assert seen['dp_clip'] == 0.5 and seen['dp_noise_multiplier'] == 0.7 and seen['dp_noise_seed'] == 11
    assert seen['dp_weighting'] == 'size' and seen['dp_adaptive_quantile'] == 0.6 and seen['dp_adaptive_lr'] == 0.3
    assert 'DPFedAvg' in seen['algos'] and seen['byzantine_fraction'] == 0.2
    assert experiment.EXTRA_DP == ['DPFedAvg']
    monkeypatch.undo()
    with pytest.raises(ValueError, match='unknown algorithm'):
        experiment.run(algos=('DPFedAvgX',), verbose=False)

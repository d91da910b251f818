"""tests/robust_restatement.py on the CPU: the trimmed-mean rule's order, ties, outliers and its
derived distance to the sorted float64 mean; the drop-ins' host checks; the driver's row order; the
header.  No GPU."""
import inspect
import os

import numpy as np
import pytest

from tests import robust_restatement as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MS = (1, 2, 3, 4, 5, 9, 33, 65, 257)


def bs(M):
    return sorted({b for b in (0, 1, (M - 1) // 4, (M - 1) // 2) if 2 * b < M})


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('kind', ['normal', 'quantised', 'near_one', 'wide'])
def test_within_the_derived_bound_of_the_sorted_float64_mean(M, kind):
    """|out - ref| <= 2^-24 |ref| + n 2^-52 mean|kept| + 2^-149 for every b."""
    W = RR.inputs(kind, M, 40)
    worst = 0.0
    for b in bs(M):
        out = RR.robust(W, b).astype(np.float64)
        err, bd = np.abs(out - RR.reference(W, b)), RR.bound(W, b)
        worst = max(worst, float((err / bd).max()))
        assert (err <= bd).all(), (M, kind, b, float((err / bd).max()))
    print('M %d %s: worst err / bound %.3f' % (M, kind, worst))


@pytest.mark.parametrize('M', [1, 3, 5, 9, 33, 65, 257, 1263, 2525])
@pytest.mark.parametrize('kind', ['normal', 'quantised', 'zeros', 'wide'])
def test_odd_median_is_numpys_bit_for_bit(M, kind):
    W = RR.inputs(kind, M, 12)
    out = RR.robust(W, (M - 1) // 2)
    if kind == 'zeros':          # (np.median's partition compares -0 == +0: the value is the same, the sign is ours)
        assert not out.any()
        assert (np.signbit(out) == (np.signbit(W).sum(0) > M // 2)).all()
    else:
        assert out.tobytes() == np.median(W, axis=0).astype(F32).tobytes()


@pytest.mark.parametrize('M', [2, 4, 64])
def test_even_median_is_the_mean_of_the_two_middle_values(M):
    W = RR.inputs('normal', M, 12)
    s = np.sort(W.astype(np.float64), 0)
    ref = ((s[M // 2 - 1] + s[M // 2]) / 2.0).astype(F32)
    assert RR.robust(W, (M - 1) // 2).tobytes() == ref.tobytes()


def test_key_order():
    """-NaN < -Inf < -1 < -0 < +0 < 1 < +Inf < +NaN, and the key is a bijection."""
    nneg = np.array([0xFFC00000], np.uint32).view(F32)[0]
    v = np.array([nneg, -np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], F32)
    assert np.signbit(v[0]) and not np.signbit(v[-1])
    k = RR.keys(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert RR.values(k).tobytes() == v.tobytes()


def test_signed_zeros_and_equal_columns():
    W = np.array([[0.0, -0.0, 2.5], [-0.0, -0.0, 2.5], [0.0, -0.0, 2.5]], F32)
    for b in (0, 1):
        out = RR.robust(W, b)
        assert out[2] == F32(2.5) and out[0] == 0 and out[1] == 0
    assert not np.signbit(RR.robust(W, 1)[0]) and np.signbit(RR.robust(W, 1)[1])   # the median is the value itself


def test_lowest_mantissa_bits_decide():
    base = np.array([1.0], F32).view(np.uint32)[0]
    col = (base + np.array([3, 0, 2, 1, 4], np.uint32)).view(F32).reshape(5, 1)
    assert RR.robust(col, 2).view(np.uint32)[0] == base + 2
    exp = (col.astype(np.float64)[[0, 2, 3], 0].sum() / 3.0)
    assert RR.robust(col, 1)[0] == F32(exp)


@pytest.mark.parametrize('M,b', [(5, 1), (9, 2), (33, 8), (65, 32)])
@pytest.mark.parametrize('bad', ['nan', 'inf', 'mixed'])
def test_b_bad_rows_per_side_give_the_clean_rows_answer(M, b, bad):
    """b rows of NaN / Inf at the top and b at the bottom: exactly the clean rows are kept, so the result is
    the clean rows' b = 0 value to the bound (the summation slices differ with the positions)."""
    clean = RR.inputs('normal', M - 2 * b, 20)
    nneg = np.array([0xFFC00000], np.uint32).view(F32)[0]
    top = {'nan': np.nan, 'inf': np.inf, 'mixed': np.nan}[bad]
    bot = {'nan': nneg, 'inf': -np.inf, 'mixed': -np.inf}[bad]
    W = np.concatenate([np.full((b, 20), top, F32), clean, np.full((b, 20), bot, F32)])
    W = W[np.random.RandomState(M).permutation(M)]
    out = RR.robust(W, b)
    assert np.isfinite(out).all()
    err = np.abs(out.astype(np.float64) - RR.reference(clean, 0))
    assert (err <= RR.bound(clean, 0)).all()
    # one more at the top survives the trim
    W2 = W.copy()
    W2[np.flatnonzero(np.isfinite(W[:, 0]))[0]] = top
    out2 = RR.robust(W2, b)
    assert (np.isnan(out2) if bad != 'inf' else np.isposinf(out2)).all()


def test_restatement_does_not_depend_on_the_rows_outside():
    W = RR.inputs('normal', 9, 8)
    big = np.full((20, 8), np.nan, F32)
    sel = np.array([1, 3, 4, 8, 9, 12, 15, 18, 19])
    big[sel] = W
    assert RR.robust(big[sel], 2).tobytes() == RR.robust(W, 2).tobytes()


def test_widths_and_trim_counts():
    assert [RR.width(M) for M in (1, 1250, 1261, 1262, 2523, 2524, 5047)] == [32, 32, 32, 16, 16, 8, 8]
    assert RR.trim_count('median', 0.1, 12) == 5 and RR.trim_count('median', 0.1, 1) == 0
    assert RR.trim_count('mean', 0.4, 12) == 0
    assert [RR.trim_count('trimmed_mean', 0.1, M) for M in (1, 9, 10, 12, 100)] == [0, 0, 1, 1, 10]
    assert RR.trim_count('trimmed_mean', 0.49, 2) == 0 and RR.trim_count('trimmed_mean', 0.49, 100) == 49


# ---- the drop-ins' host side ----

@pytest.fixture(scope='module')
def tools():
    import fedamw_amd  # noqa: F401
    from fedamw_amd.functions import tools
    return tools


def test_signatures(tools):
    fa = list(inspect.signature(tools.FedAvg).parameters.values())
    pos = [p.name for p in fa if p.kind == p.POSITIONAL_OR_KEYWORD]
    for fn, extra in ((tools.FedRobust, {'rule', 'trim', 'byzantine'}), (tools.FedMedian, {'byzantine'}),
                      (tools.FedTrimmedMean, {'trim', 'byzantine'})):
        ps = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in ps if p.kind == p.POSITIONAL_OR_KEYWORD] == pos
        kw = {p.name for p in ps if p.kind == p.KEYWORD_ONLY}
        assert kw == extra | {'stats', 'verbose', 'options', 'participation', 'sample_seed'}
    d = inspect.signature(tools.FedRobust).parameters
    assert d['rule'].default == 'median' and d['trim'].default == 0.1 and d['byzantine'].default is None


def test_argument_checks(tools):
    X = [np.zeros((4, 3), F32)] * 3
    y = [np.zeros(4, np.int64)] * 3
    a = (X, y, X[0], y[0], 'classification', 2, 8, 0.1, 1, 2, False, 0.0, False, 0.0, 1)
    for trim in (-0.1, 0.5, 1.0, float('nan')):
        with pytest.raises(ValueError, match='trim'):
            tools.FedRobust(*a, rule='trimmed_mean', trim=trim)
        with pytest.raises(ValueError, match='trim'):
            tools.FedTrimmedMean(*a, trim=trim)
    with pytest.raises(ValueError, match='rule'):
        tools.FedRobust(*a, rule='krum')
    for bz in (dict(ids=[0], fraction=0.1), dict(), dict(ids=[3]), dict(ids=[-1]), dict(fraction=1.5),
               dict(ids=[0], attack='zero'), dict(ids=[0], foo=1)):
        with pytest.raises(ValueError, match='byzantine'):
            tools.FedMedian(*a, byzantine=bz)
    with pytest.raises(ValueError, match='above'):
        tools._check_robust_rounds([12, 5048], 5047)
    with pytest.raises(ValueError, match='no client'):
        tools._check_robust_rounds([12, 0], 5047)
    tools._check_robust_rounds([1, 5047], 5047)


def test_byzantine_id_selection(tools):
    assert tools.byzantine_plan(10, None) is None
    ids, attack, scale, seed = tools.byzantine_plan(10, dict(ids=[7, 2, 2], attack='nan', scale=3))
    assert ids.tolist() == [2, 7] and ids.dtype == np.int64 and (attack, scale, seed) == ('nan', 3.0, 0)
    a = tools.byzantine_plan(40, dict(fraction=0.25, seed=4))[0]
    b = tools.byzantine_plan(40, dict(fraction=0.25, seed=4))[0]
    c = tools.byzantine_plan(40, dict(fraction=0.25, seed=5))[0]
    assert len(a) == 10 and len(set(a.tolist())) == 10 and (np.diff(a) > 0).all() and a.min() >= 0 and a.max() < 40
    assert a.tolist() == b.tolist() and a.tolist() != c.tolist()
    assert len(tools.byzantine_plan(12, dict(fraction=0.2))[0]) == 2      # floor(2.4)
    assert len(tools.byzantine_plan(12, dict(fraction=0.0))[0]) == 0
    z1, z2 = tools.byzantine_noise(3, 1, (2, 2, 5)), tools.byzantine_noise(3, 1, (2, 2, 5))
    assert z1.shape == (2, 2, 5) and z1.numpy().tobytes() == z2.numpy().tobytes()
    assert z1.numpy().tobytes() != tools.byzantine_noise(3, 2, (2, 2, 5)).numpy().tobytes()


def test_trim_count_matches_the_restatement(tools):
    for rule in tools.ROBUST_RULES:
        for trim in (0.0, 0.1, 0.25, 0.3, 0.49):
            for M in (1, 2, 3, 7, 10, 12, 100, 1250):
                b = tools.robust_trim_count(rule, trim, M)
                assert b == RR.trim_count(rule, trim, M) and 0 <= 2 * b < M


def test_driver_row_order():
    from fedamw_amd import experiment as E
    assert E.EXTRA_ROBUST == ['FedMedian', 'FedTrimmedMean']
    src = inspect.getsource(E)
    assert src.index('EXTRA_FAIR = ') < src.index('EXTRA_ROBUST = ')
    assert 'EXTRA + EXTRA_FAIR + EXTRA_ROBUST' in src
    with pytest.raises(ValueError, match='unknown algorithm'):
        E.run(algos=('FedKrum',))
    ap = inspect.getsource(E.main)
    for flag in ('--robust-trim', '--byzantine-fraction', '--byzantine-attack', '--byzantine-scale'):
        assert flag in ap


def test_header_and_exports():
    from fedamw_amd import _lib
    h = open(os.path.join(ROOT, 'include', 'fedsim.h')).read()
    for sym in ('fs_aggregate_robust', 'fs_aggregate_robust_max_m', 'fs_plan_set_robust'):
        assert sym in _lib.EXPORTS and ('int %s(' % sym) in h
    assert '#define FS_ABI_VERSION 23' in h or _lib.ABI_VERSION == 23
    L = _lib.lib()
    assert L.fs_aggregate_robust_max_m() == RR.MAX_M >= 2048
    # the error returns need no device: nothing is launched
    for M, b, ln in ((0, 0, 4), (RR.MAX_M + 1, 0, 4), (4, 2, 4), (5, 3, 4), (4, 1, 6), (4, -1, 4)):
        assert L.fs_aggregate_robust(1, ln, None, M, ln, b, 1, None) < 0, (M, b, ln)

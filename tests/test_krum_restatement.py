"""tests/krum_restatement.py on the CPU: the Krum rule's score order, ties, duplicates, +Inf rows and its
distance to the sorted float64 sum; what the rule guarantees and what it does not; the drop-ins' host
checks; the driver's row order; the header.  No GPU."""
import inspect
import os

import numpy as np
import pytest

from tests import krum_restatement as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


# ---- (ii) on hand-made D ----

def test_ties_at_the_threshold():
    D, f, m = KR.hand_made()['ties_at_threshold']
    s = KR.scores(D, f)
    assert s[0] == 3.0                       # three of the four copies of 1, not the 2
    assert s[4] == 1.0 + 1.0 + 2.0 and s[5] == 1.0 + 2.0 + 3.0
    assert KR.pick(s, 1).tolist() == [0]
    assert KR.pick(s, 5).tolist() == sorted(np.argsort(s, kind='stable')[:5].tolist())


def test_duplicate_rows_and_equal_scores_by_id():
    D, f, _ = KR.hand_made()['duplicate_rows_krum']
    s = KR.scores(D, f)                      # n = 2: rows 0 and 1 both 0 + 2
    assert s[0] == s[1] == 2.0 and D[0, 1] == 0 and D[0, 0] == 0
    assert KR.pick(s, 1).tolist() == [0]     # the smaller id wins an equal score
    assert KR.pick(s, 2).tolist() == [0, 1]
    E, f, m = KR.hand_made()['equal_scores_by_id']
    s = KR.scores(E, f)
    assert (s == 3.0).all() and KR.pick(s, m).tolist() == [0, 1, 2]
    s = KR.scores(E, 0)
    assert (s == 5.0).all() and KR.pick(s, 7).tolist() == list(range(7))


def test_self_is_excluded_by_index_not_by_value():
    """A row at distance 0 from another keeps that 0: only its own entry is left out."""
    D = KR.sym([[0, 0, 0, 5], [0, 0, 0, 6], [0, 0, 0, 7], [0, 0, 0, 0]])
    s = KR.scores(D, 0)                      # n = 2
    assert s.tolist() == [0.0, 0.0, 0.0, 11.0]
    D2 = D.copy()
    D2[0, 0] = 9.0                           # whatever stands on the diagonal is not read
    assert KR.scores(D2, 0).tolist() == s.tolist()


def test_inf_rows():
    G, f, _ = KR.hand_made()['inf_rows_krum']
    s = KR.scores(G, f)                      # M = 8, f = 2, n = 4: the good rows have 5 finite distances
    assert np.isposinf(s[[2, 5]]).all() and np.isfinite(np.delete(s, [2, 5])).all()
    assert not set(KR.pick(s, 6).tolist()) & {2, 5}
    s1 = KR.scores(G, 1)                     # n = 5: still 5 finite distances per good row
    assert np.isfinite(np.delete(s1, [2, 5])).all()
    assert KR.pick(s1, 7).tolist() == [0, 1, 2, 3, 4, 6, 7]     # m above the finite scores: the smaller Inf id
    s0 = KR.scores(G, 0)                     # n = 6 > 5: every score is +Inf, the ids decide
    assert np.isposinf(s0).all() and KR.pick(s0, 3).tolist() == [0, 1, 2]


def test_smallest_shapes():
    H, f, _ = KR.hand_made()['M3_f0_n1_krum']
    s = KR.scores(H, 0)                      # n = 1: each row's nearest neighbour
    assert s.tolist() == [1.0, 2.0, 1.0]
    assert KR.pick(s, 1).tolist() == [0] and KR.pick(s, 3).tolist() == [0, 1, 2]
    assert KR.pick(s, 2, sel=np.array([4, 7, 9])).tolist() == [4, 9]      # ids of the larger buffer, not positions
    sc, pk, q = KR.select(H, 0, 3)
    assert q.dtype == F32 and q.tolist() == [F32(1.0 / 3)] * 3 and pk.dtype == np.int32 and sc.dtype == F64


@pytest.mark.parametrize('name', sorted(KR.hand_made()))
def test_hand_made_cases_against_the_sorted_sum(name):
    D, f, m = KR.hand_made()[name]
    s, ref = KR.scores(D, f), KR.sorted_score(D, f)
    assert s.tobytes() == ref.tobytes()      # small integers and +Inf: every order gives the same double
    pk = KR.pick(s, m)
    assert len(pk) == m == len(set(pk.tolist())) and (np.diff(pk) > 0).all()
    best = sorted((float(v), a) for a, v in enumerate(s))[:m]
    assert sorted(a for _, a in best) == pk.tolist()


@pytest.mark.parametrize('M', [3, 4, 5, 17, 64, 65, 257, 600])
@pytest.mark.parametrize('quantised', [False, True])
def test_score_within_n_ulp_of_the_sorted_float64_sum(M, quantised):
    """|s - ref| <= n 2^-53 s: n double additions of non-negative terms, in whatever order."""
    D = KR.random_D(M, quantised=quantised)
    for f, m in KR.fm_cases(M):
        n = M - f - 2
        s, ref = KR.scores(D, f), KR.sorted_score(D, f)
        assert (np.abs(s - ref) <= n * 2.0 ** -53 * ref).all(), (M, f)
        if quantised:
            assert s.tobytes() == ref.tobytes()
        pk = KR.pick(s, m)
        assert len(pk) == m and (np.diff(pk) > 0).all()


def test_pick_follows_sel():
    s = np.array([5.0, 1.0, 3.0, 1.0, 4.0])
    assert KR.pick(s, 2).tolist() == [1, 3]
    assert KR.pick(s, 3, sel=np.array([10, 20, 30, 40, 50])).tolist() == [20, 30, 40]
    assert KR.pick(s, 1).tolist() == [1]


# ---- what the rule guarantees ----

def _cluster(M, L, seed):
    rs = np.random.RandomState(seed)
    x = rs.normal(size=L).astype(F32)
    return (x[None, :] + 1e-2 * rs.normal(size=(M, L))).astype(F32), x


def _device_like_D(W, x):
    """float32 D from the float64 distances; rows with a non-finite value at +Inf."""
    U = KR.centred(W, x)
    bad = ~np.isfinite(U).all(1)
    with np.errstate(all='ignore'):
        D = KR.distances64(np.where(bad[:, None], 0, W).astype(F32), x)[0]
    D[bad, :] = np.inf
    D[:, bad] = np.inf
    D[np.arange(len(D)), np.arange(len(D))] = 0
    with np.errstate(over='ignore'):
        return D.astype(F32)


@pytest.mark.parametrize('M,f', [(7, 2), (13, 5), (20, 3), (65, 31)])
@pytest.mark.parametrize('bad', ['far', 'nan', 'inf'])
def test_at_most_f_bad_rows_are_never_picked(M, f, bad):
    assert M >= 2 * f + 3
    W, x = _cluster(M, 24, M)
    rows = np.random.RandomState(f).permutation(M)[:f]
    if bad == 'far':                         # each somewhere else, 100 cluster widths away
        W[rows] = (x[None, :] + np.random.RandomState(9).normal(size=(f, 24))).astype(F32)
    else:
        W[rows, 3] = np.nan if bad == 'nan' else np.inf
    D = _device_like_D(W, x)
    for m in (1, (M - f + 1) // 2, M - f):
        s, pk, _ = KR.select(D, f, m)
        assert not set(pk.tolist()) & set(rows.tolist()), (M, f, bad, m)
        assert np.isfinite(s[pk]).all()
        if bad != 'far':
            assert np.isposinf(s[rows]).all()


def test_f_plus_one_colluding_rows_can_win():
    """f + 1 identical bad rows are each other's nearest neighbours: with n = M - f - 2 their score is the
    distance to the closest good rows only, and Krum picks one of them -- the bound is the rule's."""
    M, f = 11, 4
    W, x = _cluster(M, 24, 5)
    W = (x[None, :] + 1.0 * (W - x[None, :]) * 50).astype(F32)             # a wide cluster of good rows
    bad = np.arange(f + 1)
    W[bad] = (x + 0.05).astype(F32)                                        # f + 1 copies, just off the centre
    D = _device_like_D(W, x)
    s, pk, _ = KR.select(D, f, 1)
    assert pk[0] in bad
    # with one of them removed (f of them) and M >= 2f + 3 still true, f colluders CAN still sit at the centre;
    # what the rule promises is only that far-away or non-finite rows lose -- the case above


# ---- (i) ----

def test_distances64_and_bound_shapes():
    W, x = KR.rows('gaussian', 17, 64)
    D, n2 = KR.distances64(W, x)
    assert D.shape == (17, 17) and (D == D.T).all() and (np.diag(D) == 0).all() and (D[~np.eye(17, dtype=bool)] > 0).all()
    U = KR.centred(W, x).astype(F64)
    assert np.allclose(D[2, 5], ((U[2] - U[5]) ** 2).sum(), rtol=1e-14) and np.allclose(n2[3], (U[3] ** 2).sum())
    assert (KR.dist_bound(D, n2, 17, 64) > 0).all()
    Wd, _ = KR.rows('duplicate', 17, 64)
    assert KR.distances64(Wd, x)[0][0, 16] == 0.0
    assert KR.bad_rows(3) == [0] and KR.bad_rows(4) == [0, 2] and KR.bad_rows(17) == [0, 8, 16]


def test_split_and_chain():
    assert KR.split(100, 4096) == (16, 8)          # one tile pair: the len axis fills the chip
    assert KR.split(1000, 28672) == (14, 64)       # 36 pairs x 14 slices = 504 workgroups
    assert KR.split(5120, 64) == (1, 8) and KR.split(3, 4) == (1, 8)
    for M in (3, 100, 129, 257, 1000, 1250, 5120):
        for L in (4, 64, 260, 4096, 20480, 28672):
            S, kc = KR.split(M, L)
            assert S >= 1 and kc >= 8 and (S - 1) * kc * 32 < L <= S * kc * 32 + 31
            assert KR.chain(M, L) <= L + 2


# ---- the drop-ins' host side ----

@pytest.fixture(scope='module')
def tools():
    import fedamw_amd  # noqa: F401
    from fedamw_amd.functions import tools
    return tools


def test_signatures(tools):
    fa = list(inspect.signature(tools.FedAvg).parameters.values())
    pos = [p.name for p in fa if p.kind == p.POSITIONAL_OR_KEYWORD]
    for fn, extra in ((tools.FedKrum, {'f', 'm', 'byzantine'}), (tools.Krum, {'f', 'byzantine'}),
                      (tools.MultiKrum, {'f', 'byzantine'})):
        ps = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in ps if p.kind == p.POSITIONAL_OR_KEYWORD] == pos
        kw = {p.name for p in ps if p.kind == p.KEYWORD_ONLY}
        assert kw == extra | {'stats', 'verbose', 'options', 'participation', 'sample_seed'}
    d = inspect.signature(tools.FedKrum).parameters
    assert d['f'].default == 0.1 and d['m'].default is None and d['byzantine'].default is None


def test_argument_checks(tools):
    X = [np.zeros((4, 3), F32)] * 7
    y = [np.zeros(4, np.int64)] * 7
    a = (X, y, X[0], y[0], 'classification', 2, 8, 0.1, 1, 2, False, 0.0, False, 0.0, 1)
    for f in (-0.1, 0.5, 1.5, float('nan'), -1, '0.1', None, True):
        with pytest.raises(ValueError, match='f must be'):
            tools.FedKrum(*a, f=f)
        with pytest.raises(ValueError, match='f must be'):
            tools.Krum(*a, f=f)
    for m in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='m must be'):
            tools.FedKrum(*a, m=m)
    with pytest.raises(ValueError, match=r'M >= 2f \+ 3'):
        tools.FedKrum(*a, f=3)                       # 7 < 9
    with pytest.raises(ValueError, match=r'M >= 2f \+ 3'):
        tools.MultiKrum(*a, f=0.45)                  # floor(3.15) = 3
    with pytest.raises(ValueError, match=r'outside \[1, M - f\]'):
        tools.FedKrum(*a, f=2, m=6)
    for bz in (dict(ids=[0], fraction=0.1), dict(), dict(ids=[7]), dict(ids=[0], attack='zero')):
        with pytest.raises(ValueError, match='byzantine'):
            tools.MultiKrum(*a, byzantine=bz)
    with pytest.raises(ValueError, match='above'):
        tools._check_krum_rounds([12, KR.MAX_M + 1], 0.1, None, KR.MAX_M)
    with pytest.raises(ValueError, match=r'M >= 2f \+ 3'):
        tools._check_krum_rounds([12, 2], 0.1, None, KR.MAX_M)
    assert tools._check_krum_rounds([3, 12, KR.MAX_M], 0.1, None, KR.MAX_M) == [(0, 3), (1, 11), (512, 4608)]
    assert tools._check_krum_rounds([12, 9], 2, 1, KR.MAX_M) == [(2, 1), (2, 1)]
    with pytest.raises(ValueError, match='parallel'):
        tools._check_krum(0.1, None, 'sequential')


def test_counts_match_the_restatement(tools):
    for f in (0, 1, 3, 0.0, 0.1, 0.25, 0.3, 0.49):
        for M in (3, 7, 9, 10, 12, 100, 1250):
            for m in (None, 1, 2):
                try:
                    got = tools.krum_counts(f, m, M)
                except ValueError:
                    fc, mc = KR.counts(f, m, M)
                    assert M < 2 * fc + 3 or not 1 <= mc <= M - fc
                    continue
                assert got == KR.counts(f, m, M) and M >= 2 * got[0] + 3 and 1 <= got[1] <= M - got[0]


def test_driver_row_order():
    from fedamw_amd import experiment as E
    assert E.EXTRA_KRUM == ['Krum', 'MultiKrum'] and E.EXTRA_ROBUST == ['FedMedian', 'FedTrimmedMean']
    src = inspect.getsource(E)
    assert src.index('EXTRA_ROBUST = ') < src.index('EXTRA_KRUM = ')
    assert 'EXTRA + EXTRA_FAIR + EXTRA_ROBUST + EXTRA_KRUM' in src
    with pytest.raises(ValueError, match='unknown algorithm'):
        E.run(algos=('Bulyan',))
    ap = inspect.getsource(E.main)
    for flag in ('--krum-f', '--byzantine-fraction', '--byzantine-attack', '--byzantine-scale'):
        assert flag in ap


def test_header_and_exports():
    import ctypes
    from fedamw_amd import _lib
    h = open(os.path.join(ROOT, 'include', 'fedsim.h')).read()
    for sym in ('fs_aggregate_krum', 'fs_aggregate_krum_max_m', 'fs_krum_distances', 'fs_krum_select', 'fs_krum_split',
                'fs_plan_set_krum'):
        assert sym in _lib.EXPORTS and ('int %s(' % sym) in h
    for sym in ('fs_aggregate_krum_ws_bytes', 'fs_krum_distances_ws_bytes'):
        assert sym in _lib.EXPORTS and ('int64_t %s(' % sym) in h
    assert _lib.ABI_VERSION == 23 and 'aggregate_krum' in _lib.KERNEL_SOURCES
    L = _lib.lib()
    assert L.fs_aggregate_krum_max_m() == KR.MAX_M >= L.fs_aggregate_robust_max_m()
    # the split and the workspace sizes are host arithmetic
    for M, ln in ((3, 4), (100, 4096), (1000, 28672), (1250, 4096), (KR.MAX_M, 64), (257, 20480)):
        s, k = ctypes.c_int(), ctypes.c_int()
        assert L.fs_krum_split(M, ln, ctypes.byref(s), ctypes.byref(k)) == 0 and (s.value, k.value) == KR.split(M, ln)
        T = (M + 127) // 128
        part = max(KR.split(min(t * 128, M), ln)[0] * (t * (t + 1) // 2) * 65536 for t in range(1, T + 1))
        assert L.fs_krum_distances_ws_bytes(M, ln) == part
        assert L.fs_aggregate_krum_ws_bytes(M, ln) == part + 4 * (M + 2) * KR.ldd(M)
    # the error returns need no device: nothing is launched
    big = 1 << 40
    for M, f, m, ln, st, ws in ((2, 0, 1, 4, 4, big), (5, -1, 1, 4, 4, big), (5, 3, 1, 4, 4, big), (5, 1, 0, 4, 4, big),
                                (5, 1, 5, 4, 4, big), (KR.MAX_M + 1, 1, 1, 4, 4, big), (5, 1, 1, 6, 8, big),
                                (5, 1, 1, 4, 6, big), (5, 1, 1, 8, 4, big), (5, 1, 1, 4, 4, 16)):
        assert L.fs_aggregate_krum(1, st, None, M, ln, 1, f, m, 1, 1, 1, 1, ws, None, 0, 0, None) < 0, (M, f, m, ln, st)
    assert L.fs_aggregate_krum(1, 4, None, 5, 4, None, 1, 1, 1, 1, 1, 1, big, None, 0, 0, None) < 0
    assert L.fs_krum_select(None, 5, 1, 1, None, 1, 1, None, 1, None) < 0
    assert L.fs_krum_select(1, 5, 1, 5, None, 1, 1, None, 1, None) < 0
    assert L.fs_krum_select(1, 5, 1, 1, None, 1, 1, None, None, None) < 0
    assert L.fs_krum_distances(1, 4, None, 5, 4, 1, 1, 1, 16, None) < 0

"""tests/topk_restatement.py itself: the kept count, the exact split a == s + e', the dense identity against
fold_restatement's update fold, memory carried over two calls, tools.topk_count's rounding and FedTopK's
argument errors (no GPU)."""
import numpy as np
import pytest

from tests import fold_restatement as FR
from tests import topk_restatement as TK

F32 = np.float32


def rows(M, L, seed=0):
    rs = np.random.RandomState(seed + 7 * M + L)
    W = rs.standard_normal((M, L)).astype(F32)
    x = rs.standard_normal(L).astype(F32)
    q = rs.dirichlet(np.full(M, 2.0)).astype(F32)
    return W, x, q


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize('M,L', [(1, 4), (3, 36), (17, 132), (65, 64)])
def test_kept_count_without_ties_is_kcount(M, L):
    W, x, q = rows(M, L)
    a = TK.corrected(W, x)
    assert len(np.unique(TK.keys(a[0]))) == L          # (normal draws: no two magnitudes alike)
    for kc in sorted({1, 2, L // 2, L - 1, L}):
        tau, n, kept = TK.threshold(a, kc)
        assert (n == kc).all() and (kept.sum(axis=1) == kc).all()
        # the kept ones are the kc largest magnitudes
        for k in range(M):
            order = np.argsort(-np.abs(a[k]), kind='stable')
            assert set(np.flatnonzero(kept[k])) == set(order[:kc])
            assert tau[k] == TK.keys(a[k])[order[kc - 1]]


def test_ties_are_all_kept_and_the_count_is_at_least_kcount():
    rs = np.random.RandomState(3)
    mags = np.array([0.25, 0.5, 1.0, 2.0, 256.0], F32)         # two binades apart at the top: other radix digits
    a = (mags[rs.randint(0, 5, (6, 40))] * rs.choice([-1.0, 1.0], (6, 40))).astype(F32)
    for kc in (1, 2, 20, 39, 40):
        tau, n, kept = TK.threshold(a, kc)
        assert (n >= kc).all()
        for k in range(6):
            key = TK.keys(a[k])
            assert (key[kept[k]] >= tau[k]).all() and (key[~kept[k]] < tau[k]).all()
            assert (key > tau[k]).sum() < kc <= (key >= tau[k]).sum()
    assert (TK.threshold(a, 20)[1] > 20).any()                 # a tie at the threshold widens the set


def test_zero_row_keeps_everything_and_non_finite_values_are_always_kept():
    z = np.zeros((1, 12), F32)
    tau, n, kept = TK.threshold(z, 3)
    assert tau[0] == 0 and n[0] == 12 and kept.all()
    a = np.arange(1, 13, dtype=F32)[None, :].copy()
    a[0, 2], a[0, 5], a[0, 7] = np.inf, -np.inf, np.nan
    tau, n, kept = TK.threshold(a, 1)
    assert n[0] == 1 and kept[0, 7]                             # NaN above Inf
    tau, n, kept = TK.threshold(a, 3)
    assert n[0] == 3 and kept[0, [2, 5, 7]].all()              # +Inf and -Inf tie
    tau, n, kept = TK.threshold(a, 2)
    assert n[0] == 3


@pytest.mark.parametrize('M,L', [(2, 8), (17, 36), (65, 132)])
def test_split_is_exact(M, L):
    W, x, q = rows(M, L, 1)
    e = (np.random.RandomState(5).standard_normal((M, L)) * 0.1).astype(F32)
    r = TK.aggregate(W, x, e, q, max(1, L // 4))
    a, s, e2 = r['a'], r['s'], r['e']
    assert np.array_equal(bits((s + e2).astype(F32)), bits(a))
    assert ((s == 0) | (e2 == 0)).all() and not np.signbit(e2[s != 0]).any() and not np.signbit(s[e2 != 0]).any()
    assert np.array_equal(r['kept'], (s != 0).sum(axis=1))


@pytest.mark.parametrize('M', [1, 3, 15, 16, 17, 65, 513])
@pytest.mark.parametrize('chunks,wsp', [(0, None), (0, 64), (1, 64), (4, 64)])
def test_dense_identity(M, chunks, wsp):
    L = 20
    W, x, q = rows(M, L, 2)
    ref = TK.dense(W, x, q, chunks, wsp)
    # the same fold written with fold_restatement directly
    own = FR.fold(M, chunks, wsp, lambda k, first: (q[k] * (W[k] - x).astype(F32)).astype(F32), lambda t: (x + t).astype(F32))
    assert np.array_equal(bits(ref), bits(own))
    for e in (None, np.zeros((M, L), F32)):
        r = TK.aggregate(W, x, e, q, L, chunks, wsp)
        assert np.array_equal(bits(r['out']), bits(ref)) and (r['kept'] == L).all()
        if e is not None:
            assert not r['e'].any() and not np.signbit(r['e']).any()
    # any kcount at which every nonzero is kept: rows with zeros in them
    Wz = W.copy()
    Wz[:, ::3] = x[::3]
    nz = int((Wz[0] != x).sum())
    r = TK.aggregate(Wz, x, np.zeros((M, L), F32), q, nz, chunks, wsp)
    assert np.array_equal(bits(r['out']), bits(TK.dense(Wz, x, q, chunks, wsp))) and not r['e'].any()


def test_memory_is_carried_over_two_calls():
    M, L, kc = 5, 24, 3
    W, x, q = rows(M, L, 4)
    e0 = np.zeros((M, L), F32)
    r1 = TK.aggregate(W, x, e0, q, kc)
    assert (r1['kept'] == kc).all() and ((r1['e'] != 0).sum(axis=1) == L - kc).all()
    W2 = (W + F32(0.125)).astype(F32)
    r2 = TK.aggregate(W2, r1['out'], r1['e'], q, kc)
    a2 = ((W2 - r1['out'][None, :]).astype(F32) + r1['e']).astype(F32)
    assert np.array_equal(bits(r2['a']), bits(a2))
    nomem = TK.aggregate(W2, r1['out'], None, q, kc)
    assert not np.array_equal(bits(nomem['out']), bits(r2['out'])) and nomem['e'] is None
    # what was sent and what is left add up to everything the client ever produced
    assert np.array_equal(bits((r2['s'] + r2['e']).astype(F32)), bits(a2))


def test_topk_count_rounding():
    import fedamw_amd  # noqa: F401
    from fedamw_amd.functions import tools
    for ratio, C, D, want in [(0.01, 2, 2048, 40), (0.1, 14, 2048, 2867), (1.0, 3, 32, 96), (1e-9, 3, 32, 1),
                              (0.05, 3, 32, 4), (0.5, 1, 3, 1), (7, 3, 32, 7), (96, 3, 32, 96), (1, 3, 32, 1),
                              (np.float32(0.25), 2, 10, 5), (np.int64(5), 2, 10, 5)]:
        assert tools.topk_count(ratio, C, D) == want == TK.topk_count(ratio, C, D), (ratio, C, D)
    for bad in (0, -1, 0.0, -0.5, 1.5, float('nan'), float('inf'), True, 'all', None, 97):
        with pytest.raises(ValueError):
            tools.topk_count(bad, 3, 32)


def test_fedtopk_argument_errors_need_no_gpu():
    import fedamw_amd  # noqa: F401
    from fedamw_amd.functions import tools
    X = [np.zeros((4, 3), F32)] * 2
    y = [np.zeros(4, np.int64)] * 2
    args = (X, y, X[0], y[0], 'classification', 2, 8, 0.01, 1, 4, False, 0.1, False, 0.01, 2)
    for bad in (0.0, 1.5, -0.1, 0, True, 'half', None, float('nan')):
        with pytest.raises(ValueError, match='ratio'):
            tools.FedTopK(*args, ratio=bad, verbose=False)
    with pytest.raises(ValueError, match='ratio'):
        tools.FedTopK(*args, ratio=17, verbose=False)            # an int count above C * D = 16
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='error_feedback'):
            tools.FedTopK(*args, error_feedback=bad, verbose=False)
    with pytest.raises(ValueError, match='parallel'):
        tools._check_topk(0.1, True, 'sequential')

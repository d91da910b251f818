"""CPU checks of tests/softmax_reference.py: the inputs of tests/test_gpu_softmax.py are proven
before any kernel is judged on them.  Saturated steps are exact in fp32 (the fp32 oracle equals the
float64 reference bitwise), 'all_won' clients do not move, every 'mixed' case is well-conditioned
(the fp32 oracle within a quarter of the bound the GPU test asserts), and the inputs cover what
they claim to cover."""
import numpy as np
import pytest
import torch

from oracle import fedsim_oracle as O
from tests import softmax_reference as R

F32 = np.float32


def _same(a, b):
    return np.array_equal(np.asarray(a, F32), np.asarray(b, F32))


# --------------------------------------------------------------------------- saturated training
@pytest.mark.parametrize('n,D,C,B', [(64, 64, 3, 32), (96, 200, 10, 32), (48, 130, 17, 16), (128, 64, 26, 64),
                                     (64, 1024, 5, 32), (64, 2048, 16, 32), (64, 64, 2, 32)])
def test_saturated_training_is_exact_in_float32(n, D, C, B):
    """First-step logits exact and won by 200 or more, every row still won by GAP_EXACT or more
    through E = 2 epochs (softmax_reference.GAP_EXACT: why not 200), and the fp32 oracle's W bitwise
    the float64 reference's rounded to float32."""
    rs = np.random.RandomState(n + D + C)
    Xs, ys, W0 = R.train_problem(rs, [n], D, C, 'saturated')
    X, y = Xs[0], ys[0]
    assert X.dtype == F32 and W0.dtype == F32
    z32 = X @ W0.T
    z64 = X.astype(np.float64) @ W0.astype(np.float64).T
    perm = np.random.RandomState(1).permutation(D)
    assert np.array_equal(z32.astype(np.float64), z64) and np.array_equal(X[:, perm] @ W0[:, perm].T, z32)
    s0 = np.sort(z64, axis=1)
    assert (s0[:, -1] - s0[:, -2]).min() >= R.GAP_START
    offs = np.unique(np.round((np.sort(z64, axis=1)[:, -1] - 256.0) / 64.0))
    assert set(offs) == {-2.0, -1.0, 0.0, 1.0, 2.0}                # winners sit at 256 + 0, +-64, +-128
    torch.manual_seed(5)
    W64, l64, gap = R.train_ref64(X, y, W0, R.LR_SAT, 2, B, False, 0.0, False, 0.0)
    assert gap >= R.GAP_EXACT, gap
    torch.manual_seed(5)
    W32, l32 = O.train_client(X, y, W0, R.LR_SAT, 2, B, False, 0.0, False, 0.0)
    assert _same(W32, W64), np.abs(W32 - W64).max()
    assert abs(l32 - l64) <= R.TOL * max(1.0, abs(l64))
    moved = float(np.abs(W64 - W0).max())
    print('(n, D, C, B) = %s: gap %.1f, W moved by %.3g, loss %.4g' % ((n, D, C, B), gap, moved, l64))
    assert moved >= 2.0 ** -5                                    # not a vacuous check
    assert 0 in y and C - 1 in y and (y != np.argmax(z64, axis=1)).any()


@pytest.mark.parametrize('n,D,C,B', [(64, 64, 1, 32), (64, 64, 3, 32), (96, 200, 10, 32), (128, 64, 26, 64)])
def test_all_won_client_does_not_move(n, D, C, B):
    rs = np.random.RandomState(n + D + C + 1)
    Xs, ys, W0 = R.train_problem(rs, [n], D, C, 'all_won')
    torch.manual_seed(3)
    W64, l64, gap = R.train_ref64(Xs[0], ys[0], W0, R.LR_SAT, 2, B, False, 0.0, False, 0.0)
    assert _same(W64, W0) and l64 == 0.0
    torch.manual_seed(3)
    W32, l32 = O.train_client(Xs[0], ys[0], W0, R.LR_SAT, 2, B, False, 0.0, False, 0.0)
    assert _same(W32, W0) and l32 == 0.0


@pytest.mark.parametrize('case', R.SAT_TRAIN_CASES, ids=R.id_of)
def test_saturated_gpu_cases_are_exact(case):
    """The very inputs of the GPU test: chained and parallel, the fp32 oracle equals the float64
    reference bitwise on every client, rows start won by 200 or more and stay won by GAP_EXACT, the 'all_won' client returns
    its start with loss 0.0, and the others move."""
    form, G, D, C, B = case
    Xs, ys, W0 = R.saturated_train_inputs(*case)
    args = (R.LR_SAT, 2, B, False, 0.0, False, 0.0)
    for X in Xs if C >= 2 else ():
        s0 = np.sort(X.astype(np.float64) @ W0.astype(np.float64).T, axis=1)
        assert (s0[:, -1] - s0[:, -2]).min() >= R.GAP_START
    for chained in (False, True):
        torch.manual_seed(11)
        W64, l64, gap = R.train_chain_ref64(Xs, ys, W0, *args, chained)
        torch.manual_seed(11)
        W32, l32 = R.train_chain_f32(Xs, ys, W0, *args, chained)
        assert gap >= R.GAP_EXACT, gap
        print('%s %s: least lead %.1f' % (R.id_of(case), 'chained' if chained else 'parallel', gap))
        for j in range(len(Xs)):
            assert _same(W32[j], W64[j]), (chained, j)
            assert abs(l32[j] - l64[j]) <= R.TOL * max(1.0, abs(l64[j]))
        j = R.ALL_WON_CLIENT
        start = W64[j - 1] if chained else W0
        assert _same(W64[j], start) and l64[j] == 0.0
        if C >= 2:
            assert all(np.abs(W64[k] - (W64[k - 1] if chained and k else W0)).max() >= 2.0 ** -5
                       for k in range(len(Xs)) if k != j)
            assert all(0 in y and C - 1 in y for y in ys)


# --------------------------------------------------------------------------- saturated Z
@pytest.mark.parametrize('N,C,Bv', [(10, 2, 16), (16, 4, 16), (5, 3, 8), (100, 10, 16), (37, 20, 16), (23, 5, 32),
                                    (300, 4, 16), (1000, 10, 16)]
                         + sorted({c[1:4] for c in R.SAT_SOLVE_CASES}))
def test_saturated_solve_step_is_exact_in_float32(N, C, Bv):
    """One step (nv == Bv, a power of two, buf = None, lr = 2^-10): logits exact in any order,
    and the fp32 oracle's p and buf bitwise the float64 reference's."""
    Z, y, p0 = R.saturated_solve_inputs(N, C, Bv)
    assert float(p0.astype(np.float64).sum()) == 1.0
    if N >= 4:
        assert (p0 == 0).any() and (p0 < 0).any()
    out64 = np.einsum('ncv,n->vc', Z.astype(np.float64), p0.astype(np.float64))
    out32 = np.einsum('ncv,n->vc', Z, p0)
    perm = np.random.RandomState(2).permutation(N)
    assert np.array_equal(out32.astype(np.float64), out64)
    assert np.array_equal(np.einsum('ncv,n->vc', Z[perm], p0[perm]), out32)
    acc = np.zeros_like(out32)
    for n in range(N - 1, -1, -1):
        acc = (acc + (Z[n].T * p0[n]).astype(F32)).astype(F32)
    assert np.array_equal(acc, out32)
    s = np.sort(out64, axis=1)
    assert (s[:, -1] - s[:, -2]).min() >= 200.0
    torch.manual_seed(7)
    p64, b64 = R.solve_ref64(Z, y, p0, None, R.LR_P_SAT, 1, Bv)
    torch.manual_seed(7)
    p32, b32 = O.mixture_solve_z(Z, y, p0, None, R.LR_P_SAT, 1, Bv)
    assert _same(p32, p64) and _same(b32, b64)
    assert np.abs(b64).max() > 1.0 and 0 in y and C - 1 in y          # the step moves p


# --------------------------------------------------------------------------- mixed: conditioning
@pytest.mark.parametrize('case', R.MIXED_TRAIN_CASES, ids=R.id_of)
def test_mixed_training_cases_are_well_conditioned(case):
    """The fp32 oracle within a quarter of the GPU test's bound of the float64 reference, on the
    GPU test's own inputs, chained and parallel (forms that only run parallel: parallel)."""
    form, G, D, C, B = case
    Xs, ys, W0 = R.mixed_train_inputs(*case)
    on = R.mixed_terms(case)
    args = (R.mixed_train_lr(case), 2, B, on, R.MU, on, R.LAM)
    worst = 0.0
    for chained in ((False,) if form in R.PARALLEL_ONLY_FORMS else (False, True)):
        torch.manual_seed(11)
        W64, l64, _ = R.train_chain_ref64(Xs, ys, W0, *args, chained)
        torch.manual_seed(11)
        W32, l32 = R.train_chain_f32(Xs, ys, W0, *args, chained)
        for j in range(len(Xs)):
            assert np.isfinite(W64[j]).all() and np.isfinite(l64[j])
            eW = np.abs(W32[j] - W64[j]).max() / (R.TOL * max(1.0, np.abs(W64[j]).max()))
            el = abs(l32[j] - l64[j]) / (R.TOL * max(1.0, abs(l64[j])))
            worst = max(worst, eW, el)
            assert np.abs(W64[j] - W0).max() > 100 * R.TOL * max(1.0, np.abs(W64[j]).max())    # it trains
    print('%s: fp32 oracle at %.4f of the bound' % (R.id_of(case), worst))
    assert worst <= R.QUARTER, worst


@pytest.mark.parametrize('case', R.MIXED_SOLVE_CASES, ids=R.id_of)
def test_mixed_solve_cases_are_well_conditioned(case):
    solver, N, C, nv, Bv, _ = case
    Z, y, p0, lr = R.mixed_solve_inputs(N, C, nv, Bv)
    assert nv % Bv != 0 and nv <= 210
    p64, b64, p32, b32 = p0, None, p0, None
    worst = 0.0
    for rnd in range(2):
        torch.manual_seed(70 + rnd)
        p64, b64 = R.solve_ref64(Z, y, p64, b64, lr, 2, Bv)
        torch.manual_seed(70 + rnd)
        p32, b32 = O.mixture_solve_z(Z, y, p32, b32, lr, 2, Bv)
        ep = np.abs(p32 - p64).max() / np.abs(p64).max() / R.P_TOL
        eb = np.abs(b32 - b64).max() / np.abs(b64).max() / R.BUF_TOL
        worst = max(worst, ep, eb)
    print('%s: fp32 oracle at %.4f of the bound; p moved by %.3g of its largest entry'
          % (R.id_of(case), worst, np.abs(p64 - p0).max() / np.abs(p64).max()))
    assert worst <= R.QUARTER, worst
    assert np.abs(p64 - p0).max() > 10 * R.P_TOL * np.abs(p64).max()         # p moved: not a vacuous check
    # winner margins of the saturated rows stay at 110 or more through the rescaling
    out = np.einsum('ncv,n->vc', Z.astype(np.float64), p0.astype(np.float64))
    sat = (np.arange(nv) % 3 == 1) & (np.arange(nv) % 7 != 3)
    s = np.sort(out[sat], axis=1)
    assert (s[:, -1] - s[:, -2]).min() >= 110.0


# --------------------------------------------------------------------------- coverage
@pytest.mark.parametrize('case', R.MIXED_TRAIN_CASES, ids=R.id_of)
def test_mixed_training_inputs_cover_their_rows(case):
    """Labels include class 0 and C - 1; tie rows, saturated rows labelled with the winner and
    saturated rows labelled with a loser occur in every batch-sized window of every client;
    ragged sizes; rows of one batch sit at all five offsets."""
    form, G, D, C, B = case
    Xs, ys, W0 = R.mixed_train_inputs(*case)
    assert {len(y) % B for y in ys} == {1, 7, B - 3} and max(len(y) for y in ys) <= 128
    for X, y in zip(Xs, ys):
        z = X.astype(np.float64) @ W0.astype(np.float64).T
        assert np.array_equal((X @ W0.T).astype(np.float64), z)        # exact first-step logits
        assert 0 in y and C - 1 in y
        s = np.sort(z, axis=1)
        gap = s[:, -1] - s[:, -2]
        tie = (z == z[:, :1]).all(axis=1)
        won = gap >= 88.0                    # every loser's exp(z - m) below the fp32 normal range
        lab = np.argmax(z, axis=1) == y
        i = np.arange(len(y))
        assert tie[i % 7 == 3].all() and np.array_equal(won, (i % 3 == 1) & (i % 7 != 3))
        for w0 in range(0, len(y) - B + 1):
            w = slice(w0, w0 + B)
            assert (i[w] % 7 == 3).any() and (won[w] & lab[w]).any() and (won[w] & ~lab[w]).any(), w0
    zt = np.concatenate([X[np.arange(len(X)) % 7 == 3] @ W0.T for X in Xs])
    assert len(set(zt[:, 0])) == 5                # ties at every offset


@pytest.mark.parametrize('case', R.MIXED_SOLVE_CASES, ids=R.id_of)
def test_mixed_solve_inputs_cover_their_rows(case):
    solver, N, C, nv, Bv, _ = case
    Z, y, p0, _ = R.mixed_solve_inputs(N, C, nv, Bv)
    out = np.einsum('ncv,n->vc', Z.astype(np.float64), p0.astype(np.float64))
    assert np.array_equal(np.einsum('ncv,n->vc', Z, p0).astype(np.float64), out)
    assert 0 in y and C - 1 in y and float(p0.astype(np.float64).sum()) == 1.0
    s = np.sort(out, axis=1)
    tie = (out == out[:, :1]).all(axis=1)
    won = (s[:, -1] - s[:, -2]) >= 110.0
    lab = np.argmax(out, axis=1) == y
    v = np.arange(nv)
    assert tie[v % 7 == 3].all() and np.array_equal(won, (v % 3 == 1) & (v % 7 != 3))
    assert (won & lab).any() and (won & ~lab).any()
    # rows whose every logit is below -104: a softmax whose maximum is a padded slot's 0 underflows
    # on them (exp = 0 for every class, 0 / 0); the N = 1000 cases run at a quarter of the offsets
    # and leave that to the smaller case of their solver family
    assert (out.max(axis=1) < (-104.0 if N <= 300 else -16.0)).any()


def test_a_plain_softmax_overflows_on_these_inputs():
    """exp(z) without the maximum subtracted is inf in fp32 on the saturated rows (the plain
    formula NaN), and a zero in a padded class slot would win the maximum of a row at a negative
    offset: the inputs tell both mistakes apart from the reference."""
    Xs, ys, W0 = R.saturated_train_inputs('single', 1, 200, 10, 32)
    z = Xs[0] @ W0.T
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(z)).any()
    Xs, ys, W0 = R.mixed_train_inputs('single', 1, 200, 10, 32)
    z = Xs[0] @ W0.T
    assert (z.max(axis=1) < -104.0).any()

"""CPU checks of tests/local_eval_reference.py: the segment reference equals
``eval_reference.ce_acc_ref`` on the sliced arrays, the n_j-weighted sum of the segment losses is
the pooled mean (the objective F(W_g)), and the sweep holds every boundary it claims."""
import numpy as np

from tests.eval_reference import ce_acc_ref, exact_problem, tied_rows
from tests.local_eval_reference import (FIN_THREADS, GROUP, MANY, SINGLES, SIZES9, SWEEP_C, SWEEP_LD, case_seed,
                                        client_models, groups, many_sizes, mse_targets, objective, offsets,
                                        partitions, segment_mse_ref, segment_ref, sweep_cases, ws_doubles)


def _problem(sizes, D, C, seed=0):
    return exact_problem(np.random.RandomState(seed), int(sum(sizes)), D, C)


def test_segments_equal_the_reference_on_slices():
    sizes, D, C = SIZES9, 27, 10
    X, y, W, _ = _problem(sizes, D, C)
    off = offsets(sizes)
    rows, loss, correct = segment_ref(X, y, sizes, W)
    Wn = client_models(W, len(sizes))
    rows_o, loss_o, correct_o = segment_ref(X, y, sizes, Wn)
    for j, n in enumerate(sizes):
        a, b = off[j], off[j + 1]
        assert b - a == n == len(rows[j]) == len(rows_o[j])
        r, l, c = ce_acc_ref(X[a:b], y[a:b], W)
        assert np.allclose(rows[j], r, rtol=1e-13, atol=1e-13) and abs(loss[j] - l) <= 1e-13 * max(1.0, l)
        assert correct[j] == c
        r, l, c = ce_acc_ref(X[a:b], y[a:b], Wn[j])
        assert np.array_equal(rows_o[j], r) and loss_o[j] == l and correct_o[j] == c
    assert not np.array_equal(loss[1:], loss_o[1:])            # the per-client models differ
    assert np.array_equal(Wn[0], W)


def test_weighted_sum_is_the_pooled_mean():
    for sizes in (SIZES9, many_sizes(np.random.RandomState(1), 300, 20, 40)):
        X, y, W, _ = _problem(sizes, 27, 7, seed=2)
        _, loss, correct = segment_ref(X, y, sizes, W)
        _, pooled, pooled_correct = ce_acc_ref(X, y, W)
        assert abs(objective(loss, sizes) - pooled) <= 1e-14 * pooled
        assert int(correct.sum()) == pooled_correct
        w = W[0]
        t = mse_targets(np.random.RandomState(3), X, w)
        mse, acc = segment_mse_ref(X, t, sizes, w)
        r = X.astype(np.float64) @ w.astype(np.float64) - t
        assert abs(objective(mse, sizes) - float((r * r).mean())) <= 1e-14 * float((r * r).mean())
        assert abs(objective(acc, sizes) - 100.0 * float((t == 0).mean())) <= 1e-12


def test_mse_reference_on_slices():
    sizes = SIZES9
    X, _, W, _ = _problem(sizes, 91, 1, seed=4)
    ws = client_models(W, len(sizes))[:, 0, :]
    t = mse_targets(np.random.RandomState(5), X, W[0])
    assert (t[::4] == 0).all() and (t != 0).any()
    mse, acc = segment_mse_ref(X, t, sizes, ws)
    off = offsets(sizes)
    for j in range(len(sizes)):
        a, b = off[j], off[j + 1]
        r = X[a:b].astype(np.float64) @ ws[j].astype(np.float64) - t[a:b]
        assert mse[j] == float((r * r).mean()) and acc[j] == 100.0 * float((t[a:b] == 0).sum()) / (b - a)


def test_rolled_models_keep_ties_and_exactness():
    """client_models: a row's tied maximum stays tied under every client's model, and the
    logits stay exact (integers times one power of two)."""
    sizes, D, C = SIZES9, 27, 10
    X, y, W, info = _problem(sizes, D, C, seed=6)
    assert info['tied'] >= 10
    Wn = client_models(W, len(sizes))
    z0 = X.astype(np.float64) @ W.astype(np.float64).T
    for j in range(len(sizes)):
        z = X.astype(np.float64) @ Wn[j].astype(np.float64).T
        assert np.array_equal(z, np.roll(z0, j, axis=1) * 2.0 ** -(j % 3))
        assert tied_rows(z, y)[0] == info['tied']
        assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    # tied rows fall into several clients, so a last-maximum arg-max changes several counts
    off = offsets(sizes)
    tied = np.nonzero((z0 == z0.max(axis=1, keepdims=True)).sum(axis=1) > 1)[0]
    assert len({int(np.searchsorted(off, v, side='right')) for v in tied}) >= 3


def test_sweep_holds_every_boundary():
    assert SIZES9 == (1, 15, 16, 17, 31, 33, 16, 1, 257)
    assert {1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP + 1} <= set(SIZES9)
    assert max(SIZES9) == GROUP * GROUP + 1                    # 17 groups, the last of one row
    i = SIZES9.index(GROUP, 3)
    assert SIZES9[i - 1] % GROUP and SIZES9[i + 1] == 1        # a full group between ragged neighbours
    starts = offsets(SIZES9)[:-1] % GROUP                      # clients start on AND off the pooled 16-row grid
    assert (starts[1:] == 0).sum() >= 1 and (starts != 0).sum() >= 5
    assert SINGLES == (1, 4113) and groups((4113,)) == FIN_THREADS + 2
    assert partitions() == (SIZES9, (1,), (4113,))
    assert SWEEP_C == (1, 2, 10, 16, 17, 32)
    assert SWEEP_LD == ((64, 64 - 37), (128, 128 - 37), (2048, 2048))
    cases = sweep_cases()
    assert len(cases) == len(set(cases)) == 3 * 3 * 6
    assert {(s, ld, C) for s, ld, _, C in cases} == {(s, ld, C) for s in partitions() for ld, _ in SWEEP_LD
                                                     for C in SWEEP_C}
    assert len({case_seed(*c) for c in cases}) == len(cases)
    assert MANY == ((300, 20, 40), (3000, 1, 1))
    sizes = many_sizes(np.random.RandomState(0), 300, 20, 40)
    assert len(sizes) == 300 and min(sizes) >= 20 and max(sizes) <= 40 and groups(sizes) > 256   # > the CUs
    assert groups(SIZES9) == 1 + 1 + 1 + 2 + 2 + 3 + 1 + 1 + 17


def test_workspace_formula_covers_the_groups():
    rs = np.random.RandomState(7)
    for sizes in (SIZES9, (1,), (4113,), (16,) * 40, (1,) * 3000, many_sizes(rs, 300, 20, 40), (17, 1, 15)):
        N, total = len(sizes), int(sum(sizes))
        need = ws_doubles(total, N)
        assert need == (N + 2) // 2 + 2 * (total // 16 + N)
        assert 8 * ((N + 2) // 2) >= 4 * (N + 1)               # the int32 prefix fits its doubles
        assert groups(sizes) <= total // 16 + N                # every group has its pair

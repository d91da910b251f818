"""CPU checks of tests/eval_reference.py: the inputs really are exact in fp32, the loss bound
holds for the kernel's formula run in numpy float32, and every sweep of tests/test_gpu_eval.py
exercises the arg-max tie rule on purpose."""
import numpy as np
import pytest

from tests.eval_reference import (BIG_C, BIG_LD, BIG_N, SWEEP_TILES, case_seed, ce_acc_ref, exact_problem,
                                  kernel_formula_f32, loss_bound, sweep_cases, tied_rows)


def _problem(case, **kw):
    n, D, ld, C = case
    return exact_problem(np.random.RandomState(case_seed(*case)), n, D, C, **kw)


ALL_SWEEPS = [('tiles%d' % t, sweep_cases(t)) for t in SWEEP_TILES] + \
             [('big', [(BIG_N, BIG_LD, BIG_LD, C) for C in BIG_C])]


@pytest.mark.parametrize('case', [(33, 27, 64, 17), (17, 1563, 1600, 32), (16, 2112, 2112, 15), (70, 4160, 4160, 10)])
@pytest.mark.parametrize('spread', [20.0, 150.0])
def test_exact_problem_is_exact_in_any_order(case, spread):
    """The fp32 matmul, the float64 matmul and the fp32 matmul with permuted columns agree
    bitwise: no summation order can move a logit."""
    X, y, W, info = _problem(case, spread=spread)
    assert X.dtype == np.float32 and W.dtype == np.float32
    z32 = X @ W.T
    z64 = X.astype(np.float64) @ W.astype(np.float64).T
    perm = np.random.RandomState(1).permutation(X.shape[1])
    zp = X[:, perm] @ W[:, perm].T
    assert z32.dtype == np.float32 and np.array_equal(z32.astype(np.float64), z64) and np.array_equal(zp, z32)
    # one by one from the last column backwards, in float32
    acc = np.zeros_like(z32)
    for d in range(X.shape[1] - 1, -1, -1):
        acc = (acc + np.outer(X[:, d], W[:, d]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(acc, z32)
    assert 0 in y and (len(y) < 2 or case[3] - 1 in y)
    assert np.array_equal(np.round(z64 / info['quantum']) * info['quantum'], z64)


@pytest.mark.parametrize('name,cases', ALL_SWEEPS + [('stability', [(33, 1000, 1024, 10)])])
def test_kernel_formula_in_float32_meets_the_loss_bound(name, cases):
    """-(z_y - m - log(sum exp(z - m))) in numpy float32 stays inside loss_bound of the float64
    reference, case by case: the bound holds for the reference's own arithmetic."""
    worst = 0.0
    for case in cases:
        X, y, W, _ = _problem(case, spread=150.0 if name == 'stability' else 20.0)
        ce, loss, _ = ce_acc_ref(X, y, W)
        got = float(kernel_formula_f32(X @ W.T, y).mean())
        bound = loss_bound(case[3], ce)
        assert np.isfinite(got) and abs(got - loss) <= bound, (case, got, loss, bound)
        worst = max(worst, abs(got - loss) / bound)
    print('%s: worst |loss - ref| / bound = %.3f' % (name, worst))


@pytest.mark.parametrize('name,cases', ALL_SWEEPS)
def test_every_sweep_ties_both_ways(name, cases):
    """Each sweep holds rows with a tied maximum labelled with the lower tied class (correct
    under the lowest-index rule) and rows labelled with the higher one (wrong under it), and in
    every case with 15 rows or more and two classes or more the correct count under a
    last-maximum rule differs from the reference's."""
    low = high = told = 0
    for case in cases:
        X, y, W, info = _problem(case)
        z = X.astype(np.float64) @ W.astype(np.float64).T
        t, tl, th = tied_rows(z, y)
        assert (t, tl, th) == (info['tied'], info['tied_low'], info['tied_high'])
        low, high = low + tl, high + th
        # the one figure fs_eval reports, the correct count, must tell the two rules apart
        last = z.shape[1] - 1 - np.argmax(z[:, ::-1], axis=1)
        differs = int((last == y).sum()) != ce_acc_ref(X, y, W)[2]
        told += differs
        if case[0] >= 15 and case[3] >= 2:
            assert differs, case
    print('%s: %d rows tied on the lower label, %d on the higher; a last-maximum rule miscounts %d of %d cases'
          % (name, low, high, told, len(cases)))
    assert low >= 1 and high >= 1


def test_stability_case_overflows_a_plain_softmax():
    """At spread 150 the logits pass +-150: exp(z) without the maximum subtracted is inf in fp32
    (and the plain formula NaN), while the reference stays finite."""
    X, y, W, _ = _problem((33, 1000, 1024, 10), spread=150.0)
    z = X @ W.T
    assert z.max() >= 150.0 and z.min() <= -150.0
    with np.errstate(over='ignore', invalid='ignore'):
        assert np.isinf(np.exp(z)).any()
    assert np.isfinite(ce_acc_ref(X, y, W)[0]).all()

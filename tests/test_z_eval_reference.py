"""CPU checks of tests/z_eval_reference.py: the fp32 emulation of z_eval.hip's per-row formula
stays within ``loss_bound`` of the float64 reference on every input tests/test_gpu_z_eval.py
uses, the sweep covers what it claims, and the saturated inputs have teeth."""
import numpy as np
import pytest

from tests.z_eval_reference import (SWEEP_C, SWEEP_N, SWEEP_ROWS, ZE_ROWS, ZE_TILE, ZF_CLIENTS, ZF_STRIDES, bounds,
                                    case_seed, from_layout, grid_logits, kernel_formula_f32, ldn, mse_ref,
                                    mse_values, per_client_ref, saturated_logits, sweep_cases, tied_logits,
                                    to_layout)

# the shapes of the tied and the saturated tests of tests/test_gpu_z_eval.py
TIED_CASES = ((33, 5, 3), (65, 33, 10), (17, 2, 2))
SAT_CASES = ((33, 5, 3), (65, 257, 7), (40, 6, 10))


def _within(Z, y, N, C):
    ce, loss, _ = per_client_ref(Z, y, N, C)
    _, got = kernel_formula_f32(Z, y, N, C)
    b = bounds(C, ce)
    assert np.isfinite(got).all()
    assert (np.abs(got - loss) <= b).all(), float((np.abs(got - loss) / b).max())


def test_sweep_covers_every_pair():
    cases = sweep_cases()
    assert len(cases) == len(SWEEP_N) * len(SWEEP_C)
    assert {(N, C) for _, N, C in cases} == {(N, C) for N in SWEEP_N for C in SWEEP_C}
    assert {(n, N) for n, N, _ in cases} == {(n, N) for n in SWEEP_ROWS for N in SWEEP_N}
    # the base lists, and one below / at / above every tile boundary of the kernel
    assert {1, 4, 5, 100, 255, 256, 257, 1000} <= set(SWEEP_N)
    assert {1, 2, 10, 16, 17, 32} <= set(SWEEP_C)
    assert {1, 15, 17, 33} <= set(SWEEP_ROWS)
    assert {ZE_ROWS - 1, ZE_ROWS, ZE_ROWS + 1, 2 * ZE_ROWS - 1, 2 * ZE_ROWS, 2 * ZE_ROWS + 1} <= set(SWEEP_ROWS)
    assert {ZE_TILE - 1, ZE_TILE, ZE_TILE + 1, ZF_CLIENTS - 1, ZF_CLIENTS, ZF_CLIENTS + 1} <= set(SWEEP_N)
    assert max(SWEEP_ROWS) > ZF_STRIDES * ZE_ROWS          # the finaliser's second stride


def test_layout_round_trip():
    rs = np.random.RandomState(0)
    A = rs.normal(size=(7, 5, 3)).astype(np.float32)
    Z = to_layout(A, pad=np.nan)
    assert Z.shape == (7, 3 * ldn(5)) and ldn(5) == 8
    assert np.array_equal(from_layout(Z, 5, 3), A)
    assert np.isnan(Z.reshape(7, 3, 8)[:, :, 5:]).all()


def test_emulation_within_bound_on_the_sweep():
    for case in sweep_cases():
        n, N, C = case
        if n * N * C > 2_000_000:       # the largest shapes: the same generator at fewer clients
            N = 40
        Z, y = grid_logits(np.random.RandomState(case_seed(*case)), n, N, C)
        _within(Z, y, N, C)


@pytest.mark.parametrize('case', TIED_CASES)
def test_tied_inputs(case):
    n, N, C = case
    Z, y, info = tied_logits(np.random.RandomState(case_seed(*case)), n, N, C)
    _within(Z, y, N, C)
    ce, loss, correct = per_client_ref(Z, y, N, C)
    assert correct[0] == info['flat_correct'] == int((y == 0).sum())
    assert np.abs(ce[0] - np.log(C)).max() < 1e-12
    assert info['tied_low'] >= 1 and (n < 8 or info['tied_high'] >= 1)
    # a kernel that takes the LAST maximum counts another number of correct rows for client 1
    A = from_layout(Z, N, C)[:, 1, :]
    last = C - 1 - np.argmax(A[:, ::-1], axis=1)
    assert int((last == y).sum()) != correct[1]


@pytest.mark.parametrize('case', SAT_CASES)
def test_saturated_inputs_have_teeth(case):
    n, N, C = case
    assert C & (C - 1), 'C must not be a power of two'
    Z, y, info = saturated_logits(np.random.RandomState(case_seed(*case)), n, N, C)
    A = from_layout(Z, N, C)
    assert np.array_equal(A, np.round(A))                      # integers
    srt = np.sort(A, axis=2)
    assert (srt[:, :, -1] - srt[:, :, -2] >= 200).all()        # winners lead by >= 200
    neg = info['negative_rows']
    assert len(neg) >= 2 and (A[neg] < 0).all()
    _within(Z, y, N, C)
    ce, loss, correct = per_client_ref(Z, y, N, C)
    ce32, loss32 = kernel_formula_f32(Z, y, N, C)
    assert correct[0] == n and (ce32[0] == 0.0).all() and loss32[0] == 0.0
    # the maximum not subtracted: exp overflows / underflows, the loss is inf or NaN
    _, bad = kernel_formula_f32(Z, y, N, C, subtract_max=False)
    assert not np.isfinite(bad).any()
    # a padded class slot entering the maximum as 0: all-negative rows lose their sum
    cep, badp = kernel_formula_f32(Z, y, N, C, pad_slot=True)
    assert not (np.abs(badp - loss) <= bounds(C, ce)).any()
    deep = [v for v in neg if A[v].max() < -104]               # exp(z) is 0 in fp32 below about -103.3
    assert len(deep) >= 1 and not np.isfinite(cep[:, deep]).any()


def test_mse_reference():
    Z, y = mse_values(np.random.RandomState(3), 33, 5)
    mse, acc = mse_ref(Z, y, 5)
    assert acc == 100.0 * 11 / 33
    z32 = Z[:, :5]
    r = (z32 - y[:, None]).astype(np.float32)
    got = (r * r).astype(np.float32).astype(np.float64).mean(axis=0)
    assert (np.abs(got - mse) <= 2.0 ** -22 * mse).all()

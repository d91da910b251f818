"""fs_z_eval_* (csrc/z_eval.hip), the per-client evaluation, at the kernel level: Z is built on
the host and uploaded, so the kernel is tested apart from the GEMM, against a float64 reference
from the same fp32 Z (tests/z_eval_reference.py).  The logits are integers times a power of two,
so what is left of the kernel's error is its softmax arithmetic: the loss is held to
``eval_reference.loss_bound`` (derived there: exact logits in, exp / log within 4 ulp) and the
correct count EXACTLY.  MSE: |mse - ref| <= 2^-22 ref (the fp32 difference and square are under
4 u relative per row, the fp64 accumulation adds parts in 2^-53); the accuracy value exact.

The sweep's boundaries come from the kernel's tile constants, restated in z_eval_reference.py
(ZE_ROWS, ZE_TILE, ZE_UNROLL, ZF_STRIDES, ZF_CLIENTS).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import amd  # noqa: F401 (fixture)
from tests.test_z_eval_reference import SAT_CASES, TIED_CASES
from tests.z_eval_reference import (ZE_ROWS, bounds, case_seed, from_layout, grid_logits, ldn, mse_ref, mse_values,
                                    per_client_ref, saturated_logits, sweep_cases, tied_logits, to_layout)

pytestmark = pytest.mark.gpu

CANARY = -12345.678


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def z_eval(amd, Z, y, N, C, mse=False, chunk=None):
    """fs_z_eval_add[_mse] (in chunks of ``chunk`` rows if given) + fs_z_eval_finish on host
    arrays; canaries behind the 2 N doubles of ``out`` and behind the workspace are checked.
    Returns out [N, 2] (numpy float64)."""
    L, dev = amd.lib.lib(), torch.device('cuda')
    n = Z.shape[0]
    Zd = torch.from_numpy(np.ascontiguousarray(Z)).to(dev)
    yd = torch.from_numpy(np.asarray(y, np.float32 if mse else np.int32)).to(dev)
    need = int(L.fs_z_eval_ws_doubles(n, N))
    assert need == (n + ZE_ROWS - 1) // ZE_ROWS * ldn(N) * 2
    ws = torch.full((need + 8,), CANARY, dtype=torch.float64, device=dev)
    out = torch.full((2 * N + 8,), CANARY, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for row0 in range(0, n, chunk or n):
        rows = min(chunk or n, n - row0)
        if mse:
            rc = L.fs_z_eval_add_mse(_ptr(Zd[row0:]), _ptr(yd), n, row0, rows, N, _ptr(ws), need, st)
        else:
            rc = L.fs_z_eval_add(_ptr(Zd[row0:]), _ptr(yd), n, row0, rows, N, C, _ptr(ws), need, st)
        assert rc == 0, L.fs_last_error()
    assert L.fs_z_eval_finish(_ptr(ws), need, n, N, _ptr(out), st) == 0, L.fs_last_error()
    o = out.cpu().numpy()
    assert (o[2 * N:] == CANARY).all(), 'fs_z_eval_finish wrote behind out[2 N]'
    assert (ws[need:].cpu().numpy() == CANARY).all(), 'fs_z_eval_add wrote behind its workspace'
    return o[:2 * N].reshape(N, 2).copy()


def _check(amd, Z, y, N, C, chunk=None):
    """Loss within loss_bound per client, accuracy exactly 100 correct / n; returns the worst
    |dloss| / bound and the result."""
    n = Z.shape[0]
    ce, loss, correct = per_client_ref(Z, y, N, C)
    got = z_eval(amd, Z, y, N, C, chunk=chunk)
    b = bounds(C, ce)
    frac = np.abs(got[:, 0] - loss) / b
    print('n %d N %d C %d: worst |dloss| / bound %.3f' % (n, N, C, frac.max()))
    assert np.isfinite(got).all() and (frac <= 1.0).all(), (n, N, C, float(frac.max()))
    assert np.array_equal(got[:, 1], 100.0 * correct / n), (n, N, C)
    return float(frac.max()), got


def test_block_rows_constant(amd):
    assert amd.lib.lib().fs_z_eval_block_rows() == ZE_ROWS


@pytest.mark.parametrize('N', sorted({N for _, N, _ in sweep_cases()}))
def test_structural_sweep(amd, N):
    """Every client count with every class count and every row count (sweep_cases)."""
    for case in (c for c in sweep_cases() if c[1] == N):
        n, _, C = case
        Z, y = grid_logits(np.random.RandomState(case_seed(*case)), n, N, C)
        _check(amd, Z, y, N, C)


def test_mse_sweep(amd):
    """The MSE twin at every client count and row count of the sweep (C = 1)."""
    for n, N, C in sweep_cases():
        if C != 1 and not (C == 2 and N in (5, 257)):      # each N once, two more row counts for two of them
            continue
        Z, y = mse_values(np.random.RandomState(case_seed(n, N, 1)), n, N)
        mse, acc = mse_ref(Z, y, N)
        got = z_eval(amd, Z, y, N, 1, mse=True)
        rel = np.abs(got[:, 0] - mse) / mse
        print('mse n %d N %d: worst relative error %.3g of 2^-22' % (n, N, rel.max() * 2.0 ** 22))
        assert (rel <= 2.0 ** -22).all(), (n, N, float(rel.max()))
        assert (got[:, 1] == acc).all(), (n, N)


@pytest.mark.parametrize('N', [5, 257])
def test_padding_is_ignored(amd, N):
    """The padding columns N..ldN-1 of every class segment filled with NaN: no result moves (the
    canary behind out[2 N] is checked by every call)."""
    n, C = 33, 3
    Z, y = grid_logits(np.random.RandomState(5), n, N, C)
    _, ref = _check(amd, Z, y, N, C)
    Zn = to_layout(from_layout(Z, N, C), pad=np.nan)
    assert np.isnan(Zn).sum() == n * C * (ldn(N) - N) > 0
    assert np.array_equal(z_eval(amd, Zn, y, N, C), ref)
    Zm, ym = mse_values(np.random.RandomState(6), n, N)
    Zmn = to_layout(from_layout(Zm, N, 1), pad=np.nan)
    assert np.array_equal(z_eval(amd, Zmn, ym, N, 1, mse=True), z_eval(amd, Zm, ym, N, 1, mse=True))


@pytest.mark.parametrize('case', TIED_CASES)
def test_ties_go_to_the_lowest_class(amd, case):
    """Client 0's C logits are equal in every row: exactly 100 #{y == 0} / n, loss log C within
    the bound.  Client 1's rows with two tied maxima are labelled low / high / low."""
    n, N, C = case
    Z, y, info = tied_logits(np.random.RandomState(case_seed(*case)), n, N, C)
    _, got = _check(amd, Z, y, N, C)
    assert got[0, 1] == 100.0 * info['flat_correct'] / n
    assert abs(got[0, 0] - np.log(C)) <= bounds(C, np.full((1, n), np.log(C)))[0]


@pytest.mark.parametrize('case', SAT_CASES)
def test_saturated_and_offset_rows(amd, case):
    """Integer logits at row offsets 0, +-64, +-128 with winners leading by >= 200 (some rows all
    negative, C no power of two): a row labelled with its winner contributes exactly 0.0, and
    client 0 -- only such rows -- reports loss exactly 0.0."""
    n, N, C = case
    Z, y, info = saturated_logits(np.random.RandomState(case_seed(*case)), n, N, C)
    _, got = _check(amd, Z, y, N, C)
    assert got[0, 0] == 0.0 and got[0, 1] == 100.0
    # every row contributes exactly 0 or its integer trail: n * loss is an integer
    assert np.array_equal(np.round(got[:, 0] * n), per_client_ref(Z, y, N, C)[0].sum(axis=1).round())


def test_column_independence(amd):
    """Models [A, B, C] against [C, A] and [A] alone: the same bits per model, whatever N, the
    position and the neighbours -- across a column-tile boundary too."""
    n, C = 65, 10
    rs = np.random.RandomState(11)
    Z, y = grid_logits(rs, n, 3, C)
    A3 = from_layout(Z, 3, C)
    abc = z_eval(amd, Z, y, 3, C)
    ca = z_eval(amd, to_layout(A3[:, [2, 0]]), y, 2, C)
    a = z_eval(amd, to_layout(A3[:, [0]]), y, 1, C)
    assert np.array_equal(ca[0], abc[2]) and np.array_equal(ca[1], abc[0]) and np.array_equal(a[0], abc[0])
    # the same three models at columns 255, 256 and 299 of 300
    Zw, _ = grid_logits(rs, n, 300, C)
    Aw = from_layout(Zw, 300, C).copy()
    Aw[:, [255, 256, 299]] = A3
    wide = z_eval(amd, to_layout(Aw), y, 300, C)
    assert np.array_equal(wide[[255, 256, 299]], abc)
    Zm, ym = mse_values(rs, n, 5)
    m5 = z_eval(amd, Zm, ym, 5, 1, mse=True)
    m2 = z_eval(amd, to_layout(from_layout(Zm, 5, 1)[:, [4, 1]]), ym, 2, 1, mse=True)
    assert np.array_equal(m2, m5[[4, 1]])


@pytest.mark.parametrize('n', [33, 8 * ZE_ROWS + 1])
def test_chunk_independence(amd, n):
    """One call against chunks of one row block (and of three): bitwise equal."""
    N, C = 5, 3
    Z, y = grid_logits(np.random.RandomState(n), n, N, C)
    whole = z_eval(amd, Z, y, N, C)
    assert np.array_equal(z_eval(amd, Z, y, N, C, chunk=ZE_ROWS), whole)
    assert np.array_equal(z_eval(amd, Z, y, N, C, chunk=3 * ZE_ROWS), whole)
    Zm, ym = mse_values(np.random.RandomState(n + 1), n, N)
    assert np.array_equal(z_eval(amd, Zm, ym, N, 1, mse=True, chunk=ZE_ROWS), z_eval(amd, Zm, ym, N, 1, mse=True))


def test_repeatable(amd):
    Z, y = grid_logits(np.random.RandomState(2), 8 * ZE_ROWS + 1, 257, 10)
    a = z_eval(amd, Z, y, 257, 10)
    for _ in range(2):
        assert np.array_equal(z_eval(amd, Z, y, 257, 10), a)


def test_argument_errors(amd):
    """Bad sizes, null pointers, a row0 off the row-block grid and a short workspace return a
    negative status and a message; nothing is launched."""
    L, dev = amd.lib.lib(), torch.device('cuda')
    n, N, C = 33, 5, 3
    Z = torch.zeros(n, C * ldn(N), device=dev)
    y = torch.zeros(n, dtype=torch.int32, device=dev)
    yf = torch.zeros(n, device=dev)
    need = int(L.fs_z_eval_ws_doubles(n, N))
    ws = torch.zeros(need, dtype=torch.float64, device=dev)
    out = torch.full((2 * N,), CANARY, dtype=torch.float64, device=dev)
    p = _ptr
    bad = [
        (lambda: L.fs_z_eval_add(p(Z), p(y), n, 0, n, N, 0, p(ws), need, None), 'num_classes'),
        (lambda: L.fs_z_eval_add(p(Z), p(y), n, 0, n, N, 33, p(ws), need, None), 'num_classes'),
        (lambda: L.fs_z_eval_add(p(Z), p(y), n, 0, n, 0, C, p(ws), need, None), 'N'),
        (lambda: L.fs_z_eval_add(p(Z), p(y), 0, 0, 0, N, C, p(ws), need, None), 'n'),
        (lambda: L.fs_z_eval_add(None, p(y), n, 0, n, N, C, p(ws), need, None), 'null'),
        (lambda: L.fs_z_eval_add(p(Z), None, n, 0, n, N, C, p(ws), need, None), 'null'),
        (lambda: L.fs_z_eval_add(p(Z), p(y), n, 0, n, N, C, None, need, None), 'null'),
        (lambda: L.fs_z_eval_add(p(Z), p(y), n, 0, n, N, C, p(ws), need - 1, None), 'workspace'),
        (lambda: L.fs_z_eval_add(p(Z), p(y), n, 8, 25, N, C, p(ws), need, None), 'row0'),
        (lambda: L.fs_z_eval_add(p(Z), p(y), n, 0, 8, N, C, p(ws), need, None), 'last chunk'),
        (lambda: L.fs_z_eval_add(p(Z), p(y), n, 32, 2, N, C, p(ws), need, None), 'rows'),
        (lambda: L.fs_z_eval_add_mse(p(Z), None, n, 0, n, N, p(ws), need, None), 'null'),
        (lambda: L.fs_z_eval_add_mse(p(Z), p(yf), n, 8, 25, N, p(ws), need, None), 'row0'),
        (lambda: L.fs_z_eval_add_mse(p(Z), p(yf), n, 0, n, N, p(ws), need - 1, None), 'workspace'),
        (lambda: L.fs_z_eval_finish(p(ws), need, n, 0, p(out), None), 'N'),
        (lambda: L.fs_z_eval_finish(None, need, n, N, p(out), None), 'null'),
        (lambda: L.fs_z_eval_finish(p(ws), need, n, N, None, None), 'null'),
        (lambda: L.fs_z_eval_finish(p(ws), need - 1, n, N, p(out), None), 'workspace'),
    ]
    for call, needle in bad:
        rc = call()
        assert rc < 0, needle
        assert needle in L.fs_last_error().decode(), (needle, L.fs_last_error())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all()
    assert L.fs_z_eval_ws_doubles(0, 5) == 0 and L.fs_z_eval_ws_doubles(5, 0) == 0

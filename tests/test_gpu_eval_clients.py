"""fs_eval_clients / fs_eval_clients_mse (csrc/eval_clients.hip), the local evaluation, at the
kernel level.  Contract A: client j's two doubles equal BITWISE what fs_eval (fs_eval_mse) returns
on the client's row slice with the client's model -- for one shared model (w_stride = 0) and for
one model per client (w_stride = C ld).  Inputs are ``eval_reference.exact_problem``'s: logits
exact in fp32 in any summation order, so against the float64 reference
(tests/local_eval_reference.py) the loss is held to ``eval_reference.loss_bound`` and the correct
count EXACTLY, rows with tied maxima included.  MSE: |mse - ref| <= 2^-22 ref, the bound
tests/test_gpu_z_eval.py derives (the dot products are exact; the fp32 residual rounds once, under
2 u relative on its square; the fp64 accumulation adds parts in 2^-53); the accuracy value exact.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.eval_reference import exact_problem, loss_bound
from tests.local_eval_reference import (MANY, SIZES9, SWEEP_C, SWEEP_LD, case_seed, client_models, many_sizes,
                                        mse_targets, offsets, partitions, segment_mse_ref, segment_ref, ws_doubles)
from tests.test_gpu_parity import amd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

CANARY = -12345.678


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Device:
    """One problem resident on the GPU: features padded to ld, targets, row offsets."""

    def __init__(self, X, y, sizes, ld, mse=False):
        dev = torch.device('cuda')
        self.sizes, self.N, self.ld, self.mse, self.D = tuple(int(n) for n in sizes), len(sizes), ld, mse, X.shape[1]
        self.rows = int(sum(sizes))
        assert X.shape[0] == self.rows
        self.phi = torch.zeros(self.rows, ld, device=dev)
        self.phi[:, :self.D] = torch.from_numpy(X)
        self.y = torch.from_numpy(np.asarray(y, np.float32 if mse else np.int32)).to(dev)
        self.off = offsets(sizes)
        self.row_off = torch.from_numpy(self.off).to(dev)
        self.h_n = np.ascontiguousarray(sizes, dtype=np.int64)

    def weights(self, W):
        """W [C, D] or [N, C, D] -> the padded device buffer and its w_stride."""
        W = np.asarray(W, np.float32)
        Wd = torch.zeros(W.shape[:-1] + (self.ld,), device=self.phi.device)
        Wd[..., :self.D] = torch.from_numpy(W)
        return Wd, (0 if W.ndim == 2 else W.shape[1] * self.ld)


def eval_clients(amd, P, Wd, stride, C, ws=None):
    """fs_eval_clients[_mse] on the problem P; canaries behind out[2 N] and behind ws[need] are
    checked, ``need`` against the documented formula.  Returns out [N, 2] (numpy float64)."""
    L, dev = amd.lib.lib(), P.phi.device
    need = int(L.fs_eval_clients_ws_doubles(P.rows, P.N))
    assert need == ws_doubles(P.rows, P.N)
    if ws is None:
        ws = torch.full((need + 8,), CANARY, dtype=torch.float64, device=dev)
    out = torch.full((2 * P.N + 8,), CANARY, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if P.mse:
        rc = L.fs_eval_clients_mse(_ptr(P.phi), P.ld, _ptr(P.row_off), P.h_n.ctypes.data, _ptr(P.y), P.N, _ptr(Wd),
                                   stride, _ptr(out), _ptr(ws), need, st)
    else:
        rc = L.fs_eval_clients(_ptr(P.phi), P.ld, _ptr(P.row_off), P.h_n.ctypes.data, _ptr(P.y), P.N, _ptr(Wd),
                               stride, C, _ptr(out), _ptr(ws), need, st)
    assert rc == 0, L.fs_last_error()
    o = out.cpu().numpy()
    assert (o[2 * P.N:] == CANARY).all(), 'fs_eval_clients wrote behind out[2 N]'
    assert (ws[need:].cpu().numpy() == CANARY).all(), 'fs_eval_clients wrote behind its workspace'
    return o[:2 * P.N].reshape(P.N, 2).copy()


def eval_slices(amd, P, Wd, stride, C):
    """The loop of N fs_eval (fs_eval_mse) calls on the row slices -> [N, 2]."""
    L, dev = amd.lib.lib(), P.phi.device
    out = torch.empty(P.N, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.fs_eval_ws_doubles(max(P.sizes))), dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flat = Wd.reshape(-1)
    for j in range(P.N):
        a, n = int(P.off[j]), P.sizes[j]
        Wj = flat[j * stride:]
        if P.mse:
            rc = L.fs_eval_mse(_ptr(P.phi[a:]), P.ld, _ptr(P.y[a:]), n, _ptr(Wj), _ptr(out[j]), _ptr(ws), st)
        else:
            rc = L.fs_eval(_ptr(P.phi[a:]), P.ld, _ptr(P.y[a:]), n, _ptr(Wj), C, _ptr(out[j]), _ptr(ws), st)
        assert rc == 0, L.fs_last_error()
    return out.cpu().numpy()


def _check_ce(tag, got, X, y, sizes, W, C):
    """Loss within loss_bound per client, 100 correct / n_j exactly."""
    rows, loss, correct = segment_ref(X, y, sizes, W)
    b = np.array([loss_bound(C, r) for r in rows])
    frac = np.abs(got[:, 0] - loss) / b
    print('%s: worst |dloss| / bound %.3f' % (tag, frac.max()))
    assert np.isfinite(got).all() and (frac <= 1.0).all(), (tag, float(frac.max()))
    assert np.array_equal(got[:, 1], 100.0 * correct / np.asarray(sizes, np.float64)), tag


def _check_mse(tag, got, X, t, sizes, w):
    mse, acc = segment_mse_ref(X, t, sizes, w)
    err = np.abs(got[:, 0] - mse)
    rel = err[mse > 0] / mse[mse > 0]
    print('%s: worst relative error %.3g of 2^-22' % (tag, rel.max() * 2.0 ** 22 if len(rel) else 0.0))
    assert (err <= 2.0 ** -22 * mse).all(), (tag, float((err - 2.0 ** -22 * mse).max()))
    assert np.array_equal(got[:, 1], acc), tag


@pytest.mark.parametrize('ld,D', SWEEP_LD)
@pytest.mark.parametrize('sizes', partitions(), ids=lambda s: 'n' + '_'.join(map(str, s[:3])))
def test_contract_a_and_float64_bound(amd, sizes, ld, D):
    """Every class count of the sweep on one partition and leading dimension: bitwise fs_eval on
    the slices, shared model and per-client models; loss_bound and exact counts against float64."""
    N = len(sizes)
    for C in SWEEP_C:
        rs = np.random.RandomState(case_seed(sizes, ld, D, C))
        X, y, W, info = exact_problem(rs, int(sum(sizes)), D, C)
        P = Device(X, y, sizes, ld)
        for tag, Wh in (('shared', W), ('own', client_models(W, N))):
            Wd, stride = P.weights(Wh)
            got = eval_clients(amd, P, Wd, stride, C)
            assert np.array_equal(got, eval_slices(amd, P, Wd, stride, C)), (tag, sizes, ld, C)
            _check_ce('%s N %d rows %d ld %d C %d (%d tied)' % (tag, N, P.rows, ld, C, info['tied']), got, X, y,
                      sizes, Wh, C)


@pytest.mark.parametrize('ld,D', SWEEP_LD)
def test_mse_contract_a_and_bound(amd, ld, D):
    """fs_eval_clients_mse: bitwise fs_eval_mse on the slices, 2^-22 against float64."""
    for sizes in partitions():
        N = len(sizes)
        rs = np.random.RandomState(case_seed(sizes, ld, D, 1))
        X, _, W, _ = exact_problem(rs, int(sum(sizes)), D, 1)
        t = mse_targets(rs, X, W[0])
        P = Device(X, t, sizes, ld, mse=True)
        for tag, Wh in (('shared', W), ('own', client_models(W, N))):
            Wd, stride = P.weights(Wh)
            got = eval_clients(amd, P, Wd, stride, 1)
            assert np.array_equal(got, eval_slices(amd, P, Wd, stride, 1)), (tag, sizes, ld)
            _check_mse('mse %s N %d rows %d ld %d' % (tag, N, P.rows, ld), got, X, t, sizes,
                       Wh[0] if Wh.ndim == 2 else Wh[:, 0, :])


@pytest.mark.parametrize('mse', [False, True])
def test_independence(amd, mse):
    """Client j's two doubles in the 9-client partition, with the same clients reversed, and as
    the only client: the same bits -- whatever N, the position and the neighbours."""
    ld, D, C = 128, 91, 1 if mse else 10
    N = len(SIZES9)
    rs = np.random.RandomState(17)
    X, y, W, _ = exact_problem(rs, int(sum(SIZES9)), D, C)
    if mse:
        y = mse_targets(rs, X, W[0])
    Wn = client_models(W, N)
    off = offsets(SIZES9)
    P = Device(X, y, SIZES9, ld, mse)
    fwd = eval_clients(amd, P, *P.weights(Wn), C)
    order = list(range(N))[::-1]
    Xr = np.concatenate([X[off[j]:off[j + 1]] for j in order])
    yr = np.concatenate([y[off[j]:off[j + 1]] for j in order])
    Pr = Device(Xr, yr, [SIZES9[j] for j in order], ld, mse)
    rev = eval_clients(amd, Pr, *Pr.weights(Wn[order]), C)
    assert np.array_equal(rev[::-1], fwd)
    for j in range(N):
        P1 = Device(X[off[j]:off[j + 1]], y[off[j]:off[j + 1]], [SIZES9[j]], ld, mse)
        alone = eval_clients(amd, P1, *P1.weights(Wn[j:j + 1]), C)
        assert np.array_equal(alone[0], fwd[j]), j
    assert len({tuple(r) for r in fwd}) == N           # nine different results, so the order matters


@pytest.mark.parametrize('N,lo,hi', MANY)
def test_many_clients(amd, N, lo, hi):
    """More workgroups than CUs (300 clients of 20-40 rows) and 3000 clients of one row each:
    the binary search over the group prefix at depth, and the prefix kernel with several clients
    per thread.  Against the float64 reference, both model sets, CE and MSE."""
    ld, D, C = 64, 27, 10
    rs = np.random.RandomState(N)
    sizes = many_sizes(rs, N, lo, hi)
    X, y, W, _ = exact_problem(rs, int(sum(sizes)), D, C)
    P = Device(X, y, sizes, ld)
    for tag, Wh in (('shared', W), ('own', client_models(W, N))):
        got = eval_clients(amd, P, *P.weights(Wh), C)
        _check_ce('many %s N %d' % (tag, N), got, X, y, sizes, Wh, C)
    Xm, _, Wm, _ = exact_problem(rs, int(sum(sizes)), D, 1)
    t = mse_targets(rs, Xm, Wm[0])
    Pm = Device(Xm, t, sizes, ld, mse=True)
    Wh = client_models(Wm, N)
    got = eval_clients(amd, Pm, *Pm.weights(Wh), 1)
    _check_mse('many mse N %d' % N, got, Xm, t, sizes, Wh[:, 0, :])


def test_repeated_calls_into_one_workspace(amd):
    """The workspace holds nothing between calls: a second problem through the same workspace,
    then the first again -- the same bits as with a fresh one."""
    L, ld, D, C = amd.lib.lib(), 128, 91, 17
    rs = np.random.RandomState(3)
    X, y, W, _ = exact_problem(rs, int(sum(SIZES9)), D, C)
    P = Device(X, y, SIZES9, ld)
    Wd, stride = P.weights(client_models(W, P.N))
    first = eval_clients(amd, P, Wd, stride, C)
    need = int(L.fs_eval_clients_ws_doubles(P.rows, P.N))
    ws = torch.full((need + 8,), CANARY, dtype=torch.float64, device=P.phi.device)
    assert np.array_equal(eval_clients(amd, P, Wd, stride, C, ws=ws), first)
    Pr = Device(X, y, SIZES9[::-1], ld)               # other boundaries, the same row total and N
    other = eval_clients(amd, Pr, Wd, stride, C, ws=ws)
    assert not np.array_equal(other, first)
    for _ in range(2):
        assert np.array_equal(eval_clients(amd, P, Wd, stride, C, ws=ws), first)


def test_argument_errors(amd):
    """C = 33, ld = 96, null pointers, a short workspace and a client with n_j = 0: a negative
    status and a message, nothing launched (the output keeps its canaries)."""
    L, dev = amd.lib.lib(), torch.device('cuda')
    sizes, ld, C = (5, 17, 3), 64, 3
    N, rows = len(sizes), sum(sizes)
    phi = torch.zeros(rows, 128, device=dev)
    y = torch.zeros(rows, dtype=torch.int32, device=dev)
    yf = torch.zeros(rows, device=dev)
    W = torch.zeros(N, 33, 128, device=dev)
    off = torch.from_numpy(offsets(sizes)).to(dev)
    h_n = np.ascontiguousarray(sizes, dtype=np.int64)
    h_zero = np.ascontiguousarray((5, 0, 20), dtype=np.int64)
    need = int(L.fs_eval_clients_ws_doubles(rows, N))
    assert need == ws_doubles(rows, N)
    ws = torch.zeros(need, dtype=torch.float64, device=dev)
    out = torch.full((2 * N,), CANARY, dtype=torch.float64, device=dev)
    p, h, hz = _ptr, h_n.ctypes.data, h_zero.ctypes.data

    def ce(phi_=phi, ld_=ld, off_=off, h_=h, y_=y, N_=N, W_=W, stride=0, C_=C, out_=out, ws_=ws, need_=need):
        return L.fs_eval_clients(p(phi_), ld_, p(off_), h_, p(y_), N_, p(W_), stride, C_, p(out_), p(ws_), need_, None)

    def mse(phi_=phi, ld_=ld, off_=off, h_=h, y_=yf, N_=N, W_=W, stride=0, out_=out, ws_=ws, need_=need):
        return L.fs_eval_clients_mse(p(phi_), ld_, p(off_), h_, p(y_), N_, p(W_), stride, p(out_), p(ws_), need_,
                                     None)

    bad = [
        (lambda: ce(C_=33), 'num_classes'), (lambda: ce(C_=0), 'num_classes'),
        (lambda: ce(ld_=96), 'ld'), (lambda: mse(ld_=96), 'ld'),
        (lambda: ce(N_=0), 'N'),
        (lambda: ce(phi_=None), 'null'), (lambda: ce(off_=None), 'null'), (lambda: ce(h_=None), 'null'),
        (lambda: ce(y_=None), 'null'), (lambda: ce(W_=None), 'null'), (lambda: ce(out_=None), 'null'),
        (lambda: ce(ws_=None), 'null'), (lambda: mse(y_=None), 'null'), (lambda: mse(ws_=None), 'null'),
        (lambda: ce(need_=need - 1), 'workspace'), (lambda: mse(need_=need - 1), 'workspace'),
        (lambda: ce(h_=hz), 'n_j'), (lambda: mse(h_=hz), 'n_j'),
        (lambda: ce(stride=-4), 'w_stride'), (lambda: ce(stride=C * ld + 2), 'w_stride'),
    ]
    for call, needle in bad:
        rc = call()
        assert rc < 0, needle
        assert needle in L.fs_last_error().decode(), (needle, L.fs_last_error())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all()
    assert L.fs_eval_clients_ws_doubles(0, 5) == 0 and L.fs_eval_clients_ws_doubles(5, 0) == 0
    assert ce() == 0 and mse() == 0                    # the same arguments, unbroken, are accepted
    torch.cuda.synchronize()

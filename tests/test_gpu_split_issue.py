"""The split form's in-backward row loads at G = 2 (csrc/local_train_split.hip, SP_BWD_FENCE).

The 16x16x4 early instance of config 2's shape (ld = 2048, G = 2, full slices) now ends every
backward iteration that issues next-step row loads with a scheduling fence, so the loads go out
where the source puts them and land in registers of their own (scripts/lt_issue_points.py shows
the compiled schedule; tests/test_split_schedule.py checks it).  Only the issue time and the
registers of a load move: weights and losses must be BITWISE those of the late-issue instance
(split_early = -1), and within the usual tolerance of the oracle.  Reference: train_loop,
/root/reference/functions/tools.py:177-215.
"""
import numpy as np
import pytest
import torch

from oracle import fedsim_oracle as O
from tests.test_gpu_parity import _rand_clients, _train_via_abi, amd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

G, D, E = 2, 2048, 2


def _kernel(amd):
    return amd.lib.LT_KERNELS[amd.lib.lib().fs_local_train_last_kernel()]


def _early_and_late(amd, Xs, ys, W0, args, seed):
    out = []
    for early in (0, -1):
        with amd.lib.tuning(split_early=early):
            out.append(_train_via_abi(amd, Xs, ys, W0, *args, seed=seed, split=G))
            assert _train_via_abi.last_G == G
            assert _kernel(amd) == 'split'
    return out


def _check_oracle(Xs, ys, W0, W, loss, lr, B, reg, lam, seed, chained=False, every=1):
    torch.manual_seed(seed)
    start = W0
    for j, (X, y) in enumerate(zip(Xs, ys)):
        if j % every == 0 or chained:
            Wr, lref = O.train_client(X, y, start, lr, E, B, False, 0.0, reg, lam)
            assert np.abs(W[j] - Wr).max() <= 2e-5 * max(1.0, np.abs(Wr).max()), j
            assert abs(loss[j] - lref) <= 2e-5 * max(1.0, abs(lref)), j
            if chained:
                start = Wr
        else:
            torch.empty(2 * E, dtype=torch.int64).random_()     # the oracle's draws for client j


@pytest.mark.parametrize('C', [10, 16])
@pytest.mark.parametrize('B', [32, 17])
@pytest.mark.parametrize('reg', [False, True])
def test_split_issue_bitwise(amd, C, B, reg):
    """Parallel clients of 17, 40 and 95 rows (one-step and two-step epochs, ragged last batches:
    the pre-forward's first and last step and the client switch), plain and with the ridge term
    (FedAMW's local training, the same instance)."""
    rs = np.random.RandomState(100 * C + B + reg)
    Xs, ys = _rand_clients(rs, [17, 40, 95], D, C)
    W0 = (rs.normal(size=(C, D)) * 0.1).astype(np.float32)
    lam = 0.002 if reg else 0.0
    args = (0.4, E, B, False, 0.0, reg, lam, False)
    (We, le), (Wl, ll) = _early_and_late(amd, Xs, ys, W0, args, 5)
    assert np.array_equal(We, Wl), np.abs(We - Wl).max()
    assert np.array_equal(le, ll)
    _check_oracle(Xs, ys, W0, We, le, 0.4, B, reg, lam, 5)


def test_split_issue_group_walks_clients(amd):
    """A group that walks several clients refills its row registers across the client boundary.
    The launch takes min(N, CUs / G) groups and no argument lowers that, so 5 clients on 2 groups
    cannot be asked for: instead (a) 5 chained clients -- ONE group walks all five, the same
    instance at this shape -- and (b) 2 * (CUs / G) + 5 small parallel clients, so every group
    walks two or three."""
    rs = np.random.RandomState(77)
    C, B = 10, 32
    W0 = (rs.normal(size=(C, D)) * 0.1).astype(np.float32)
    Xs, ys = _rand_clients(rs, [17, 40, 95, 33, 64], D, C)
    args = (0.4, E, B, False, 0.0, True, 0.002, True)
    (We, le), (Wl, ll) = _early_and_late(amd, Xs, ys, W0, args, 6)
    assert np.array_equal(We, Wl) and np.array_equal(le, ll)
    _check_oracle(Xs, ys, W0, We, le, 0.4, B, True, 0.002, 6, chained=True)

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 2 * (cus // G) + 5
    sizes = list(rs.randint(17, 41, size=N))
    Xs, ys = _rand_clients(rs, sizes, D, C)
    args = (0.3, E, B, False, 0.0, False, 0.0, False)
    (We, le), (Wl, ll) = _early_and_late(amd, Xs, ys, W0, args, 8)
    assert np.array_equal(We, Wl) and np.array_equal(le, ll)
    _check_oracle(Xs, ys, W0, We, le, 0.3, B, False, 0.0, 8, every=53)

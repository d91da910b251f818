"""The split form's trimmed hand-off chain (csrc/local_train_split.hip, round 12).

Between a step's forward and its backward the split kernel publishes its partial logits, polls its
partners', sums, and runs the softmax.  Round 12 took out of that chain what the result never
needed: the cross-entropy of epochs whose loss is discarded, two integer divisions per step (the
(epoch, batch) of a step is now carried as counters and reset at every client), the IEEE division
1 / batch rows, a second exchange slot no C <= 15 ever filled (C = 16 keeps it, on kernels of its
own) and the two norm granules under plain FedAvg.  No float operation that reaches W or the loss
moved, so the results must stay

  * within tests/fixtures.py's bounds of the oracle (O.train_client; reference: train_loop,
    /root/reference/functions/tools.py:177-215), and
  * BITWISE those of the pipe form (G | G_PIPE) and, at G = 4, of the pair form, neither of which
    this change touched.

ld = 2048 at G = 2 is the only width that reaches config 2's instance class (two 16-row tiles, full
16-tile slices, the early row issue).
"""
import numpy as np
import pytest
import torch

from oracle import fedsim_oracle as O
from tests.fixtures import LOSS_RTOL, W_RTOL
from tests.test_gpu_parity import _rand_clients, _train_via_abi, amd  # noqa: F401 (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("mb_off")]

LD, G2 = 2048, 2
SIZES = [1, 17, 32, 33, 64, 95]     # 33: a tail batch of one row at B = 32; 32: none
LR, MU, LAM = 0.3, 0.05, 0.002
TERMS = {'none': (False, False), 'ridge': (False, True), 'prox': (True, False), 'prox+ridge': (True, True)}
_DATA = {}


def _clients(C, n):
    """n clients of the SIZES cycle at width LD, made once per C and shared (never written to)"""
    key = (C, n)
    if key not in _DATA:
        rs = np.random.RandomState(100 * C + n)
        Xs, ys = _rand_clients(rs, [SIZES[j % len(SIZES)] for j in range(n)], LD, C)
        W0 = (rs.normal(size=(C, LD)) * 0.1).astype(np.float32)
        _DATA[key] = (Xs, ys, W0)
    return _DATA[key]


def _check_oracle(Xs, ys, W0, W, loss, E, B, prox, reg, chained, seed, sample):
    """clients in `sample` against the oracle under fixtures.py's bounds (the oracle draws every
    client's passes in order, so the others' draws are consumed)"""
    torch.manual_seed(seed)
    start, worst_w, worst_l = W0, 0.0, 0.0
    for j, (X, y) in enumerate(zip(Xs, ys)):
        if chained or j in sample:
            Wr, lref = O.train_client(X, y, start, LR, E, B, prox, MU, reg, LAM)
            dw = np.abs(W[j] - Wr).max() / np.abs(Wr).max()
            dl = abs(loss[j] - lref) / max(1.0, abs(lref))
            worst_w, worst_l = max(worst_w, dw), max(worst_l, dl)
            if chained:
                start = Wr
        else:
            torch.empty(2 * E, dtype=torch.int64).random_()     # the oracle's draws for client j
    print('max|W - W_ref| / max|W_ref| = %.3g (bound %g), loss %.3g (bound %g)' % (worst_w, W_RTOL, worst_l, LOSS_RTOL))
    assert worst_w <= W_RTOL, worst_w
    assert worst_l <= LOSS_RTOL, worst_l


def _run(amd, Xs, ys, W0, E, B, prox, reg, chained, seed, split):
    out = _train_via_abi(amd, Xs, ys, W0, LR, E, B, prox, MU, reg, LAM, chained, seed=seed, split=split)
    assert _train_via_abi.last_G == split
    return out


@pytest.mark.parametrize('mode', ['parallel', 'chain'])
@pytest.mark.parametrize('terms', list(TERMS))
@pytest.mark.parametrize('E', [1, 2, 3])
@pytest.mark.parametrize('B', [32, 17])
@pytest.mark.parametrize('C', [10, 15, 16])
def test_split_chain_sweep(amd, C, B, E, terms, mode):
    """ld = 2048, G = 2.  C = 15 is the last one-slot class count, 16 runs the two-slot kernels.
    parallel: 2 x groups + 5 clients, so some groups walk two or three clients and the (epoch, batch)
    counters reset mid-launch; chain: 5 clients, the weights carried in registers.  Bitwise the pipe
    form; the oracle on the first and last clients of the launch (every size, both tiers)."""
    prox, reg = TERMS[terms]
    chained = mode == 'chain'
    groups = torch.cuda.get_device_properties(0).multi_processor_count // G2
    n = 5 if chained else 2 * groups + 5
    Xs, ys, W0 = _clients(C, n)
    seed = 7
    Ws, ls = _run(amd, Xs, ys, W0, E, B, prox, reg, chained, seed, G2)
    Wp, lp = _run(amd, Xs, ys, W0, E, B, prox, reg, chained, seed, G2 | amd.lib.G_PIPE)
    assert np.array_equal(Ws, Wp), np.abs(Ws - Wp).max()
    assert np.array_equal(ls, lp), np.abs(ls - lp).max()
    sample = set(range(len(SIZES))) | set(range(n - len(SIZES), n))
    _check_oracle(Xs, ys, W0, Ws, ls, E, B, prox, reg, chained, seed, sample)


@pytest.mark.parametrize('terms', ['none', 'prox+ridge'])
@pytest.mark.parametrize('C', [10, 14])
def test_split_chain_pair_g4(amd, C, terms):
    """ld = 2048 at G = 4 (half slices: the late instances, one slot): bitwise the pair form, which
    covers C <= 14; the oracle on every client."""
    prox, reg = TERMS[terms]
    Xs, ys, W0 = _clients(C, 9)
    Ws, ls = _run(amd, Xs, ys, W0, 2, 32, prox, reg, False, 3, 4)
    Wp, lp = _run(amd, Xs, ys, W0, 2, 32, prox, reg, False, 3, 4 | amd.lib.G_PAIR)
    assert np.array_equal(Ws, Wp), np.abs(Ws - Wp).max()
    assert np.array_equal(ls, lp)
    _check_oracle(Xs, ys, W0, Ws, ls, 2, 32, prox, reg, False, 3, set(range(9)))


@pytest.mark.parametrize('G', [4, 8, 16])
def test_split_chain_wider_groups(amd, G):
    """One case at each wider group, at the smallest full-slice width (D = 1024 G - 24, the last
    tile ragged), plain FedAvg (no norm granules): bitwise the pipe form, every client against the
    oracle."""
    rs = np.random.RandomState(40 + G)
    D, C, E, B = 1024 * G - 24, 10, 2, 32
    Xs, ys = _rand_clients(rs, [65, 33, 0, 7, 96, 1, 40], D, C)
    W0 = (rs.normal(size=(C, D)) * 0.1).astype(np.float32)
    Ws, ls = _run(amd, Xs, ys, W0, E, B, False, False, False, 5, G)
    Wp, lp = _run(amd, Xs, ys, W0, E, B, False, False, False, 5, G | amd.lib.G_PIPE)
    assert np.array_equal(Ws, Wp), np.abs(Ws - Wp).max()
    assert np.array_equal(ls, lp)
    _check_oracle(Xs, ys, W0, Ws, ls, E, B, False, False, False, 5, set(range(len(Xs))))


@pytest.mark.parametrize('terms', ['none', 'ridge'])
def test_split_chain_timeout_raises(amd, terms):
    """The injected hand-off timeout (fs_tuning.inject_timeout, spin_limit = 0) still surfaces as
    FedsimError with the shrunken exchange (no norm granules, one slot)."""
    prox, reg = TERMS[terms]
    Xs, ys, W0 = _clients(10, 5)
    with amd.lib.tuning(inject_timeout=1):
        with pytest.raises(amd.lib.FedsimError, match='timed out'):
            _train_via_abi(amd, Xs, ys, W0, LR, 2, 32, prox, MU, reg, LAM, False, split=G2)

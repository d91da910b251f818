"""fs_eval and the fused evaluation blocks (csrc/eval_rows.h, the one body both run) against a
plain float64 reference (tests/eval_reference.py), at the edges of the kernel's structure.

On exact inputs (integers times a power of two: the logits carry no rounding in any summation
order) the accuracy is compared EXACTLY -- no one-sample slack, ties to the lowest class index --
and the loss within the bound of the softmax arithmetic alone (eval_reference.loss_bound, derived
there).  Every test prints its worst |loss - reference| as a fraction of its bound.
"""
import numpy as np
import pytest
import torch

from tests.eval_reference import (BIG_C, BIG_LD, BIG_N, SWEEP_TILES, case_seed, ce_acc_ref, dot_bound_rows,
                                  exact_problem, loss_bound, sweep_cases)
from tests.test_gpu_parity import amd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678


def _evaluate(amd, X, y, W, C, ld, runs=1):
    """fs_eval through engine.Evaluator with sentinels behind out[1] and behind the workspace's
    fs_eval_ws_doubles(n) doubles; returns the ``runs`` results [runs, 2] and checks the sentinels."""
    dev = torch.device('cuda')
    n, D = X.shape
    ev = amd.engine.Evaluator(torch.from_numpy(X), torch.from_numpy(y), D, C, dev, ld)
    assert ev.f.ld == ld and ev.n == n
    need = int(amd.lib.lib().fs_eval_ws_doubles(n))
    assert ev.ws.numel() == need
    ev.ws = torch.full((need + 8,), SENTINEL, dtype=torch.float64, device=dev)
    Wd = torch.zeros(C, ld, device=dev)
    Wd[:, :D] = torch.from_numpy(W)
    res = []
    for _ in range(runs):
        out = torch.full((6,), SENTINEL, dtype=torch.float64, device=dev)
        ev.run(Wd, out)
        o = out.cpu().numpy()
        assert (o[2:] == SENTINEL).all(), 'fs_eval wrote behind out[1]'
        res.append(o[:2])
    assert (ev.ws[need:].cpu().numpy() == SENTINEL).all(), 'fs_eval wrote behind its workspace'
    return np.array(res)


def _check_exact(amd, case, spread=20.0, runs=1):
    """One exact-input case: exact accuracy, loss within loss_bound; returns |dloss| / bound."""
    n, D, ld, C = case
    X, y, W, info = exact_problem(np.random.RandomState(case_seed(*case)), n, D, C, spread=spread)
    ce, loss, correct = ce_acc_ref(X, y, W)
    got = _evaluate(amd, X, y, W, C, ld, runs)
    acc = 100.0 * correct / n
    assert abs(got[0, 1] - acc) <= 1e-12 * acc, (case, got[0, 1], acc, info)
    bound = loss_bound(C, ce)
    frac = abs(got[0, 0] - loss) / bound
    assert np.isfinite(got[0, 0]) and frac <= 1.0, (case, got[0, 0], loss, bound)
    for r in got[1:]:
        assert np.array_equal(r, got[0]), 'fs_eval is not bitwise repeatable'
    return frac, info


@pytest.mark.parametrize('tiles', SWEEP_TILES)
def test_eval_structural_sweep(amd, tiles):
    """ld / 64 = ``tiles`` feature tiles (the boundaries of the 8-wave tile split: one tile, one
    per wave, wave 0's second tile, every second tile, a second trip of the loop) with every row
    count in {1, 15, 16, 17, 33} and every class count in {1, 2, 15, 16, 17, 31, 32} (both
    eval_kernel instances, the class clamp at 17 and 31, ragged and full row groups), D = ld and
    D = ld - 37.  Exact inputs: accuracy exact (the sweep's tied rows carry labels on the lower
    and on the higher tied class, test_eval_reference.py), loss within loss_bound."""
    worst, tied = 0.0, 0
    for case in sweep_cases(tiles):
        frac, info = _check_exact(amd, case)
        worst, tied = max(worst, frac), tied + info['tied']
    print('tiles %d: worst |loss - ref| / bound = %.3f over %d cases, %d tied rows'
          % (tiles, worst, len(sweep_cases(tiles)), tied))


@pytest.mark.parametrize('C', BIG_C)
def test_eval_finalizer_second_stride(amd, C):
    """4113 rows at ld = 64: 258 workgroups, so threads 0 and 1 of the finaliser each fold a
    second partial (i += 256) and the last row group holds one row."""
    assert (BIG_N + 15) // 16 == 258
    frac, info = _check_exact(amd, (BIG_N, BIG_LD, BIG_LD, C))
    print('n = %d, C = %d: |loss - ref| / bound = %.3f, %d tied rows' % (BIG_N, C, frac, info['tied']))


@pytest.mark.parametrize('lo,hi,C', [(3, 5, 8), (3, 5, 32), (3, 19, 20), (3, 19, 32)])
def test_eval_argmax_ties_go_to_the_lowest_class(amd, lo, hi, C):
    """Two classes with identical weight rows -- in one class tile (3, 5) and across the two
    tiles of eval_kernel<2> (3, 19) -- scaled by 4 so that the pair is the maximum of many rows;
    half the rows labelled ``lo`` (correct wherever the pair wins), half ``hi`` (never
    correct).  The expected correct count is the reference's np.argmax, exactly."""
    n, D = 64, 200
    rs = np.random.RandomState(100 * lo + hi + C)
    X, y, W, _ = exact_problem(rs, n, D, C)
    W[lo] *= 4.0                                   # (integers up to 12: still exact)
    W[hi] = W[lo]
    y[:] = np.where(np.arange(n) % 2 == 0, lo, hi)
    z = X.astype(np.float64) @ W.astype(np.float64).T
    wins = (z[:, lo] == z.max(axis=1)) & (np.argmax(z, axis=1) == lo)
    n_lo, n_hi = int((wins & (y == lo)).sum()), int((wins & (y == hi)).sum())
    assert n_lo >= 4 and n_hi >= 4                 # the rule decides rows of both kinds
    ce, loss, correct = ce_acc_ref(X, y, W)
    assert correct == n_lo                         # a last-maximum rule would give n_hi
    got = _evaluate(amd, X, y, W, C, 256)[0]
    assert got[1] == 100.0 * correct / n, (got[1] * n / 100.0, correct, n_hi)
    frac = abs(got[0] - loss) / loss_bound(C, ce)
    print('tie %d/%d of %d classes: %d rows to the lower, %d on the higher label; |loss - ref| / bound = %.3f'
          % (lo, hi, C, n_lo, n_hi, frac))
    assert frac <= 1.0


def test_eval_stability_at_large_logits(amd):
    """Logits past +-150 (exp(z) alone overflows fp32 above 88.7): the maximum is subtracted,
    so the exact-input assertions hold unchanged."""
    case = (33, 1000, 1024, 10)
    X, y, W, _ = exact_problem(np.random.RandomState(case_seed(*case)), *case[:2], case[3], spread=150.0)
    z = X @ W.T
    assert z.max() >= 150.0 and z.min() <= -150.0
    frac, _ = _check_exact(amd, case, spread=150.0)
    print('logits in [%.0f, %.0f]: |loss - ref| / bound = %.3f' % (z.min(), z.max(), frac))


def test_eval_bitwise_repeatable(amd):
    """Two runs of one case (33 tiles, 33 rows, 17 classes: every wave's partials, two class
    tiles, three workgroups) give bitwise equal out."""
    frac, _ = _check_exact(amd, (33, 2112 - 37, 2112, 17), runs=2)
    print('repeat: |loss - ref| / bound = %.3f' % frac)


@pytest.mark.parametrize('n,D,C,seed', [(70, 1000, 10, 0), (33, 2048, 26, 0)])
def test_eval_random_inputs(amd, n, D, C, seed):
    """cos(.) / sqrt(D) features and normal weights, where the fp32 logits do round: the loss
    within loss_bound plus the mean of dot_bound_rows (2 (D + 7) 2^-24 max_c sum_d |x_d w_cd|
    per row, the worst case of any summation order); the arg-max must match on every row whose
    top two float64 logits are further apart than that per-row figure (each of the two can move
    by half of it, so no closer pair can change order -- the tightest reading of "twice the
    bound"), and such rows are at most 2 % of the test set."""
    rs = np.random.RandomState(seed)
    X = (np.cos(rs.normal(size=(n, D))) / np.sqrt(D)).astype(np.float32)
    W = rs.normal(size=(C, D)).astype(np.float32)
    y = rs.randint(0, C, size=n).astype(np.int64)
    y[0], y[-1] = 0, C - 1
    ce, loss, _ = ce_acc_ref(X, y, W)
    z = X.astype(np.float64) @ W.astype(np.float64).T
    rows = dot_bound_rows(X, W)
    top = np.sort(z, axis=1)
    unsure = (top[:, -1] - top[:, -2]) < rows
    sure_correct = int(((np.argmax(z, axis=1) == y) & ~unsure).sum())
    got = _evaluate(amd, X, y, W, C, (D + 63) // 64 * 64)[0]
    bound = loss_bound(C, ce) + float(rows.mean())
    frac = abs(got[0] - loss) / bound
    correct = got[1] * n / 100.0
    print('random (%d, %d, %d): |loss - ref| / bound = %.2e, %d of %d rows excluded from the arg-max check'
          % (n, D, C, frac, int(unsure.sum()), n))
    assert unsure.sum() <= 0.02 * n
    assert frac <= 1.0, (got[0], loss, bound)
    assert abs(correct - round(correct)) <= 1e-9 and sure_correct <= round(correct) <= sure_correct + unsure.sum()


# ---------------------------------------------------------------------------------------------
# the fused evaluation, per training form

def _forms(amd):
    L = amd.lib
    off = dict(train_form=1, split_mb=-1, split_dbuf=-1, split_pipe=-1, split_teams=-1)
    return {
        # form: (fs_tuning, D = ld, trainer.G, FS_LT_*)
        'split': (off, 1024, 2, 2),
        'mb': (dict(off, split_mb=1), 1024, 2, 7),
        'dbuf': (dict(off, split_dbuf=1), 2048, 2, 3),
        'pair': (dict(off, train_form=2), 1024, 2 | L.G_PAIR, 4),
        'pipe': (dict(off, train_form=0, split_pipe=1), 2048, 2 | L.G_PIPE, 5),
        'teams': (dict(off, split_teams=1), 2048, 4 | L.G_TEAMS, 6),
    }


def _run_federation(amd, Xs, ys, Xt, yt, C, D, defer):
    """Two FedAvg rounds with parallel clients; (federation, W_rounds, eval history [2, 2] in
    float64, the FS_LT_* of each round's training launch)."""
    stats = {'trace': True}
    torch.manual_seed(11)
    fed = amd.tools.Federation('fedavg', Xs, ys, Xt, yt, None, 'classification', C, D, 0.5, 1, 32, False, 0.0,
                               False, 0.0, 2, 1e-3, 'parallel', stats=stats, verbose=False,
                               options={'defer_eval': defer})
    kernels = []
    for _ in range(2):
        fed.round()
        kernels.append(int(amd.lib.lib().fs_local_train_last_kernel()))
    fed.results()
    return fed, stats['W_rounds'], fed.eval_hist.cpu().numpy().copy(), kernels


@pytest.mark.parametrize('clients', ['ten', 'idle'])
@pytest.mark.parametrize('form', ['split', 'mb', 'dbuf', 'pair', 'pipe', 'teams'])
def test_fused_eval_per_training_form(amd, form, clients):
    """Every training form's launch carries the deferred evaluation in its own call site and LDS
    buffer: FedAvg, parallel clients, C = 10, B = 32, the form forced by fs_tuning at its
    narrowest width, an exact test set.  'ten': N = 10 (the aggregate's one-launch form with one
    sub-range carries the finaliser; one row group per evaluation block).  'idle': as many
    clients as leave 8 to 8 + width - 1 CUs idle and 16 (2 idle) + 5 test rows, so that every
    evaluation block walks two row groups and block 0 a third (eval_persistent's rg += E).

    Round 0's evaluation rides on round 1's training launch, round 1's runs as fs_eval.  Per
    round: the accuracy equals the float64 reference on that round's traced W exactly and the
    loss lies within loss_bound of it -- the bound of exact LOGITS, kept although a trained W
    is no power-of-two grid: with features of three significant bits the fp32 dot product's
    error stays a small part of it (the printed fraction) -- and the deferred run agrees with
    the run that evaluates every round in a launch of its own to 1e-12, on bitwise equal W."""
    tune, D, G, kernel = _forms(amd)[form]
    C = 10
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    width = G & (amd.lib.G_PAIR - 1)
    per = 2 if G & (amd.lib.G_PAIR | amd.lib.G_TEAMS) else 1
    if clients == 'ten':
        N, n_t = 10, 16 * 16 + 5
    else:
        N = (cus - 8) // width * per
        n_t = 16 * (2 * (cus - (cus - 8) // width * width)) + 5
    rs = np.random.RandomState(len(form) * 7 + N)
    sizes = rs.randint(8, 41, size=N)
    Xall = (np.cos(rs.normal(size=(int(sizes.sum()), D))) / np.sqrt(D)).astype(np.float32)
    yall = rs.randint(0, C, size=int(sizes.sum())).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    Xs = [torch.from_numpy(Xall[off[j]:off[j + 1]]) for j in range(N)]
    ys = [torch.from_numpy(yall[off[j]:off[j + 1]]) for j in range(N)]
    Xt, yt, _, info = exact_problem(rs, n_t, D, C)
    with amd.lib.tuning(**tune):
        args = (amd, Xs, ys, torch.from_numpy(Xt), torch.from_numpy(yt), C, D)
        ref, W0, ev0, k0 = _run_federation(*args, defer=False)
        fed, W1, ev1, k1 = _run_federation(*args, defer=True)
    tr = fed.trainer
    assert tr.G == G and ref.trainer.G == G and k0 == [kernel, kernel] and k1 == [kernel, kernel], (tr.G, k0, k1)
    idle = cus - tr.groups(cus) * tr.width
    E = fed.plan.eval_blocks()
    assert E == min(idle, (n_t + 15) // 16) and E > 0 and ref.plan.eval_blocks() == E
    if clients == 'idle':
        assert 4 <= idle <= 16 and E == idle and (n_t + 15) // 16 == 2 * E + 1
    assert np.array_equal(W0, W1)
    np.testing.assert_allclose(ev1, ev0, rtol=1e-12, atol=0)
    worst = 0.0
    for t in range(2):
        ce, loss, correct = ce_acc_ref(Xt, yt, W1[t])
        acc = 100.0 * correct / n_t
        bound = loss_bound(C, ce)
        for ev in (ev0, ev1):
            assert abs(ev[t, 1] - acc) <= 1e-12 * acc, (t, ev[t, 1], acc)
            frac = abs(ev[t, 0] - loss) / bound
            assert frac <= 1.0, (t, ev[t, 0], loss, bound)
            worst = max(worst, frac)
    print('%s, N = %d, %d idle CUs, %d evaluation blocks over %d rows: worst |loss - ref| / bound = %.3f'
          % (form, N, idle, E, n_t, worst))

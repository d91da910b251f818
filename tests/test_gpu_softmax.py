"""The softmax of every form of fs_local_train and every solver of fs_mix_solve at saturated and
offset logits (tests/softmax_reference.py; the inputs are proven on the CPU in
tests/test_softmax_reference.py).

Every other GPU test of these kernels draws logits below about 2 in magnitude, where a softmax
that subtracts no maximum, takes it over the wrong lanes, lets a padded class slot in as 0 or leaks
an invalid row of a short batch still gives near-right answers.  Here the rows of one batch sit at
offsets 0, +-64 and +-128 and

  'saturated'  every row is won by about 256: exp(z - m) is exactly 0 for every loser, the gradient
               is exactly +-1/b or 0 and the whole step is exact in fp32 in any summation order --
               the kernel's result is compared BITWISE with the float64 reference rounded to fp32
               (this rests on v_rcp_f32(1.0) == 1.0 in the fast e * rcp(sum e) forms);
  'mixed'      saturated rows (won by 120), rows whose logits all tie exactly and plain rows share
               ragged batches; compared with the float64 reference within the project's bounds
               (2e-5 for training, 1e-5 / 1e-4 for p and its momentum buffer), each case admitted
               only where the fp32 oracle itself stays within a quarter of the bound.

Each test asserts the form (fs_local_train_last_kernel) or solver (fs_mix_solve_last_mode) that
ran.  Reference: train_loop and the p-SGD, functions/tools.py:177-215, 441-453 of the reference.
"""
import numpy as np
import pytest
import torch

from tests import softmax_reference as R
from tests.test_gpu_parity import _record_margin, _train_via_abi, amd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32


def _train(amd, form, G, Xs, ys, W0, args, chained, seed=11):
    """One launch of the named form at width G; asserts that it is the form that ran."""
    L = amd.lib
    split = {'single': 1, 'split': G, 'mb': G, 'dbuf': G, 'pair': G | L.G_PAIR, 'pipe': G | L.G_PIPE,
             'teams': G | L.G_TEAMS}[form]
    tune = dict(split_mb=1 if form == 'mb' else -1, split_dbuf=1 if form == 'dbuf' else -1)
    with L.tuning(**tune):
        W, loss = _train_via_abi(amd, Xs, ys, W0, *args, chained, seed=seed, split=split)
        ran = L.LT_KERNELS[L.lib().fs_local_train_last_kernel()]
    assert ran == form and _train_via_abi.last_G == split, (ran, form, _train_via_abi.last_G)
    return W, loss


def _modes(form):
    return (False,) if form in R.PARALLEL_ONLY_FORMS else (False, True)


@pytest.mark.parametrize('case', R.SAT_TRAIN_CASES, ids=R.id_of)
def test_train_saturated_bitwise(amd, case):
    """E = 2, lr = 2^-6, no prox, no ridge, parallel and chained clients: W_out bitwise the float64
    reference rounded to fp32, the loss within 2e-5 max(1, |loss|); the 'all_won' client returns
    its start bitwise with loss 0.0 (chained: the next client starts from it); pair, pipe and dbuf
    bitwise the split form too.  A class count the split form has no instance for (more than 512
    exchanged values at G >= 8) must be refused by the planner, not run."""
    form, G, D, C, B = case
    Xs, ys, W0 = R.saturated_train_inputs(*case)
    args = (R.LR_SAT, 2, B, False, 0.0, False, 0.0)
    if form == 'split' and not R.split_fits(G, C, B):
        with pytest.raises(amd.lib.FedsimError, match='not available'):
            _train(amd, form, G, Xs, ys, W0, args, False)
        return
    for chained in _modes(form):
        W, loss = _train(amd, form, G, Xs, ys, W0, args, chained)
        torch.manual_seed(11)
        Wr, lr_, gap = R.train_chain_ref64(Xs, ys, W0, *args, chained)
        assert gap >= R.GAP_EXACT
        for j in range(len(Xs)):
            assert np.array_equal(W[j], Wr[j].astype(F32)), (chained, j, np.abs(W[j] - Wr[j]).max())
            assert abs(loss[j] - lr_[j]) <= R.TOL * max(1.0, abs(lr_[j])), (chained, j, loss[j], lr_[j])
        j = R.ALL_WON_CLIENT
        assert np.array_equal(W[j], W[j - 1] if chained else W0) and loss[j] == 0.0
        if C >= 2:
            assert not np.array_equal(W[j + 1], W[j] if chained else W0)        # ... and the next one moves
        if form in R.BITWISE_SPLIT_FORMS:
            Ws, ls = _train(amd, 'split', G, Xs, ys, W0, args, chained)
            assert np.array_equal(W, Ws) and np.array_equal(loss, ls), chained


@pytest.mark.parametrize('case', R.MIXED_TRAIN_CASES, ids=R.id_of)
def test_train_mixed_vs_float64(amd, case):
    """E = 2 on ragged clients (tail batches of 1, 7 and B - 3 rows) that mix saturated, tied and
    plain rows at five offsets; prox (mu = 0.03) and ridge (lam = 0.002) on in every other case:
    W within 2e-5 max(1, |W_ref|max) of the float64 reference, the loss within 2e-5 max(1, |loss|),
    everything finite; pair, pipe and dbuf bitwise the split form."""
    form, G, D, C, B = case
    Xs, ys, W0 = R.mixed_train_inputs(*case)
    on = R.mixed_terms(case)
    args = (R.mixed_train_lr(case), 2, B, on, R.MU, on, R.LAM)
    worst = 0.0
    for chained in _modes(form):
        W, loss = _train(amd, form, G, Xs, ys, W0, args, chained)
        assert np.isfinite(W).all() and np.isfinite(loss).all()
        torch.manual_seed(11)
        Wr, lr_, _ = R.train_chain_ref64(Xs, ys, W0, *args, chained)
        eW = [float(np.abs(W[j] - Wr[j]).max() / (R.TOL * max(1.0, np.abs(Wr[j]).max()))) for j in range(len(Xs))]
        el = [float(abs(loss[j] - lr_[j]) / (R.TOL * max(1.0, abs(lr_[j])))) for j in range(len(Xs))]
        print('%s %s: |W - ref| / bound %s, |loss - ref| / bound %s'
              % (R.id_of(case), 'chained' if chained else 'parallel', np.round(eW, 4), np.round(el, 4)))
        worst = max([worst] + eW + el)
        _record_margin('softmax-train-' + R.id_of(case), dict(chained=chained, W_over_bound=eW, loss_over_bound=el))
        assert max(eW) <= 1.0 and max(el) <= 1.0, (chained, eW, el)
        if form in R.BITWISE_SPLIT_FORMS:
            Ws, ls = _train(amd, 'split', G, Xs, ys, W0, args, chained)
            assert np.array_equal(W, Ws) and np.array_equal(loss, ls), chained


def _mixture(amd, Z, y, p0, Bv):
    """A fresh Mixture whose Z [nv][C][ldN] holds the given logits, padding client columns 0 (as
    fs_mix_z leaves them)."""
    N, C, nv = Z.shape
    dev = torch.device('cuda')
    mix = amd.engine.Mixture(torch.zeros(nv, 64), torch.from_numpy(y), 64, C, N, Bv, torch.from_numpy(p0), dev)
    mix.Z.zero_()
    mix.Z.view(nv, C, mix.ldN)[:, :, :N] = torch.from_numpy(np.ascontiguousarray(Z.transpose(2, 1, 0))).to(dev)
    return mix


@pytest.mark.parametrize('case', R.SAT_SOLVE_CASES, ids=R.id_of)
def test_solve_saturated_step_bitwise(amd, case):
    """One step (nv == Bv, one epoch, no momentum buffer yet, lr = 2^-10) on saturated validation
    logits written straight into Z: p and buf bitwise the float64 reference rounded to fp32."""
    solver, N, C, Bv, tune = case
    Z, y, p0 = R.saturated_solve_inputs(N, C, Bv)
    with amd.lib.tuning(mix_solver=solver, **tune):
        mix = _mixture(amd, Z, y, p0, Bv)
        torch.manual_seed(7)
        mix.solve(None, amd.rng.draw_pass_seeds(1), R.LR_P_SAT, z=False)
        torch.cuda.synchronize()
        mix.check_errors()
        assert amd.lib.SOLVER_NAMES[amd.lib.lib().fs_mix_solve_last_mode()] == solver
    torch.manual_seed(7)
    pr, br = R.solve_ref64(Z, y, p0, None, R.LR_P_SAT, 1, Bv)
    p, b = mix.p.cpu().numpy(), mix.buf.cpu().numpy()
    assert np.array_equal(b, br.astype(F32)), np.abs(b - br).max()
    assert np.array_equal(p, pr.astype(F32)), np.abs(p - pr).max()
    assert not np.array_equal(p, p0)


@pytest.mark.parametrize('case', R.MIXED_SOLVE_CASES, ids=R.id_of)
def test_solve_mixed_vs_float64(amd, case):
    """2 rounds of 2 epochs (the momentum buffer kept across the rounds) with a ragged last batch
    on validation rows that mix saturated, tied and plain logits at five offsets: p within 1e-5
    and buf within 1e-4 of the float64 reference, relative to its largest entry."""
    solver, N, C, nv, Bv, tune = case
    Z, y, p0, lr = R.mixed_solve_inputs(N, C, nv, Bv)
    pr, br = p0, None
    with amd.lib.tuning(mix_solver=solver, **tune):
        mix = _mixture(amd, Z, y, p0, Bv)
        for rnd in range(2):
            torch.manual_seed(70 + rnd)
            mix.solve(None, amd.rng.draw_pass_seeds(2), lr, z=False)
            torch.cuda.synchronize()
            mix.check_errors()
            assert amd.lib.SOLVER_NAMES[amd.lib.lib().fs_mix_solve_last_mode()] == solver
            torch.manual_seed(70 + rnd)
            pr, br = R.solve_ref64(Z, y, pr, br, lr, 2, Bv)
            p, b = mix.p.cpu().numpy(), mix.buf.cpu().numpy()
            assert np.isfinite(p).all() and np.isfinite(b).all()
            ep = float(np.abs(p - pr).max() / np.abs(pr).max())
            eb = float(np.abs(b - br).max() / np.abs(br).max())
            print('%s round %d: ep / bound %.4f, eb / bound %.4f' % (R.id_of(case), rnd, ep / R.P_TOL, eb / R.BUF_TOL))
            _record_margin('softmax-solve-' + R.id_of(case), dict(round=rnd, p_over_bound=ep / R.P_TOL,
                                                                   buf_over_bound=eb / R.BUF_TOL))
            assert ep <= R.P_TOL and eb <= R.BUF_TOL, (rnd, ep, eb)

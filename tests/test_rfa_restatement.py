"""tests/rfa_restatement.py on the CPU: what the RFA rule of include/fedsim.h guarantees (the geometric
median's breakdown bound from init='start', non-finite rows at weight 0, a non-rising objective, convergence
to a float64 Weiszfeld run), its edge cases, the drop-in's host checks, the driver's row, the header.  No GPU."""
import inspect
import os

import numpy as np
import pytest

from tests import rfa_restatement as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24


def _norm(v):
    return float(np.sqrt((np.asarray(v, F64) ** 2).sum()))


# ---- the rule ----

@pytest.mark.parametrize('attack', RR.ATTACKS)
@pytest.mark.parametrize('case', RR.ATTACK_CASES)
def test_breakdown_bound_from_start(case, attack):
    """||v_T - c|| <= (2 (1 - rho) / (1 - 2 rho)) max_good ||W_k - c||, c the good rows' mean, rho the corrupted
    share of alpha: the bound of the geometric median itself (Lopuhaa and Rousseeuw 1991; RFA's Lemma), held
    by the T-step iterate from x for T in {1, 3, 8}.  Non-finite rows end with b_k == 0 exactly."""
    M, L, bad = case
    W, x, alpha, ids = RR.attacked(M, L, bad, attack)
    good = np.setdiff1d(np.arange(M), ids)
    a64 = alpha.astype(F64)
    rho = a64[ids].sum() / a64.sum()
    assert rho <= 0.45
    c = W[good].astype(F64).mean(0)
    radius = max(_norm(W[k].astype(F64) - c) for k in good)
    bound = 2.0 * (1.0 - rho) / (1.0 - 2.0 * rho) * radius
    for T in (1, 3, 8):
        r = RR.chain(W, x, alpha, T=T, nu=1e-6, init='start')
        assert np.isfinite(r['out']).all()
        ratio = _norm(r['out'].astype(F64) - c) / bound
        print('M=%d len=%d bad=%d %s T=%d rho=%.3f ratio to the bound %.3f' % (M, L, bad, attack, T, rho, ratio))
        assert ratio <= 1.0
        if attack in ('nan', 'inf'):
            assert (r['b'][ids] == 0).all() and not np.isfinite(r['dist'][ids]).any()
            assert (r['b'][good] > 0).all() and np.isfinite(r['dist'][good]).all()
        assert abs(float(r['b'].astype(F64).sum()) - 1.0) <= M * EPS


@pytest.mark.parametrize('init', RR.INITS)
@pytest.mark.parametrize('attack', RR.ATTACKS)
@pytest.mark.parametrize('case', RR.ATTACK_CASES)
def test_objective_never_rises(case, attack, init):
    """A smoothed Weiszfeld step minimises a majoriser of g that touches it at v, so g(v') <= g(v) in exact
    arithmetic while the set of finite rows stays the same.  The slack for the arithmetic: g is A-Lipschitz in
    v (h is 1-Lipschitz), A = sum of the finite rows' alpha.  v' carries the rounding of the b_k to float (the
    fold moves by at most eps sum_k b_k ||W_k|| <= eps R) and its own rounding to float (eps ||v'|| <= eps R),
    R the largest norm of a finite row and eps = 2^-24; each of the two values of g compared carries the relative
    eps of the float difference in every d_k (the double sums add 2^-50 at most).  With a factor 2 on each:
        g(v') <= g(v) (1 + 4 eps) + 4 eps A R."""
    M, L, bad = case
    W, x, alpha, ids = RR.attacked(M, L, bad, attack)
    r = RR.chain(W, x, alpha, T=8, nu=1e-6, init=init)
    fin = np.isfinite(W).all(1)
    A = float(alpha[fin].astype(F64).sum())
    R = max(_norm(W[k]) for k in np.nonzero(fin)[0])
    obj = r['obj']
    first = 1 if init == 'mean' else 0          # (g(x) -> g(mean) is no Weiszfeld step)
    last = 8 + (1 if init == 'mean' else 0)
    assert np.isfinite(obj[:last + 1]).all() and np.isnan(obj[last + 1:]).all()
    for t in range(first, last):
        rise = obj[t + 1] - obj[t]
        assert rise <= 4 * EPS * obj[t] + 4 * EPS * A * R, (t, rise / obj[t])


@pytest.mark.parametrize('case', RR.ATTACK_CASES)
def test_converges_to_a_float64_weiszfeld_run(case):
    """No bad rows, T = 8 from x against a float64 Weiszfeld run r_0 = x, ..., r_300.  Two checks, both with
    tolerances taken from the reference run and the number format, none from the rule's own output:
      (a) against the reference's own 8th iterate: ||v_8 - r_8|| <= 4 eps ||r_8||.  Every fold rounds v to
          float, eps ||v|| in norm, which the contracting iteration carries on as a geometric series (factor 2),
          and as much again for the b_k and the distances' float differences.
      (b) against the run's end: ||v_8 - r_300|| <= (a)'s tolerance + ||r_8 - r_300|| + ||r_300 - r_299||, the
          reference's own distance from its 8th iterate to its last one and its last movement.
    Without the term ||r_8 - r_300|| no implementation can pass (b) at M = 5, len = 36: there the float64
    run itself is 1.3e-4 from its end after 8 iterations (8 steps contract by about 1 / M each, not to float
    precision), against 1.6e-6 for the last movement plus the float rounding.  At the other four shapes
    ||r_8 - r_300|| is below the float rounding and (b) holds without it."""
    M, L, _ = case
    W, x, alpha, _ = RR.attacked(M, L, 0, 'nan')
    r = RR.chain(W, x, alpha, T=8, nu=1e-6, init='start')
    its = RR.weiszfeld64(W, alpha, x, 300, 1e-6)
    v8 = r['out'].astype(F64)
    rnd = 4 * EPS * _norm(its[8])
    trunc, move = _norm(its[8] - its[300]), _norm(its[300] - its[299])
    print('M=%d len=%d: ||v_8 - r_8|| = %.3g (float rounding %.3g), ||v_8 - r_300|| = %.3g, ||r_8 - r_300|| = %.3g, '
          '||r_300 - r_299|| = %.3g' % (M, L, _norm(v8 - its[8]), rnd, _norm(v8 - its[300]), trunc, move))
    assert _norm(v8 - its[8]) <= rnd
    assert _norm(v8 - its[300]) <= rnd + trunc + move
    if M > 5:
        assert trunc <= rnd and _norm(v8 - its[300]) <= rnd + move


def test_edges():
    W, x, alpha = RR.inputs('normal', 9, 36)
    # T = 0
    r = RR.chain(W, x, alpha, T=0, init='start')
    assert r['out'].tobytes() == x.tobytes() and np.isfinite(r['obj'][0]) and np.isnan(r['obj'][1])
    assert (r['dist'] == np.sqrt(RR.d2_of(W, x))).all()
    m = RR.chain(W, x, alpha, T=0, init='mean')
    want = (alpha.astype(F64)[:, None] * W.astype(F64)).sum(0) / alpha.astype(F64).sum()
    assert np.abs(m['out'].astype(F64) - want).max() <= 4 * EPS * np.abs(want).max()
    assert np.isfinite(m['obj']).all() and (m['b'] == (alpha.astype(F64) / RR.sliced_sum(alpha.astype(F64), 256)).astype(F32)).all()
    # M = 1: the row itself from the first step on
    r = RR.chain(W[:1], x, alpha[:1], T=2)
    assert r['out'].tobytes() == W[0].tobytes() and r['b'].tolist() == [1.0] and r['dist'][0] == 0.0
    # every row NaN: x bit for bit, objective NaN, weights 0
    for init in RR.INITS:
        r = RR.chain(np.full_like(W, np.nan), x, alpha, T=3, init=init)
        assert r['out'].tobytes() == x.tobytes() and np.isnan(r['obj']).all() and (r['b'] == 0).all()
    # alpha with zeros: those rows weigh 0, the rest is the chain over the others up to the summation order
    a0 = alpha.copy()
    a0[[1, 4]] = 0
    r = RR.chain(W, x, a0, T=3)
    assert (r['b'][[1, 4]] == 0).all() and (np.delete(r['b'], [1, 4]) > 0).all()
    s = RR.chain(np.delete(W, [1, 4], 0), x, np.delete(a0, [1, 4]), T=3)
    assert np.abs(r['out'].astype(F64) - s['out']).max() <= 8 * EPS * np.abs(x).max()
    # nu above every distance: the weights reduce to alpha / sum(alpha)
    r = RR.chain(W, x, alpha, T=2, nu=1e6)
    assert (r['b'] == (alpha.astype(F64) / 1e6 / RR.sliced_sum(alpha.astype(F64) / 1e6, 256)).astype(F32)).all()
    assert np.abs(r['b'].astype(F64) - alpha.astype(F64) / alpha.astype(F64).sum()).max() <= 2 * EPS
    # all-equal rows: distance 0, the nu branch, g = nu / 2 * sum(alpha)
    We, xe, ae = RR.inputs('equal', 5, 36)
    r = RR.chain(We, xe, ae, T=2, nu=1e-3)
    assert r['out'].tobytes() == xe.tobytes() and (r['dist'] == 0).all()
    assert abs(r['obj'][2] - 0.5e-3 * ae.astype(F64).sum()) <= 1e-18


def test_mean_init_is_dragged_by_a_huge_finite_row():
    """Why 'start' is the default: a finite row of 1e30 pulls the weighted mean out, and a few steps do not
    bring the iterate back; from x the same rows stay inside the bound (test_breakdown_bound_from_start)."""
    W, x, alpha, ids = RR.attacked(12, 132, 2, 'huge')
    good = np.setdiff1d(np.arange(12), ids)
    c = W[good].astype(F64).mean(0)
    radius = max(_norm(W[k].astype(F64) - c) for k in good)
    r = RR.chain(W, x, alpha, T=8, init='mean')
    assert _norm(r['out'].astype(F64) - c) > 1e6 * radius


def test_widths_and_workspace():
    assert [RR.width(M) for M in (1, 1261, 1262, 2523, 2524, 5047)] == [32, 32, 16, 16, 8, 8]
    assert RR.stripes(5, 36) == 2 and RR.stripes(1262, 36) == 3 and RR.stripes(5047, 36) == 5
    for L in (4, 36, 20480):
        prev = 0
        for M in (1, 2, 1261, 1262, 2523, 2524, 5047):
            assert RR.ws_bytes(M, L) >= prev
            prev = RR.ws_bytes(M, L)


def test_orders_by_hand():
    # the tree: ((p0 + p1) + (p2 + p3)); a slice sum is sequential
    big = 2.0 ** 53
    assert RR.tree(np.array([big, 1.0, 1.0, -big])) == 1.0            # (big + 1 = big) + (1 - big): not the
    assert RR.sliced_sum(np.array([big, 1.0, 1.0, -big]), 2) == 1.0   # sequential sum, which gives 0
    assert RR.sliced_sum(np.array([1.0, big, 1.0, -big]), 2) == 2.0   # (1 + 1) + (big - big)
    assert RR.sliced_sum(np.array([big, 1.0, 1.0, -big]), 1) == 0.0   # one slice is sequential
    # a row with b == 0 is never multiplied
    W = np.array([[1.0, 2.0, 3.0, 4.0], [np.nan, np.inf, -np.inf, 1.0]], F32)
    assert RR.fold(W, np.array([1.0, 0.0], F32)).tolist() == [1.0, 2.0, 3.0, 4.0]
    # a ragged last stripe takes its own columns only
    W, x, _ = RR.inputs('normal', 3, 36)
    p = RR.partials(W, x)
    e = (W - x[None, :]).astype(F32).astype(F64) ** 2
    assert p.shape == (2, 3) and np.allclose(p[1], e[:, 32:].sum(1), rtol=1e-15) and np.allclose(p[0], e[:, :32].sum(1), rtol=1e-15)


# ---- the drop-in's host side ----

@pytest.fixture(scope='module')
def tools():
    import fedamw_amd  # noqa: F401
    from fedamw_amd.functions import tools
    return tools


def test_signature(tools):
    fa = list(inspect.signature(tools.FedAvg).parameters.values())
    pos = [p.name for p in fa if p.kind == p.POSITIONAL_OR_KEYWORD]
    ps = list(inspect.signature(tools.FedRFA).parameters.values())
    assert [p.name for p in ps if p.kind == p.POSITIONAL_OR_KEYWORD] == pos
    kw = {p.name: p.default for p in ps if p.kind == p.KEYWORD_ONLY}
    assert kw == dict(iters=3, nu=1e-6, init='start', weighting='size', byzantine=None, stats=None, verbose=True,
                      options=None, participation=None, sample_seed=0)


def test_argument_checks(tools):
    X = [np.zeros((4, 3), F32)] * 7
    y = [np.zeros(4, np.int64)] * 7
    a = (X, y, X[0], y[0], 'classification', 2, 8, 0.1, 1, 2, False, 0.0, False, 0.0, 1)
    for it in (-1, 33, 1.5, '3', None, True):
        with pytest.raises(ValueError, match='iters must be'):
            tools.FedRFA(*a, iters=it)
    for nu in (0, 0.0, -1e-6, float('inf'), float('nan'), '1e-6', None, True):
        with pytest.raises(ValueError, match='nu must be'):
            tools.FedRFA(*a, nu=nu)
    for init in ('median', 0, None):
        with pytest.raises(ValueError, match='init must be'):
            tools.FedRFA(*a, init=init)
    for w in ('none', None, 1):
        with pytest.raises(ValueError, match='weighting must be'):
            tools.FedRFA(*a, weighting=w)
    for bz in (dict(ids=[0], fraction=0.1), dict(), dict(ids=[7]), dict(ids=[0], attack='zero')):
        with pytest.raises(ValueError, match='byzantine'):
            tools.FedRFA(*a, byzantine=bz)
    with pytest.raises(ValueError, match='above'):
        tools._check_rfa_rounds([12, RR.MAX_M + 1], RR.MAX_M)
    with pytest.raises(ValueError, match='no client'):
        tools._check_rfa_rounds([12, 0], RR.MAX_M)
    tools._check_rfa_rounds([1, 12, RR.MAX_M], RR.MAX_M)
    with pytest.raises(ValueError, match='parallel'):
        tools._check_rfa(3, 1e-6, 'start', 'size', 'sequential')
    assert tools.RFA_MAX_ITERS == RR.MAX_ITERS and tuple(tools.RFA_INITS) == RR.INITS


def test_driver_row_order():
    from fedamw_amd import experiment as E
    assert E.EXTRA_RFA == ['FedRFA'] and E.EXTRA_KRUM == ['Krum', 'MultiKrum']
    src = inspect.getsource(E)
    assert src.index('EXTRA_KRUM = ') < src.index('EXTRA_RFA = ')
    assert 'known = NAMES + EXTRA + EXTRA_FAIR + EXTRA_ROBUST + EXTRA_KRUM + EXTRA_RFA' in src
    run = inspect.getsource(E.run)
    assert run.index('for name in EXTRA_KRUM:') < run.index('for name in EXTRA_RFA:')
    with pytest.raises(ValueError, match='unknown algorithm'):
        E.run(algos=('Bulyan',))
    ap = inspect.getsource(E.main)
    for flag in ('--rfa-iters', '--rfa-nu', '--rfa-init', '--rfa-weighting', '--byzantine-fraction',
                 '--byzantine-attack', '--byzantine-scale'):
        assert flag in ap
    d = inspect.signature(E.run).parameters
    assert (d['rfa_iters'].default, d['rfa_nu'].default, d['rfa_init'].default, d['rfa_weighting'].default) == \
        (3, 1e-6, 'start', 'size')


def test_header_and_exports():
    from fedamw_amd import _lib
    h = open(os.path.join(ROOT, 'include', 'fedsim.h')).read()
    for sym in ('fs_aggregate_rfa', 'fs_aggregate_rfa_max_m', 'fs_rfa_step', 'fs_rfa_weights', 'fs_rfa_width',
                'fs_plan_set_rfa'):
        assert sym in _lib.EXPORTS and ('int %s(' % sym) in h
    assert 'fs_aggregate_rfa_ws_bytes' in _lib.EXPORTS and 'int64_t fs_aggregate_rfa_ws_bytes(' in h
    assert '#define FS_RFA_INIT_START 0' in h and '#define FS_RFA_INIT_MEAN 1' in h and '#define FS_RFA_MAX_ITERS 32' in h
    assert _lib.ABI_VERSION == 23 and '#define FS_ABI_VERSION 23' in h and 'aggregate_rfa' in _lib.KERNEL_SOURCES
    L = _lib.lib()
    assert L.fs_aggregate_rfa_max_m() == RR.MAX_M >= 5047 and RR.MAX_M >= L.fs_aggregate_robust_max_m()
    # the widths and the workspace size are host arithmetic
    for M in (1, 2, 64, 1250, RR.MAX_M32, RR.MAX_M32 + 1, RR.MAX_M16, RR.MAX_M16 + 1, RR.MAX_M):
        assert L.fs_rfa_width(M) == RR.width(M)
        for ln in (4, 36, 132, 20480, 163840):
            assert L.fs_aggregate_rfa_ws_bytes(M, ln) == RR.ws_bytes(M, ln)
    assert L.fs_rfa_width(0) == 0 and L.fs_rfa_width(RR.MAX_M + 1) == 0
    assert L.fs_aggregate_rfa_ws_bytes(RR.MAX_M + 1, 36) == 0
    # the error returns need no device: nothing is launched
    big = 1 << 40
    nan, inf = float('nan'), float('inf')

    def call(M=5, ln=4, st=4, T=3, nu=1e-6, init=0, ws=big, W=1, x=1, al=1, out=1, dist=1, b=1, obj=1, wsp=1):
        return L.fs_aggregate_rfa(W, st, None, M, ln, x, al, T, nu, init, out, dist, b, obj, wsp, ws, None)

    for kw in (dict(M=0), dict(M=-1), dict(M=RR.MAX_M + 1), dict(T=-1), dict(T=33), dict(nu=0.0), dict(nu=-1.0),
               dict(nu=nan), dict(nu=inf), dict(init=2), dict(init=-1), dict(ln=6, st=8), dict(st=6), dict(ln=8),
               dict(ln=0, st=0), dict(ws=16), dict(ws=RR.ws_bytes(5, 4) - 1), dict(W=None), dict(x=None),
               dict(al=None), dict(out=None), dict(dist=None), dict(b=None), dict(obj=None), dict(wsp=None)):
        assert call(**kw) == -1, kw
        assert b'rfa' in L.fs_last_error()
    assert L.fs_rfa_step(1, 4, None, 0, 4, 1, None, None, 1, 1, None) == -1
    assert L.fs_rfa_step(1, 4, None, RR.MAX_M + 1, 4, 1, None, None, 1, 1, None) == -1
    assert L.fs_rfa_step(1, 4, None, 5, 6, 1, None, None, 1, 1, None) == -1
    assert L.fs_rfa_step(1, 4, None, 5, 4, None, None, None, 1, 1, None) == -1
    assert L.fs_rfa_step(1, 4, None, 5, 4, 1, 1, None, 1, 1, None) == -1           # b without a flag
    assert L.fs_rfa_weights(None, 5, 4, 1, 0.0, 0, 1, 1, 1, 1, 1, None) == -1
    assert L.fs_rfa_weights(None, 0, 4, 1, 1e-6, 0, 1, 1, 1, 1, 1, None) == -1
    assert L.fs_rfa_weights(None, 5, 4, 1, 1e-6, 2, 1, 1, 1, 1, 1, None) == -1
    assert L.fs_rfa_weights(None, 5, 4, None, 1e-6, 0, 1, 1, 1, 1, 1, None) == -1
    assert L.fs_plan_set_rfa(None, 1, 3, 1e-6, 0, 0, 1, 1, 1, 1, big) == -1
    assert L.fs_plan_set_rfa(None, 0, 0, 0.0, 0, 0, None, None, None, None, 0) == -1

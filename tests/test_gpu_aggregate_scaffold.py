"""fs_aggregate_scaffold at kernel level, on the shape set of test_gpu_aggregate_nova.py: W_g bitwise
fs_aggregate_nova's mode 2 in every regime, c bitwise the numpy left fold in the left-fold regime
and inside the summation bound everywhere, the identity r = 0 / cs = 1, in-place operation and
argument validation.

Shapes: M in {1, 2, 15, 16, 48, 513} x len in {4, 192, 1028} (513 at len <= 192 only), chunks in
{0, 1} and 3 at M = 20; rows 0..M-1 and a strictly ascending subset of a 2M-row buffer whose other
rows hold NaN."""
import numpy as np
import pytest
import torch

from tests import scaffold_restatement as SR
from tests.test_gpu_aggregate_nova import SHAPES, U, case, left_fold_regime
from tests.test_gpu_aggregate_nova import run as run_nova

pytestmark = pytest.mark.gpu

CS = 0.6180339


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


def coef(cs):
    """r_k = p_k / (K_k lr) at the scale the drop-in produces (no powers of two), and the start c."""
    rs = np.random.RandomState(31 * cs['M'] + cs['L'])
    r = (cs['q'].astype(np.float64) / rs.uniform(0.3, 7.0, size=cs['M'])).astype(np.float32)
    c0 = rs.normal(size=cs['L']).astype(np.float32)
    return r, c0


def run(amd, cs, chunks, r, c0, cs_=CS, q=None, x=None):
    """One call on fresh copies -> (W_g, c) as numpy."""
    dev = amd.dev
    t = lambda a: None if a is None else torch.tensor(a, device=dev)   # noqa: E731
    agg = amd.engine.Aggregator(cs['M'], 1, cs['L'], dev, chunks=chunks)
    Wg, c = t(cs['base'] if x is None else x), t(c0)
    agg.run_scaffold(t(cs['W']), t(cs['q'] if q is None else q), t(r), cs_, Wg, c, sel=t(cs['sel']))
    return Wg.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_model_fold_is_mode_2_and_variate_fold_is_bounded(amd, M, L, chunks):
    """W_g bitwise run_nova(mode 2, base = W_g) in every regime (same q, chunks; the Aggregator's
    workspace holds more partials than any shape here asks for, so half of it clamps nothing), and
    per element |c - ref64| <= (M + 3) 2^-24 (|cs c| + sum_k |term_k|): the bound of the nova test --
    (M - 1) u of the sum in any order, a difference and a product inside a term, fl(cs c) and the
    final sum.  Nothing fitted."""
    for gathered in (False, True):
        cs = case(M, L, gathered)
        r, c0 = coef(cs)
        Wg, c = run(amd, cs, chunks, r, c0)
        ref = run_nova(amd, cs, chunks, 2)
        assert np.isfinite(Wg).all() and Wg.tobytes() == ref.tobytes(), (gathered, np.abs(Wg - ref).max())
        R = np.stack(cs['rows']).astype(np.float64)
        x = cs['base'].astype(np.float64)
        terms = r.astype(np.float64)[:, None] * (x - R)
        base = float(np.float32(CS)) * c0.astype(np.float64)
        err = np.abs(c.astype(np.float64) - (base + terms.sum(0)))
        bound = (M + 3) * U * (np.abs(base) + np.abs(terms).sum(0))
        print('M %d len %d chunks %d gathered %d: c max err/bound %.3f' % (M, L, chunks, gathered, (err / bound).max()))
        assert np.isfinite(c).all() and (err <= bound).all()


@pytest.mark.parametrize('M,L,chunks', [s for s in SHAPES if left_fold_regime(s[0], s[2])])
def test_left_fold_regime_is_bitwise_numpy(amd, M, L, chunks):
    for gathered in (False, True):
        cs = case(M, L, gathered)
        r, c0 = coef(cs)
        Wg, c = run(amd, cs, chunks, r, c0)
        xr, cr = SR.server(cs['base'], c0, cs['rows'], cs['q'], r, np.float32(CS), np.float32)
        assert Wg.tobytes() == xr.tobytes(), (gathered, np.abs(Wg - xr).max())
        bad = np.flatnonzero(c != cr)
        assert c.tobytes() == cr.tobytes(), (gathered, len(bad), c[bad[:4]], cr[bad[:4]])


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_zero_r_and_unit_cs_return_c(amd, M, L, chunks):
    for gathered in (False, True):
        cs = case(M, L, gathered)
        _, c0 = coef(cs)
        Wg, c = run(amd, cs, chunks, np.zeros(M, np.float32), c0, cs_=1.0)
        assert np.array_equal(c, c0)
        assert Wg.tobytes() == run_nova(amd, cs, chunks, 2).tobytes()


@pytest.mark.parametrize('M', [15, 48, 513])
@pytest.mark.parametrize('chunks', [0, 1])
def test_in_place(amd, M, chunks):
    """Both outputs are updated in place: the result equals the out-of-place evaluation (mode 2 into a
    fresh buffer for W_g; for c the same call on a second copy), bitwise, and a second call on the
    updated pair is again its own out-of-place evaluation -- x and c are read before they are written."""
    for L in (4, 192):
        for gathered in (False, True):
            cs = case(M, L, gathered)
            r, c0 = coef(cs)
            W1, c1 = run(amd, cs, chunks, r, c0)
            assert W1.tobytes() == run_nova(amd, cs, chunks, 2).tobytes()
            assert not np.array_equal(W1, cs['base']) and not np.array_equal(c1, c0)
            W2, c2 = run(amd, cs, chunks, r, c1, x=W1)
            assert W2.tobytes() == run_nova(amd, cs, chunks, 2, base=W1).tobytes()
            if left_fold_regime(M, chunks):
                assert c2.tobytes() == SR.server(W1, c1, cs['rows'], cs['q'], r, np.float32(CS), np.float32)[1].tobytes()


def test_bad_arguments_leave_both_outputs_untouched(amd):
    dev, L = amd.dev, amd.lib.lib()
    M, n = 4, 64
    W = torch.randn(M, n, device=dev)
    q = torch.full((M,), 0.25, device=dev)
    r = torch.full((M,), 0.5, device=dev)
    Wg = torch.full((n,), 7.0, device=dev)
    c = torch.full((n,), 5.0, device=dev)
    ws = torch.empty(8 * n, device=dev)
    P = amd.lib.ptr

    def call(W_=W, stride=n, q_=q, r_=r, M_=M, len_=n, Wg_=Wg, c_=c):
        p = lambda x: None if x is None else P(x)   # noqa: E731
        return L.fs_aggregate_scaffold(p(W_), stride, None, p(q_), p(r_), 0.5, M_, len_, p(Wg_), p(c_), P(ws),
                                       ws.numel(), 0, amd.lib.stream_ptr())

    for kw in (dict(M_=0), dict(len_=62), dict(stride=66), dict(W_=None), dict(q_=None), dict(r_=None), dict(Wg_=None),
               dict(c_=None), dict(c_=Wg)):
        assert call(**kw) == -1, kw
        assert 'aggregate_scaffold' in L.fs_last_error().decode()
    torch.cuda.synchronize()
    assert bool((Wg == 7.0).all()) and bool((c == 5.0).all())
    assert call() == 0                                           # (and the good call writes both)
    torch.cuda.synchronize()
    assert bool((Wg != 7.0).all()) and bool((c != 5.0).all())

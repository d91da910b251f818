"""fs_aggregate_opt at kernel level: its reduction to fs_aggregate_nova's mode 2, the exact left fold
and finish against tests/fedopt_restatement.py, the finish on the GPU's own delta in every regime,
in-place chaining, a zero update, and argument validation.

Shapes, rows and weights are tests/test_gpu_aggregate_nova.py's (M in {1, 2, 15, 16, 48, 513} x len in
{4, 192, 1028}, both ``chunks`` settings, contiguous and gathered rows with NaN in the rows outside
the sample): the smallest that reach every regime, a short last group and a partial last workgroup.

The fold's reordering and the finish are checked apart.  delta_gpu comes from an AVGM probe with
beta1 = 0 (m' = delta bitwise, whatever the regime); it is held to mode 2's summation bound
(M + 3) 2^-24 sum_k |term_k| against the float64 sum and, in the left-fold regime, to the numpy
float32 fold bitwise.  The finish applied in numpy float32 to delta_gpu must then be the kernel's
W_g, m and v bit for bit -- correctly rounded products, sums, quotient and square root, so no
tolerance.  v is drawn on both sides of delta_gpu^2 with every fifth element equal to it, so YOGI's
three signs occur in every case; all inputs stay in the normal float range."""
import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO
from tests.test_gpu_aggregate_nova import SHAPES, case, left_fold_regime
from tests.test_gpu_aggregate_nova import run as run_nova

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32 = np.float32
SC = FO.scalars(0.37, 0.9, 0.99, 1e-3)          # eta, beta1, omb1, beta2, omb2, tau
PROBE = FO.scalars(1.0, 0.0, 0.0, 1.0)


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


def run_opt(amd, cs, chunks, rule, sc, x, m, v):
    """One fs_aggregate_opt call on copies of (x, m, v); returns the three buffers after it."""
    dev = amd.dev
    t = lambda a: None if a is None else torch.tensor(a, device=dev)   # noqa: E731
    agg = amd.engine.Aggregator(cs['M'], 1, cs['L'], dev, chunks=chunks)
    xd, md, vd = t(x), t(m), t(v)
    eta, b1, o1, b2, o2, tau = (float(a) for a in sc)
    agg.run_opt(t(cs['W']), t(cs['q']), rule, xd, md, vd, eta, b1, o1, b2, o2, tau, sel=t(cs['sel']))
    return xd.cpu().numpy(), md.cpu().numpy(), None if vd is None else vd.cpu().numpy()


def delta_gpu(amd, cs, chunks, x):
    """The kernel's own fold at x: AVGM with beta1 = 0 leaves it in m (and x + delta in x)."""
    x2, d, _ = run_opt(amd, cs, chunks, 'avgm', PROBE, x, np.full_like(x, 3.0), None)
    return x2, d


def check_delta(cs, chunks, x, d):
    """delta_gpu against the float64 sum (mode 2's bound without the base term) and, in the left-fold
    regime, the numpy float32 fold bitwise."""
    M = cs['M']
    terms = cs['q'].astype(np.float64)[:, None] * (np.stack(cs['rows']).astype(np.float64) - x.astype(np.float64))
    err, bound = np.abs(d.astype(np.float64) - terms.sum(0)), (M + 3) * U * np.abs(terms).sum(0)
    assert np.isfinite(d).all() and (err <= bound).all(), (err / bound).max()
    if left_fold_regime(M, chunks):
        ref = FO.delta(cs['rows'], cs['q'], x)
        assert d.tobytes() == ref.tobytes(), np.abs(d - ref).max()


def moments(cs, d, seed):
    """m, and v on both sides of d^2 (four times it at even positions, a quarter of it at odd ones)
    with every fifth element equal to it, so that len = 4 has all three; all in the normal range."""
    rs = np.random.RandomState(seed)
    d2 = (d * d).astype(F32)
    m = (0.1 * rs.normal(size=d.shape)).astype(F32)
    v = (d2 * np.where(np.arange(d.size) % 2 == 0, F32(4.0), F32(0.25))).astype(F32)
    v[::5] = d2[::5]
    assert (np.abs(d) > 1e-15).all() and (v > 1e-30).all()
    return m, v


def same(got, ref, what):
    bad = np.flatnonzero(got != ref)
    assert got.tobytes() == ref.tobytes(), (what, len(bad), got[bad[:4]], ref[bad[:4]])


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_avgm_probe_is_mode_2(amd, M, L, chunks):
    """AVGM with beta1 = 0, eta = 1: W_g is bitwise fs_aggregate_nova mode 2 in place, in every regime."""
    for gathered in (False, True):
        cs = case(M, L, gathered)
        ref = run_nova(amd, cs, chunks, 2, in_place=True)
        x2, d = delta_gpu(amd, cs, chunks, cs['base'])
        assert np.isfinite(ref).all() and not np.array_equal(ref, cs['base'])
        same(x2, ref, gathered)
        same(x2, (cs['base'] + d).astype(F32), 'x + delta')


@pytest.mark.parametrize('rule', FO.RULES)
@pytest.mark.parametrize('M,L,chunks', [s for s in SHAPES if left_fold_regime(s[0], s[2])])
def test_left_fold_regime_is_bitwise_the_restatement(amd, M, L, chunks, rule):
    """M < 16 or chunks = 1: W_g, m and v are bitwise the numpy float32 restatement, two calls chained
    in place."""
    for gathered in (False, True):
        cs = case(M, L, gathered)
        x = cs['base']
        m, v = moments(cs, FO.delta(cs['rows'], cs['q'], x), 11)
        for call in range(2):
            ref = FO.server(rule, x, m, v, cs['rows'], cs['q'], SC)
            got = run_opt(amd, cs, chunks, rule, SC, x, m, None if rule == 'avgm' else v)
            same(got[0], ref[0], (gathered, call, 'x'))
            same(got[1], ref[1], (gathered, call, 'm'))
            if rule != 'avgm':
                same(got[2], ref[2], (gathered, call, 'v'))
                assert np.isfinite(got[2]).all() and (got[2] > 0).all()
                v = got[2]
            assert not np.array_equal(got[0], x)
            x, m = got[0], got[1]


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_finish_is_exact_on_the_gpus_delta_in_every_regime(amd, M, L, chunks):
    """Every regime, all four rules, two calls chained in place: delta_gpu within the summation bound,
    and the numpy finish on delta_gpu bitwise the kernel's three outputs."""
    for gathered in (False, True):
        cs = case(M, L, gathered)
        _, d0 = delta_gpu(amd, cs, chunks, cs['base'])
        m0, v0 = moments(cs, d0, 13)
        d2 = (d0 * d0).astype(F32)
        assert (v0 > d2).any() and (v0 < d2).any() and (v0 == d2).any()
        for rule in FO.RULES:
            x, m, v = cs['base'], m0, v0
            for call in range(2):
                _, d = delta_gpu(amd, cs, chunks, x)
                check_delta(cs, chunks, x, d)
                ref = FO.finish(rule, d, x, m, v, SC)
                got = run_opt(amd, cs, chunks, rule, SC, x, m, None if rule == 'avgm' else v)
                same(got[0], ref[0], (gathered, rule, call, 'x'))
                same(got[1], ref[1], (gathered, rule, call, 'm'))
                if rule != 'avgm':
                    same(got[2], ref[2], (gathered, rule, call, 'v'))
                    v = got[2]
                x, m = got[0], got[1]
            if rule == 'yogi':        # the three signs moved v as they should in the first call
                _, _, v1 = FO.finish(rule, d0, cs['base'], m0, v0, SC)
                assert (v1[v0 > d2] < v0[v0 > d2]).all() and (v1[v0 < d2] > v0[v0 < d2]).all()
                assert (v1[v0 == d2] == v0[v0 == d2]).all()


@pytest.mark.parametrize('M,chunks', [(2, 0), (48, 0), (48, 1), (513, 0)])
def test_zero_update(amd, M, chunks):
    """All rows equal x, so delta = 0: m' = fl(beta1*m), ADAM's v' = fl(beta2*v) and the other rules keep
    v, x moves by the old momentum alone (the numpy finish of a zero delta) and with m = 0 is
    unchanged; nothing is NaN at v = 0."""
    L = 192
    rs = np.random.RandomState(M)
    x = rs.normal(size=L).astype(F32)
    cs = dict(M=M, L=L, W=np.tile(x, (M, 1)), sel=None, q=case(M, L, False)['q'])
    m = (0.1 * rs.normal(size=L)).astype(F32)
    v = rs.uniform(0.5, 2.0, size=L).astype(F32)
    zero = np.zeros(L, F32)
    for rule in FO.RULES:
        for mm, vv in ((m, v), (m, zero), (zero, v), (zero, zero)):
            got = run_opt(amd, cs, chunks, rule, SC, x, mm, None if rule == 'avgm' else vv)
            assert np.isfinite(got[0]).all()
            same(got[0], FO.finish(rule, zero, x, mm, vv, SC)[0], (rule, 'x'))
            if not mm.any():
                same(got[0], x, (rule, 'x unchanged'))
            same(got[1], (SC[1] * mm).astype(F32), (rule, 'm'))
            if rule != 'avgm':
                assert np.isfinite(got[2]).all()
                want = (SC[3] * vv).astype(F32) if rule == 'adam' else vv
                same(got[2], want, (rule, 'v'))


def test_bad_arguments_leave_the_buffers_untouched(amd):
    """Every bad argument returns FS_EINVAL with a message; none of the three buffers (7, 8, 9) is
    written."""
    dev, L = amd.dev, amd.lib.lib()
    M, n = 4, 64
    W = torch.randn(M, n, device=dev)
    q = torch.full((M,), 0.25, device=dev)
    x = torch.full((n,), 7.0, device=dev)
    m = torch.full((n,), 8.0, device=dev)
    v = torch.full((n,), 9.0, device=dev)
    ws = torch.empty(4 * n, device=dev)
    P = amd.lib.ptr

    def call(W_=W, stride=n, q_=q, rule=3, tau=1e-3, M_=M, len_=n, x_=x, m_=m, v_=v):
        p = lambda a: None if a is None else P(a)   # noqa: E731
        return L.fs_aggregate_opt(p(W_), stride, None, p(q_), rule, 0.1, 0.9, 0.1, 0.99, 0.01, tau, M_, len_, p(x_),
                                  p(m_), p(v_), P(ws), ws.numel(), 0, amd.lib.stream_ptr())

    bad = [dict(M_=0), dict(len_=62), dict(stride=66), dict(stride=60, len_=64), dict(rule=0), dict(rule=5),
           dict(W_=None), dict(q_=None), dict(x_=None), dict(m_=None), dict(v_=None), dict(rule=2, v_=None),
           dict(rule=4, v_=None), dict(tau=0.0), dict(tau=-1.0), dict(rule=2, tau=0.0), dict(rule=4, tau=0.0),
           dict(m_=x), dict(v_=x), dict(v_=m), dict(rule=1, m_=x), dict(rule=1, v_=m)]
    for kw in bad:
        assert call(**kw) == -1, kw
        msg = L.fs_last_error().decode()
        assert 'fs_aggregate_opt' in msg or 'aggregate_opt_launch' in msg
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((m == 8.0).all()) and bool((v == 9.0).all())
    assert call(rule=1, v_=None, tau=0.0) == 0                    # AVGM needs neither d_v nor tau
    torch.cuda.synchronize()
    assert bool((x != 7.0).all()) and bool((m != 8.0).all()) and bool((v == 9.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((v != 9.0).all()) and bool(torch.isfinite(x).all())

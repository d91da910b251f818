"""fs_aggregate_qffl and fs_qffl_coef at kernel level.

Shapes, rows and weights are tests/test_gpu_aggregate_nova.py's (M in {1, 2, 15, 16, 48, 513} x len in
{4, 192, 1028}, both ``chunks`` settings, contiguous and gathered rows with NaN in the rows outside
the sample), plus len = 2308: 577 float4 positions, three 256-position blocks whose last holds one
full wave and one lane (and 73 8-position blocks whose last holds one lane).

The three outputs are checked apart.  d_S must be bitwise the d_m an AVGM probe of fs_aggregate_opt
(beta1 = 0) leaves with q = u, in every regime.  d_n is held to 16 * 2^-24 relative of the float64 sum
of the squares of the float32 differences -- the kernel's 10 float roundings per wave share with a
margin; everything above a wave is double -- and must be the same bits on a second call and with
the same rows gathered from a larger buffer.  The finish in numpy (tests/qffl_restatement.finish:
float64 sums with k ascending, IEEE + * /) on the GPU's own d_n and d_S must then be d_hc and d_W_g
bit for bit, for two calls chained in place."""
import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO
from tests import qffl_restatement as QR
from tests.test_gpu_aggregate_nova import SHAPES as NOVA_SHAPES
from tests.test_gpu_aggregate_nova import case, left_fold_regime
from tests.test_gpu_aggregate_opt import delta_gpu

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32 = np.float32
SHAPES = NOVA_SHAPES + [(M, 2308, c) for M in (1, 2, 15, 16, 48) for c in (0, 1)] + [(513, 2308, 0), (20, 2308, 3)]
LC = 2.0


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


def coefs(M, seed=5):
    """u and g of M clients: the nova case's weights times a loss power, g of the size q u / F L^2."""
    rs = np.random.RandomState(seed + M)
    n = rs.randint(1, 200, size=M)
    F = rs.uniform(0.3, 2.5, size=M)
    u = (n / n.sum() * F ** 2).astype(F32)
    g = (n / n.sum() * 2 * F * LC * LC).astype(F32)
    return u, g


def gather(cs, seed=9):
    """The same rows in the same order, scattered over a buffer of twice as many rows, NaN elsewhere."""
    M, L = cs['M'], cs['L']
    rs = np.random.RandomState(seed + M)
    sel = np.sort(rs.permutation(2 * M)[:M]).astype(np.int32)
    W = np.full((2 * M, L), np.nan, F32)
    W[sel] = np.stack(cs['rows'])
    return dict(cs, W=W, sel=sel)


def run_qffl(amd, cs, chunks, u, g, Lc, x, calls=1):
    """``calls`` fs_aggregate_qffl calls chained in place on a copy of x; per call (x', S, n, hc)."""
    dev = amd.dev
    t = lambda a: None if a is None else torch.tensor(a, device=dev)   # noqa: E731
    M, L = cs['M'], cs['L']
    agg = amd.engine.Aggregator(M, 1, L, dev, chunks=chunks)
    W, sel, ud, gd, xd = t(cs['W']), t(cs['sel']), t(u), t(g), t(x)
    nws = agg.qffl_ws(M)
    out = []
    for _ in range(calls):
        S = torch.full((L,), np.nan, device=dev)
        n = torch.full((M,), np.nan, dtype=torch.float64, device=dev)
        hc = torch.full((2,), np.nan, dtype=torch.float64, device=dev)
        nws.fill_(float('nan'))
        agg.run_qffl(W, ud, gd, Lc, xd, S, n, hc, nws, sel=sel)
        out.append(tuple(a.cpu().numpy().copy() for a in (xd, S, n, hc)))
    return out


def same(got, ref, what):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    bad = np.flatnonzero(got != ref)
    assert got.tobytes() == ref.tobytes(), (what, len(bad), got[bad[:4]], ref[bad[:4]])


def check_norms(cs, x, n, what):
    d = (np.stack(cs['rows']) - x).astype(F32).astype(np.float64)
    ref = (d * d).sum(1)
    err = np.abs(n - ref)
    print(what, 'norm rel err max %.3g of %.3g' % ((err / ref).max(), 16 * U))
    assert np.isfinite(n).all() and (err <= 16 * U * ref).all(), (what, (err / ref).max())


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_fold_norms_and_finish_in_every_regime(amd, M, L, chunks):
    u, g = coefs(M)
    for gathered in (False, True):
        cs = case(M, L, gathered)
        x = cs['base']
        outs = run_qffl(amd, cs, chunks, u, g, LC, x, calls=2)
        for call, (x2, S, n, hc) in enumerate(outs):
            what = (gathered, call)
            # S: the AVGM probe's d_m with q = u, bitwise; the numpy left fold where the regime is one
            _, d = delta_gpu(amd, dict(cs, q=u), chunks, x)
            same(S, d, what + ('S',))
            if left_fold_regime(M, chunks):
                same(S, FO.delta(cs['rows'], u, x), what + ('S numpy',))
            check_norms(cs, x, n, what)
            # the finish on the GPU's own n and S
            ref, H, coef = QR.finish(S, n, u, g, LC, x)
            assert H > 0 and coef > 0
            assert hc[0] == H and hc[1] == float(coef), (what, hc, H, coef)
            same(x2, ref, what + ('x',))
            assert np.isfinite(x2).all() and not np.array_equal(x2, x)
            x = x2


@pytest.mark.parametrize('M,L,chunks', [s for s in SHAPES if s[1] in (192, 2308)])
def test_norms_repeat_and_do_not_depend_on_the_gather(amd, M, L, chunks):
    """The same bits from a second call on the same inputs, and from the same rows gathered out of
    a buffer twice as large (S and x' too)."""
    u, g = coefs(M)
    cs = case(M, L, False)
    a = run_qffl(amd, cs, chunks, u, g, LC, cs['base'])[0]
    b = run_qffl(amd, cs, chunks, u, g, LC, cs['base'])[0]
    c = run_qffl(amd, gather(cs), chunks, u, g, LC, cs['base'])[0]
    for k, name in enumerate(('x', 'S', 'n', 'hc')):
        same(a[k], b[k], ('repeat', name))
        same(a[k], c[k], ('gathered', name))


@pytest.mark.parametrize('M,chunks', [(2, 0), (48, 0), (48, 1), (513, 0)])
def test_zero_update_and_zero_weights(amd, M, chunks):
    """All rows equal x: n = 0, S = 0, H = L U, x unchanged.  u = 0 and g = 0: H = 0, coef = 0 and x is
    left as it is; so is it when H is negative."""
    L = 192
    rs = np.random.RandomState(M)
    x = rs.normal(size=L).astype(F32)
    u, g = coefs(M)
    cs = dict(M=M, L=L, W=np.tile(x, (M, 1)), sel=None)
    x2, S, n, hc = run_qffl(amd, cs, chunks, u, g, LC, x)[0]
    assert not n.any() and not S.any()
    same(x2, x, 'zero update')
    assert hc[0] == QR.finish(S, n, u, g, LC, x)[1] and hc[1] > 0
    cs = case(M, L, False)
    zero = np.zeros(M, F32)
    x2, S, n, hc = run_qffl(amd, cs, chunks, zero, zero, LC, cs['base'])[0]
    assert hc[0] == 0.0 and hc[1] == 0.0 and not S.any() and (n > 0).all()
    same(x2, cs['base'], 'u = 0')
    x2, S, n, hc = run_qffl(amd, cs, chunks, u, (-1e6 * np.ones(M)).astype(F32), LC, cs['base'])[0]
    assert hc[0] < 0.0 and hc[1] == 0.0 and S.any()
    same(x2, cs['base'], 'H < 0')


def test_bad_arguments_leave_the_buffers_untouched(amd):
    """Every bad argument returns FS_EINVAL with a message; no output buffer is written."""
    dev, L = amd.dev, amd.lib.lib()
    M, n = 4, 64
    W = torch.randn(M, n, device=dev)
    u = torch.full((M,), 0.25, device=dev)
    g = torch.full((M,), 0.5, device=dev)
    x = torch.full((n,), 7.0, device=dev)
    S = torch.full((n,), 8.0, device=dev)
    nn = torch.full((M,), 9.0, dtype=torch.float64, device=dev)
    hc = torch.full((2,), 10.0, dtype=torch.float64, device=dev)
    ws = torch.empty(4 * n, device=dev)
    need = int(L.fs_aggregate_qffl_ws_doubles(M, n))
    assert need >= 1 and L.fs_aggregate_qffl_ws_doubles(0, n) == 0
    nws = torch.full((need,), 11.0, dtype=torch.float64, device=dev)
    P = amd.lib.ptr

    def call(W_=W, stride=n, u_=u, g_=g, Lc=2.0, M_=M, len_=n, x_=x, S_=S, n_=nn, hc_=hc, nws_=nws, nwsd=need):
        p = lambda a: None if a is None else P(a)   # noqa: E731
        return L.fs_aggregate_qffl(p(W_), stride, None, p(u_), p(g_), Lc, M_, len_, p(x_), p(S_), p(n_), p(hc_),
                                   P(ws), ws.numel(), 0, p(nws_), nwsd, amd.lib.stream_ptr())

    bad = [dict(M_=0), dict(len_=62), dict(stride=66), dict(stride=60, len_=64), dict(W_=None), dict(u_=None),
           dict(g_=None), dict(x_=None), dict(S_=None), dict(n_=None), dict(hc_=None), dict(nws_=None), dict(Lc=0.0),
           dict(Lc=-1.0), dict(Lc=float('inf')), dict(Lc=float('nan')), dict(nwsd=need - 1), dict(S_=x)]
    for kw in bad:
        assert call(**kw) == -1, kw
        msg = L.fs_last_error().decode()
        assert 'fs_aggregate_qffl' in msg or 'aggregate_qffl_launch' in msg
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((S == 8.0).all()) and bool((nn == 9.0).all())
    assert bool((hc == 10.0).all()) and bool((nws == 11.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((x != 7.0).all()) and bool((S != 8.0).all()) and bool((nn != 9.0).all()) and bool((hc != 10.0).all())
    assert bool(torch.isfinite(x).all())


@pytest.mark.parametrize('q', [0.0, 0.5, 1.0, 2.0, 5.0])
def test_qffl_coef(amd, q):
    """q = 0: u = p and g = 0 exactly.  Else against numpy float64 ``np.power``, 2^-22 relative on the
    float outputs: a few double ulps of pow can move the float rounding by at most one ulp.  A
    gathered and a NULL d_sel."""
    dev = amd.dev
    N, Lc = 37, 2.5
    rs = np.random.RandomState(int(10 * q) + 1)
    F = np.stack([rs.uniform(0.05, 3.0, size=N), rs.uniform(0, 100, size=N)], 1)
    F[3, 0] = 1e-3                                    # a client the model fits well
    Fd = torch.tensor(F, device=dev)
    for sel in (None, np.unique(np.append(rs.permutation(N)[:10], 3)).astype(np.int32)):
        rows = np.arange(N) if sel is None else sel
        p = rs.uniform(0.01, 0.2, size=len(rows)).astype(F32)
        u = torch.full((len(rows),), np.nan, device=dev)
        g = torch.full((len(rows),), np.nan, device=dev)
        amd.engine.qffl_coef(Fd, torch.tensor(p, device=dev), q, Lc, u, g,
                             None if sel is None else torch.tensor(sel, device=dev))
        u, g = u.cpu().numpy(), g.cpu().numpy()
        ru, rg = QR.coefficients(F[rows, 0], p, q, Lc, np.float64)
        if q == 0.0:
            same(u, p, 'u = p')
            assert not g.any()
            continue
        assert np.isfinite(u).all() and np.isfinite(g).all() and (u > 0).all() and (g > 0).all()
        for got, ref, name in ((u, ru, 'u'), (g, rg, 'g')):
            err = np.abs(got.astype(np.float64) - ref)
            print('q = %g %s: max rel err %.3g of %.3g' % (q, name, (err / ref).max(), 2.0 ** -22))
            assert (err <= 2.0 ** -22 * ref).all(), (q, name)
    L = amd.lib.lib()
    P = amd.lib.ptr
    pd, ud, gd = torch.ones(4, device=dev), torch.full((4,), 5.0, device=dev), torch.full((4,), 6.0, device=dev)
    for kw in (dict(q=-0.5), dict(L=0.0), dict(L=-1.0), dict(F=None), dict(p=None), dict(u=None), dict(g=None),
               dict(M=0)):
        a = dict(F=Fd, p=pd, u=ud, g=gd, q=1.0, L=2.0, M=4)
        a.update(kw)
        pp = lambda t: None if t is None else P(t)   # noqa: E731
        assert L.fs_qffl_coef(pp(a['F']), None, pp(a['p']), a['q'], a['L'], a['M'], pp(a['u']), pp(a['g']),
                              amd.lib.stream_ptr()) == -1, kw
        assert 'fs_qffl_coef' in L.fs_last_error().decode()
    torch.cuda.synchronize()
    assert bool((ud == 5.0).all()) and bool((gd == 6.0).all())

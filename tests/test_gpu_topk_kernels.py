"""fs_topk_threshold and fs_aggregate_topk at kernel level: bitwise tests/topk_restatement.py (NaN as NaN).

M in {1, 2, 3, 15, 16, 17, 65, 513, 1250}: both sides of the exact-fold bound (16) and of AG_ONE_MAX_N (512).
len in {4, 36, 132, 1028}, and -- the select has one path, whose only boundary is a row of exactly one
float4 per thread of its 1024-thread workgroup -- 4092, 4096 and 4100 at M in {1, 3, 17}, and 40964 (above the
40,960 floats of a CU's LDS) at M = 3.  kcount in {1, 2, len // 2, len - 1, len}.  Contiguous rows, and the
same rows gathered from a buffer of twice as many with NaN elsewhere and a sentinel in the other residuals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import topk_restatement as TK

pytestmark = pytest.mark.gpu

F32 = np.float32
MS = (1, 2, 3, 15, 16, 17, 65, 513, 1250)
LENS = (4, 36, 132, 1028)
SHAPES = [(M, L) for M in MS for L in LENS] + [(M, L) for M in (1, 3, 17) for L in (4092, 4096, 4100)] \
    + [(3, TK.LDS_FLOATS + 4)]
SENTINEL = F32(7.5)


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


def kcounts(L):
    return sorted({1, 2, max(1, L // 2), L - 1, L})


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(got, ref, what):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    ok = bits(got) == bits(ref)
    if got.dtype.kind == 'f':
        ok |= np.isnan(got) & np.isnan(ref)
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, (what, len(bad), got[bad[:4]], ref[bad[:4]], bad[:4])


def dv(amd, a):
    return None if a is None else torch.from_numpy(np.array(a, order='C')).to(amd.dev)      # (a copy: the inputs are read-only)


@functools.lru_cache(maxsize=None)
def inputs(M, L, values='normal'):
    """(W [M, L], x [L], e [M, L], q [M]); read-only, shared by the tests."""
    rs = np.random.RandomState(1000 * M + L)
    x = rs.standard_normal(L).astype(F32)
    q = rs.dirichlet(np.full(M, 2.0)).astype(F32)
    e = (rs.standard_normal((M, L)) * 0.25).astype(F32)
    if values == 'normal':
        W = rs.standard_normal((M, L)).astype(F32)
    elif values == 'ties':
        # five magnitudes, mixed signs, as exact differences: ties everywhere, also at the threshold, the
        # magnitudes spread over all four radix digits (exponent, and mantissa bits 22..15, 14..7, 6..0)
        mags = np.array([0.5, 0.5 + 2.0 ** -9, 0.5 + 2.0 ** -17, 0.5 + 2.0 ** -24, 192.0], F32)
        a = (mags[rs.randint(0, 5, (M, L))] * rs.choice([-1.0, 1.0], (M, L))).astype(F32)
        x = np.zeros(L, F32)
        e = np.zeros((M, L), F32)
        W = a
    elif values == 'zeros':
        W = np.broadcast_to(x, (M, L)).copy()
        e = np.zeros((M, L), F32)
    elif values == 'denormal':
        x = np.zeros(L, F32)
        W = (rs.randint(1, 1 << 22, (M, L)).astype(np.uint32)
             | (rs.randint(0, 2, (M, L)).astype(np.uint32) << 31)).view(F32)
        e = (rs.randint(0, 1 << 20, (M, L)).astype(np.uint32)).view(F32)
        q = np.full(M, F32(1.0), F32) if M == 1 else q
    elif values == 'nonfinite':
        W = rs.standard_normal((M, L)).astype(F32)
        for k in range(M):
            p = rs.permutation(L)
            W[k, p[0]] = np.inf
            if L > 4:
                W[k, p[1]], W[k, p[2]] = -np.inf, np.nan
            if L > 36 and k % 2:
                W[k, p[3:3 + L // 8]] = np.nan
    else:
        raise KeyError(values)
    for a in (W, x, e, q):
        a.setflags(write=False)
    return W, x, e, q


def gather(W, e, seed=9):
    """The same rows in the same order scattered over a buffer of twice as many rows: NaN in the other rows
    of W, a sentinel in the other rows of e."""
    M, L = W.shape
    sel = np.sort(np.random.RandomState(seed + M).permutation(2 * M)[:M]).astype(np.int32)
    big = np.full((2 * M, L), np.nan, F32)
    big[sel] = W
    ebig = None
    if e is not None:
        ebig = np.full((2 * M, L), SENTINEL, F32)
        ebig[sel] = e
    return big, ebig, sel


def run(amd, W, x, e, q, kcount, sel=None, chunks=0, calls=1, M=None):
    """``calls`` consecutive fs_aggregate_topk calls on the same device buffers (W_g and e carried);
    [dict(out, e, tau, kept)] as numpy after each."""
    M = (W.shape[0] if sel is None else len(sel)) if M is None else M
    L = W.shape[1]
    agg = amd.engine.Aggregator(M, 1, L, amd.dev, chunks=chunks)
    Wd, xd, ed, qd, sd = dv(amd, W), dv(amd, x), dv(amd, e), dv(amd, q), dv(amd, sel)
    res = []
    for _ in range(calls):
        tau = torch.full((M,), -1.0, device=amd.dev)
        kept = torch.full((M,), -1, dtype=torch.int32, device=amd.dev)
        agg.ws.fill_(float('nan'))
        agg.run_topk(Wd, qd, int(kcount), xd, ed, tau, kept, sel=sd, ws=agg.topk_ws())
        res.append(dict(out=xd.cpu().numpy().copy(), e=None if ed is None else ed.cpu().numpy().copy(),
                        tau=tau.cpu().numpy(), kept=kept.cpu().numpy()))
    assert torch.equal(Wd.cpu().isnan(), torch.from_numpy(np.isnan(W)))
    return res, agg.ws.numel() // L


def check(got, ref, what, rows=None, e_all=None):
    same(got['out'], ref['out'], (what, 'out'))
    same(got['tau'], ref['tau'], (what, 'tau'))
    same(got['kept'], ref['kept'], (what, 'kept'))
    if ref['e'] is not None:
        ge = got['e'] if rows is None else got['e'][rows]
        same(ge, ref['e'], (what, 'e'))
        if rows is not None:
            others = np.setdiff1d(np.arange(got['e'].shape[0]), rows)
            assert (got['e'][others] == SENTINEL).all(), (what, 'residual rows outside the sample were written')


@pytest.mark.parametrize('M,L', SHAPES)
def test_bitwise_contiguous_and_gathered(amd, M, L):
    W, x, e, q = inputs(M, L)
    big, ebig, sel = gather(W, e)
    for kc in kcounts(L):
        got, wsp = run(amd, W, x, e, q, kc)
        ref = TK.aggregate(W, x, e, q, kc, 0, wsp)
        assert (ref['kept'] >= kc).all()
        check(got[0], ref, (M, L, kc, 'contiguous'))
        got, _ = run(amd, big, x, ebig, q, kc, sel=sel)
        check(got[0], ref, (M, L, kc, 'gathered'), rows=sel)


@pytest.mark.parametrize('values', ['ties', 'zeros', 'denormal', 'nonfinite'])
@pytest.mark.parametrize('M,L', [(1, 4), (3, 132), (17, 1028), (65, 36), (3, 4100)])
def test_value_sets(amd, M, L, values):
    W, x, e, q = inputs(M, L, values)
    big, ebig, sel = gather(W, e)
    for kc in kcounts(L):
        ref = TK.aggregate(W, x, e, q, kc, 0, min(64, M))
        got, _ = run(amd, W, x, e, q, kc)
        check(got[0], ref, (values, M, L, kc))
        got, _ = run(amd, big, x, ebig, q, kc, sel=sel)
        check(got[0], ref, (values, M, L, kc, 'gathered'), rows=sel)
        if values == 'zeros':
            assert (ref['kept'] == L).all() and (ref['tau'].view(np.uint32) == 0).all()
        if values == 'ties' and L >= 36:
            assert (ref['kept'] > kc).any() or kc == L
        nomem = TK.aggregate(W, x, None, q, kc, 0, min(64, M))
        got, _ = run(amd, W, x, None, q, kc)
        check(got[0], nomem, (values, M, L, kc, 'no memory'))


@pytest.mark.parametrize('M,L', [(2, 36), (17, 132), (65, 1028), (513, 36), (3, 4096)])
def test_null_memory_equals_zero_memory(amd, M, L):
    W, x, _, q = inputs(M, L)
    for kc in (1, L // 2, L):
        a, _ = run(amd, W, x, None, q, kc)
        b, _ = run(amd, W, x, np.zeros((M, L), F32), q, kc)
        same(a[0]['out'], b[0]['out'], (M, L, kc, 'out'))
        same(a[0]['tau'], b[0]['tau'], (M, L, kc, 'tau'))
        same(a[0]['kept'], b[0]['kept'], (M, L, kc, 'kept'))


@pytest.mark.parametrize('M,L', [(3, 36), (17, 132), (65, 1028), (1250, 132)])
def test_two_calls_carry_the_residual(amd, M, L):
    W, x, e, q = inputs(M, L)
    kc = max(1, L // 8)
    big, ebig, sel = gather(W, e)
    for rows, args in ((None, (W, x, e, q, kc)), (sel, (big, x, ebig, q, kc))):
        got, wsp = run(amd, *args, sel=rows, calls=2)
        r1 = TK.aggregate(W, x, e, q, kc, 0, wsp)
        r2 = TK.aggregate(W, r1['out'], r1['e'], q, kc, 0, wsp)
        check(got[0], r1, (M, L, 'first'), rows=rows)
        check(got[1], r2, (M, L, 'second'), rows=rows)
        assert not np.array_equal(r1['out'], r2['out'])


@pytest.mark.parametrize('M,L', [(3, 132), (65, 1028), (513, 36), (3, TK.LDS_FLOATS + 4)])
def test_same_bits_from_the_same_inputs(amd, M, L):
    """d_W_g is updated in place; two runs from the same inputs leave the same bits everywhere."""
    W, x, e, q = inputs(M, L)
    kc = max(1, L // 16)
    a, _ = run(amd, W, x, e, q, kc)
    b, _ = run(amd, W, x, e, q, kc)
    for key in ('out', 'e', 'tau', 'kept'):
        same(a[0][key], b[0][key], (M, L, key))


@pytest.mark.parametrize('chunks', [1, 3, 8])
@pytest.mark.parametrize('M', [2, 17, 65, 513, 1250])
def test_forced_chunks(amd, M, chunks):
    L = 132
    W, x, e, q = inputs(M, L)
    big, ebig, sel = gather(W, e)
    kc = 13
    got, wsp = run(amd, W, x, e, q, kc, chunks=chunks)
    ref = TK.aggregate(W, x, e, q, kc, chunks, wsp)
    check(got[0], ref, (M, chunks))
    got, _ = run(amd, big, x, ebig, q, kc, sel=sel, chunks=chunks)
    check(got[0], ref, (M, chunks, 'gathered'), rows=sel)
    nomem, _ = run(amd, W, x, None, q, kc, chunks=chunks)
    check(nomem[0], TK.aggregate(W, x, None, q, kc, chunks, wsp), (M, chunks, 'no memory'))


@pytest.mark.parametrize('chunks', [0, 1, 4])
@pytest.mark.parametrize('M', [1, 3, 15, 16, 17, 65, 513, 1250])
def test_dense_identity_against_fs_aggregate_opt(amd, M, chunks):
    """kcount = len -- and a smaller kcount that still keeps every nonzero -- with e = 0 is fs_aggregate_opt's
    AVGM step at beta1 = 0, eta = 1 bit for bit, and e stays +0."""
    L = 132
    W, x, _, q = inputs(M, L)
    Wz = W.copy()
    Wz[:, ::3] = x[::3]                      # exact zeros in every update: kcount = the nonzeros suffices
    nz = int((Wz[0] != x).sum())
    assert ((Wz != x).sum(axis=1) == nz).all()
    agg = amd.engine.Aggregator(M, 1, L, amd.dev, chunks=chunks)
    for rows, kc in ((W, L), (Wz, nz)):
        xd, md = dv(amd, x), torch.zeros(L, device=amd.dev)
        agg.run_opt(dv(amd, rows), dv(amd, q), 'avgm', xd, md, None, eta=1.0, beta1=0.0)
        opt = xd.cpu().numpy()
        got, wsp = run(amd, rows, x, np.zeros((M, L), F32), q, kc, chunks=chunks)
        same(got[0]['out'], opt, (M, chunks, kc, 'opt'))
        same(got[0]['out'], TK.dense(rows, x, q, chunks, wsp), (M, chunks, kc, 'restatement'))
        assert not got[0]['e'].any() and not np.signbit(got[0]['e']).any()
        nomem, _ = run(amd, rows, x, None, q, kc, chunks=chunks)
        same(nomem[0]['out'], opt, (M, chunks, kc, 'no memory'))


@pytest.mark.parametrize('M,L', [(1, 4), (3, 132), (17, 4096), (65, 1028), (3, TK.LDS_FLOATS + 4)])
def test_threshold_alone_leaves_the_corrected_update_in_the_residual(amd, M, L):
    W, x, e, q = inputs(M, L)
    big, ebig, sel = gather(W, e)
    agg = amd.engine.Aggregator(M, 1, L, amd.dev)
    for kc in kcounts(L):
        a = TK.corrected(W, x, e)
        tau, n, _ = TK.threshold(a, kc)
        for rows, Wh, eh in ((None, W, e), (sel, big, ebig)):
            xd, ed = dv(amd, x), dv(amd, eh)
            td = torch.full((M,), -1.0, device=amd.dev)
            kd = torch.full((M,), -1, dtype=torch.int32, device=amd.dev)
            agg.topk_threshold(dv(amd, Wh), xd, ed, kc, td, kd, sel=dv(amd, rows), M=M)
            same(td.cpu().numpy(), tau.view(F32), (M, L, kc, 'tau'))
            same(kd.cpu().numpy(), n, (M, L, kc, 'kept'))
            same(xd.cpu().numpy(), x, (M, L, kc, 'W_g is not written'))
            ge = ed.cpu().numpy()
            same(ge if rows is None else ge[rows], a, (M, L, kc, 'a in e'))
            if rows is not None:
                assert (ge[np.setdiff1d(np.arange(2 * M), rows)] == SENTINEL).all()
        # without memory: the thresholds of W - x, nothing else written
        tau0, n0, _ = TK.threshold(TK.corrected(W, x), kc)
        td = torch.full((M,), -1.0, device=amd.dev)
        kd = torch.full((M,), -1, dtype=torch.int32, device=amd.dev)
        agg.topk_threshold(dv(amd, W), dv(amd, x), None, kc, td, kd, M=M)
        same(td.cpu().numpy(), tau0.view(F32), (M, L, kc, 'tau, no memory'))
        same(kd.cpu().numpy(), n0, (M, L, kc, 'kept, no memory'))


def test_workspace_size_is_exported(amd):
    assert amd.engine.topk_ws_bytes(100, 4096) == 0 and amd.engine.topk_ws_bytes(1250, 28672) == 0


def test_einval_leaves_every_output_unchanged(amd):
    """Every FS_EINVAL case returns before any launch: sentinel-filled outputs keep their bits."""
    lib = amd.lib.lib()
    M, L, stride = 5, 36, 40
    dev = amd.dev
    W = torch.randn(M, stride, device=dev)
    q = torch.full((M,), 0.2, device=dev)
    sel = torch.arange(M, dtype=torch.int32, device=dev)

    def fresh():
        return dict(x=torch.full((L,), 3.0, device=dev), e=torch.full((M, stride), 5.0, device=dev),
                    tau=torch.full((M,), -1.0, device=dev), kept=torch.full((M,), -7, dtype=torch.int32, device=dev),
                    ws=torch.full((4 * L,), 9.0, device=dev))

    def p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    good = dict(W=W, stride=stride, sel=sel, q=q, M=M, L=L, kc=4, ws_floats=4 * L, chunks=0, sws_bytes=0)
    cases = {
        'M < 1': dict(M=0),
        'kcount < 1': dict(kc=0),
        'kcount > len': dict(kc=L + 1),
        'len no multiple of 4': dict(L=34),
        'stride no multiple of 4': dict(stride=38),
        'stride < len': dict(stride=32),
        'null W_all': dict(W=None),
        'null q': dict(q=None),
        'null W_g': dict(x=None),
        'null tau': dict(tau=None),
        'null kept': dict(kept=None),
        'workspace too small': dict(sws_bytes=-1),
        'e is W_all': dict(e=W),
        'e is W_g': dict(e='x'),
    }
    for name, change in cases.items():
        for entry in ('aggregate', 'threshold'):
            if entry == 'threshold' and name == 'null q':
                continue
            a = dict(good)
            out = fresh()
            bufs = dict(out)
            for k, v in change.items():
                if k in bufs:
                    bufs[k] = bufs['x'] if isinstance(v, str) else v
                else:
                    a[k] = v
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if entry == 'aggregate':
                rc = lib.fs_aggregate_topk(p(a['W']), a['stride'], p(a['sel']), p(a['q']), a['M'], a['L'], a['kc'],
                                           p(bufs['x']), p(bufs['e']), p(bufs['tau']), p(bufs['kept']), p(out['ws']),
                                           a['ws_floats'], a['chunks'], None, a['sws_bytes'], st)
            else:
                rc = lib.fs_topk_threshold(p(a['W']), a['stride'], p(a['sel']), a['M'], a['L'], p(bufs['x']),
                                           p(bufs['e']), a['kc'], p(bufs['tau']), p(bufs['kept']), None,
                                           a['sws_bytes'], st)
            assert rc == -1, (name, entry, rc)                                   # FS_EINVAL
            assert lib.fs_last_error(), (name, entry)
            torch.cuda.synchronize()
            assert bool((out['x'] == 3.0).all()) and bool((out['e'] == 5.0).all()), (name, entry)
            assert bool((out['tau'] == -1.0).all()) and bool((out['kept'] == -7).all()), (name, entry)
            assert bool((out['ws'] == 9.0).all()), (name, entry)
    # d_sel, d_e, d_ws and d_sws may be NULL
    out = fresh()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.fs_aggregate_topk(p(W), stride, None, p(q), M, L, 4, p(out['x']), None, p(out['tau']), p(out['kept']), None,
                               0, 0, None, 0, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out['kept'] >= 4).all()) and bool((out['e'] == 5.0).all()) and not bool((out['x'] == 3.0).all())

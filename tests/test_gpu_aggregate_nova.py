"""fs_aggregate_nova at kernel level: its reduction to fs_aggregate / fs_aggregate_sel, the exact
left fold (the test of the correctly rounded division), the summation bound in the other regimes,
in-place operation of the update form, and argument validation.

Shapes: M in {1, 2, 15, 16, 48, 513} -- one sub-range, the first two sub-ranges, eight, and the
two-stage form with 8 chunks of 65 -- at len in {4, 192, 1028} (one float4, a count that does not
fill a workgroup, one float4 past a workgroup; M = 513 at len <= 192 only), chunks in {0, 1} and 3
at M = 20.  Every shape runs on rows 0..M-1 (d_sel NULL) and on a strictly ascending subset of a
2M-row buffer whose other rows hold NaN: a NaN in the result would show they were read."""
import functools

import numpy as np
import pytest
import torch

from tests import fednova_restatement as FR

pytestmark = pytest.mark.gpu

SHAPES = [(M, L, c) for M in (1, 2, 15, 16, 48, 513) for L in (4, 192, 1028) for c in (0, 1) if M < 513 or L <= 192]
SHAPES += [(20, L, 3) for L in (4, 192, 1028)]
TE, S0 = 4.9876, 0.731
U = 2.0 ** -24


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


@functools.lru_cache(maxsize=None)
def case(M, L, gathered):
    """Host inputs of one shape, built once: W [rows, L], sel (None: rows 0..M-1), q from unequal
    client sizes, b in [0.1, 40] (no powers of two), base."""
    rs = np.random.RandomState(1000 * M + L + (7 if gathered else 0))
    if gathered:
        sel = np.sort(rs.permutation(2 * M)[:M]).astype(np.int32)
        W = np.full((2 * M, L), np.nan, np.float32)
        W[sel] = rs.normal(size=(M, L)).astype(np.float32)
    else:
        sel = None
        W = rs.normal(size=(M, L)).astype(np.float32)
    n = rs.randint(1, 200, size=M)
    q = (n / n.sum()).astype(np.float32)
    b = rs.uniform(0.1, 40.0, size=M).astype(np.float32)
    assert not np.any(np.log2(b) == np.round(np.log2(b)))
    base = rs.normal(size=L).astype(np.float32)
    rows = [W[j] for j in (sel if gathered else range(M))]
    for a in (W, q, b, base):
        a.setflags(write=False)
    return dict(M=M, L=L, W=W, sel=sel, q=q, b=b, base=base, rows=rows)


def run(amd, cs, chunks, mode, q=None, b=None, te=TE, s0=S0, base=None, in_place=False):
    dev = amd.dev
    t = lambda a: None if a is None else torch.tensor(a, device=dev)   # noqa: E731
    agg = amd.engine.Aggregator(cs['M'], 1, cs['L'], dev, chunks=chunks)
    q = cs['q'] if q is None else q
    if mode == 1:
        out = torch.full((cs['L'],), np.nan, device=dev)
        agg.run_nova(t(cs['W']), t(q), out, 1, b=t(cs['b'] if b is None else b), te=te, s0=s0, sel=t(cs['sel']))
    else:
        bs = t(cs['base'] if base is None else base)
        out = bs if in_place else torch.full((cs['L'],), np.nan, device=dev)
        agg.run_nova(t(cs['W']), t(q), out, 2, base=bs, sel=t(cs['sel']))
    return out.cpu().numpy()


def plain(amd, cs, chunks):
    """fs_aggregate (rows 0..M-1) or fs_aggregate_sel (gathered) on the same inputs."""
    dev = amd.dev
    agg = amd.engine.Aggregator(cs['M'], 1, cs['L'], dev, chunks=chunks)
    W, q = torch.tensor(cs['W'], device=dev), torch.tensor(cs['q'], device=dev)
    out = torch.full((cs['L'],), np.nan, device=dev)
    if cs['sel'] is None:
        return agg.run(W, q, out).cpu().numpy()
    return agg.run_sel(W, torch.tensor(cs['sel'], device=dev), q, out).cpu().numpy()


def left_fold_regime(M, chunks):
    return M < 16 or chunks == 1


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_reduces_to_the_plain_aggregate(amd, M, L, chunks):
    """(a) mode 1 with te = 1, b == 1, s0 = q_0 is bitwise fs_aggregate / fs_aggregate_sel; mode 2
    with a zero base equals them numerically (-0 == 0)."""
    for gathered in (False, True):
        cs = case(M, L, gathered)
        ref = plain(amd, cs, chunks)
        assert np.isfinite(ref).all()
        got1 = run(amd, cs, chunks, 1, b=np.ones(M, np.float32), te=1.0, s0=float(cs['q'][0]))
        assert got1.tobytes() == ref.tobytes(), (gathered, np.abs(got1 - ref).max())
        got2 = run(amd, cs, chunks, 2, base=np.zeros(L, np.float32))
        assert np.array_equal(got2, ref), (gathered, np.abs(got2 - ref).max())


@pytest.mark.parametrize('M,L,chunks', [s for s in SHAPES if left_fold_regime(s[0], s[2])])
def test_left_fold_regime_is_bitwise_numpy(amd, M, L, chunks):
    """(b) M < 16 or chunks = 1: both modes are bitwise the float32 numpy left fold, every operation
    rounded separately -- for mode 1 the test of the correctly rounded division."""
    for gathered in (False, True):
        cs = case(M, L, gathered)
        ref1 = FR.aggregate_reference(cs['rows'], cs['q'], cs['b'], np.float32(TE), np.float32(S0), np.float32)
        got1 = run(amd, cs, chunks, 1)
        bad = np.flatnonzero(got1 != ref1)
        assert got1.tobytes() == ref1.tobytes(), (gathered, len(bad), got1[bad[:4]], ref1[bad[:4]])
        ref2 = FR.aggregate_updates(cs['rows'], cs['q'], cs['base'], np.float32)
        got2 = run(amd, cs, chunks, 2)
        assert got2.tobytes() == ref2.tobytes(), (gathered, np.abs(got2 - ref2).max())


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_summation_bound_in_every_regime(amd, M, L, chunks):
    """(c) per element |got - ref64| <= (M + 3) 2^-24 sum_k |term_k|, ref64 and the terms in float64:
    the standard bound of a sum of M terms in any order ((M - 1) u sum|term|) plus the roundings
    inside a term (mode 1: two products and a quotient, 3u; mode 2: a difference and a product, and
    the base as one more term of the final sum) -- nothing fitted."""
    for gathered in (False, True):
        cs = case(M, L, gathered)
        R = np.stack(cs['rows']).astype(np.float64)
        q, b, base = cs['q'].astype(np.float64), cs['b'].astype(np.float64), cs['base'].astype(np.float64)
        te, s0 = float(np.float32(TE)), float(np.float32(S0))
        coef = q * te / b
        coef[0] = s0
        terms1 = coef[:, None] * R
        got1 = run(amd, cs, chunks, 1).astype(np.float64)
        err1, bound1 = np.abs(got1 - terms1.sum(0)), (M + 3) * U * np.abs(terms1).sum(0)
        terms2 = q[:, None] * (R - base)
        got2 = run(amd, cs, chunks, 2).astype(np.float64)
        err2 = np.abs(got2 - (base + terms2.sum(0)))
        bound2 = (M + 3) * U * (np.abs(base) + np.abs(terms2).sum(0))
        print('M %d len %d chunks %d gathered %d: mode 1 max err/bound %.3f, mode 2 %.3f'
              % (M, L, chunks, gathered, (err1 / bound1).max(), (err2 / bound2).max()))
        assert (err1 <= bound1).all() and (err2 <= bound2).all()


@pytest.mark.parametrize('M', [15, 48, 513])
@pytest.mark.parametrize('chunks', [0, 1])
def test_update_form_in_place(amd, M, chunks):
    """(d) mode 2 with d_W_base == d_W_bar equals the out-of-place call, bitwise."""
    for L in (4, 192):
        for gathered in (False, True):
            cs = case(M, L, gathered)
            out = run(amd, cs, chunks, 2)
            inp = run(amd, cs, chunks, 2, in_place=True)
            assert np.isfinite(out).all() and not np.array_equal(out, cs['base'])
            assert inp.tobytes() == out.tobytes(), (L, gathered)


def test_bad_arguments_leave_the_output_untouched(amd):
    """(e) every bad argument returns FS_EINVAL with a message; the output (7.0) is not written."""
    dev, L = amd.dev, amd.lib.lib()
    M, n = 4, 64
    W = torch.randn(M, n, device=dev)
    q = torch.full((M,), 0.25, device=dev)
    b = torch.full((M,), 3.0, device=dev)
    base = torch.zeros(n, device=dev)
    out = torch.full((n,), 7.0, device=dev)
    ws = torch.empty(4 * n, device=dev)
    P = amd.lib.ptr

    def call(W_=W, stride=n, q_=q, b_=b, mode=1, base_=base, M_=M, len_=n, out_=out):
        p = lambda x: None if x is None else P(x)   # noqa: E731
        return L.fs_aggregate_nova(p(W_), stride, None, p(q_), p(b_), 1.0, 1.0, mode, p(base_), M_, len_, p(out_),
                                   P(ws), ws.numel(), 0, amd.lib.stream_ptr())

    bad = [dict(M_=0), dict(len_=62), dict(stride=66), dict(W_=None), dict(q_=None), dict(out_=None),
           dict(mode=1, b_=None), dict(mode=2, base_=None), dict(mode=0), dict(mode=3)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert 'fs_aggregate_nova' in L.fs_last_error().decode() or 'aggregate_nova_launch' in L.fs_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0 and call(mode=2, b_=None) == 0            # (and the good calls do write it)
    torch.cuda.synchronize()
    assert bool((out != 7.0).all())

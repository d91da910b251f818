"""fs_aggregate_robust at kernel level: bitwise tests/robust_restatement.py (NaN as NaN).

M in {1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 257, 1250}, the first M of each narrower stripe (1262: 16
columns, 2524: 8 columns) and fs_aggregate_robust_max_m() = 5047; M = max_m + 1 is an error without a
launch.  len in {4, 32, 36, 132}: one float4 lane, one full 32-column stripe, a ragged last stripe,
several stripes.  b in {0, 1, (M-1)//4, (M-1)//2} where valid.  Contiguous rows and the same rows
gathered from a buffer of twice as many, NaN in the rows outside the sample."""
import numpy as np
import pytest
import torch

from tests import robust_restatement as RR

pytestmark = pytest.mark.gpu

F32 = np.float32
MS = (1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 257, 1250, RR.MAX_M32 + 1, RR.MAX_M16 + 1, RR.MAX_M)
LENS = (4, 32, 36, 132)


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


def bs(M):
    return sorted({b for b in (0, 1, (M - 1) // 4, (M - 1) // 2) if 2 * b < M})


def gather(W, seed=9):
    """The same rows in the same order, scattered over a buffer of twice as many rows, NaN elsewhere."""
    M, L = W.shape
    sel = np.sort(np.random.RandomState(seed + M).permutation(2 * M)[:M]).astype(np.int32)
    big = np.full((2 * M, L), np.nan, F32)
    big[sel] = W
    return big, sel


def run(amd, W, b, sel=None, M=None, out=None, calls=1):
    """``calls`` launches on the rows of W (sel: gathered); the outputs as numpy."""
    dev = amd.dev
    M = (W.shape[0] if sel is None else len(sel)) if M is None else M
    agg = amd.engine.Aggregator(M, 1, W.shape[1], dev)
    Wd = torch.from_numpy(np.ascontiguousarray(W)).to(dev)
    sd = None if sel is None else torch.from_numpy(sel).to(dev)
    res = []
    for _ in range(calls):
        o = torch.full((W.shape[1],), 7.0, device=dev) if out is None else out
        agg.run_robust(Wd, b, o, sel=sd)
        res.append(o.cpu().numpy().copy())
    return res


def same(got, ref, what):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    bad = np.flatnonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    assert RR.same_bits(got, ref), (what, len(bad), got[bad[:4]], ref[bad[:4]], bad[:4])


def test_max_m(amd):
    assert amd.engine.robust_max_m() == RR.MAX_M >= 2048 and RR.width(1250) == 32


@pytest.mark.parametrize('M', MS)
def test_bitwise_the_restatement(amd, M):
    """Random normals at every len and b, contiguous and gathered, twice: the restatement's bits, the
    same bits on the second call and from the larger buffer."""
    for L in LENS:
        W = RR.inputs('normal', M, L)
        big, sel = gather(W)
        for b in bs(M):
            ref = RR.robust(W, b)
            assert np.isfinite(ref).all()
            a1, a2 = run(amd, W, b, calls=2)
            same(a1, ref, (M, L, b, 'contiguous'))
            same(a2, a1, (M, L, b, 'second call'))
            same(run(amd, big, b, sel=sel)[0], ref, (M, L, b, 'gathered'))


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('kind', ['quantised', 'equal', 'zeros', 'wide', 'near_one', 'digits'])
def test_ties_and_key_order(amd, M, kind):
    """At most 3 distinct values per column, all-equal columns, +-0, mixed signs over 1e-30 .. 1e30, and
    keys that differ in one 4-bit digit only (len 36: column j in digit j % 8)."""
    W = RR.inputs(kind, M, 36)
    for b in bs(M):
        same(run(amd, W, b)[0], RR.robust(W, b), (M, kind, b))


@pytest.mark.parametrize('M', [3, 5, 9, 64, 257, 1250, RR.MAX_M16 + 1])
def test_b_outlier_rows_per_side_are_discarded(amd, M):
    """b rows of +-Inf / NaN (either sign) per side, gathered: finite, the restatement's bits, and per
    coordinate within the min and max of the other rows; with one more NaN row a bad value survives."""
    rs = np.random.RandomState(M)
    for b in [x for x in bs(M) if x > 0]:
        W = RR.inputs('normal', M, 36)
        nneg = np.array([0xFFC00000], np.uint32).view(F32)[0]
        rows = rs.permutation(M)
        top, bot = rows[:b], rows[b:2 * b]
        W[top] = np.where(rs.randint(0, 2, size=(b, 36)) == 1, np.nan, np.inf).astype(F32)
        W[bot] = np.where(rs.randint(0, 2, size=(b, 36)) == 1, nneg, -np.inf).astype(F32)
        big, sel = gather(W)
        out = run(amd, big, b, sel=sel)[0]
        same(out, RR.robust(W, b), (M, b))
        clean = np.delete(W, rows[:2 * b], 0)
        assert np.isfinite(out).all() and (out >= clean.min(0)).all() and (out <= clean.max(0)).all()
        # one more NaN row: the smallest of the b + 1 top values survives the trim -- +Inf where a top row
        # held one, NaN where all of them were NaN
        all_nan = np.isnan(W[top]).all(0)
        W[rows[2 * b]] = np.nan
        out = run(amd, W, b)[0]
        same(out, RR.robust(W, b), (M, b, 'one more'))
        assert (np.isnan(out) == all_nan).all() and np.isposinf(out[~all_nan]).all()


@pytest.mark.parametrize('M,f', [(9, 2), (65, 16), (257, 64)])
def test_range_property_with_arbitrary_rows(amd, M, f):
    """f <= b rows of arbitrary bits: every output coordinate lies within the other rows' min and max."""
    rs = np.random.RandomState(3 * M)
    W = RR.inputs('normal', M, 132)
    bad = rs.permutation(M)[:f]
    W[bad] = rs.randint(0, 2 ** 32, size=(f, 132), dtype=np.uint64).astype(np.uint32).view(F32)
    clean = np.delete(W, bad, 0)
    for b in (f, (M - 1) // 2):
        out = run(amd, W, b)[0]
        same(out, RR.robust(W, b), (M, b))
        assert (out >= clean.min(0)).all() and (out <= clean.max(0)).all()


def test_output_may_be_the_global_model(amd):
    """d_out = a separate W_g buffer that held other values: overwritten whole, nothing else touched."""
    M, L = 65, 132
    W = RR.inputs('normal', M, L)
    buf = torch.full((L + 8,), 3.0, device=amd.dev)
    out = run(amd, W, 16, out=buf[:L])[0]
    same(out, RR.robust(W, 16), 'W_g')
    assert bool((buf[L:] == 3.0).all())


def test_errors_return_without_a_launch(amd):
    dev = amd.dev
    L = amd.lib.lib()
    W = torch.zeros(4, 8, device=dev)
    out = torch.full((8,), 5.0, device=dev)
    p = amd.lib.ptr
    for M, b, ln in ((0, 0, 8), (RR.MAX_M + 1, 0, 8), (4, 2, 8), (3, 2, 8), (4, -1, 8), (4, 1, 6)):
        assert L.fs_aggregate_robust(p(W), ln, None, M, ln, b, p(out), amd.lib.stream_ptr()) < 0, (M, b, ln)
    agg = amd.engine.Aggregator(RR.MAX_M + 1, 1, 4, dev)
    with pytest.raises(ValueError, match='max_m'):
        agg.run_robust(torch.zeros(RR.MAX_M + 1, 4, device=dev), 0, torch.zeros(4, device=dev))
    with pytest.raises(amd.lib.FedsimError, match='2b < M'):
        amd.engine.Aggregator(4, 1, 8, dev).run_robust(W, 2, out)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


def test_finaliser_rides_and_gives_fs_evals_numbers(amd):
    """A deferred evaluation fused into the next TRAIN launch leaves its finaliser to the robust
    aggregate's extra last workgroup: the models are bitwise the undeferred run's, the test metrics
    fs_eval's to the 1e-12 relative the header states for a fused deferral."""
    from fedamw_amd.functions import tools
    tune = dict(train_form=1, split_mb=-1, split_dbuf=-1, split_pipe=-1, split_teams=-1)
    C, Nc, R, D, n_t = 10, 10, 3, 1024, 16 * 16 + 5
    rs = np.random.RandomState(17)
    sizes = rs.randint(8, 41, size=Nc)
    Xs = [torch.from_numpy((np.cos(rs.normal(size=(n, D))) / np.sqrt(D)).astype(F32)) for n in sizes]
    ys = [torch.from_numpy(rs.randint(0, C, size=n).astype(np.int64)) for n in sizes]
    Xt = torch.from_numpy((np.cos(rs.normal(size=(n_t, D))) / np.sqrt(D)).astype(F32))
    yt = torch.from_numpy(rs.randint(0, C, size=n_t).astype(np.int64))
    runs = {}
    with amd.lib.tuning(**tune):
        for defer in (False, True):
            stats = {'trace': True}
            torch.manual_seed(11)
            fed = tools.Federation('fedrobust', Xs, ys, Xt, yt, None, 'classification', C, D, 0.5, 1, 32, False, 0.0,
                                   False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False,
                                   options={'defer_eval': defer}, robust=dict(rule='trimmed_mean', trim=0.2))
            for _ in range(R):
                fed.round()
            fed.results()
            assert fed.plan.eval_blocks() > 0
            runs[defer] = (stats['W_rounds'], fed.eval_hist.cpu().numpy().copy())
    assert np.array_equal(runs[False][0], runs[True][0]) and np.isfinite(runs[True][0]).all()
    assert np.isfinite(runs[True][1]).all()
    np.testing.assert_allclose(runs[True][1], runs[False][1], rtol=1e-12, atol=0)

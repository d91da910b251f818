"""fs_krum_select, fs_krum_distances and fs_aggregate_krum at kernel level: three separate contracts, so
that no pick is ever ambiguous.

(a) fs_krum_select on host-made D: bitwise restatement (ii) of tests/krum_restatement.py.
(b) fs_krum_distances: within the a-priori bound of include/fedsim.h of restatement (i); exactly
    symmetric, a zero diagonal, +Inf in exactly the rows and columns of NaN / Inf / overflowing rows,
    the same bits from a larger buffer and on a second call.
(c) fs_aggregate_krum: scores and pick bitwise restatement (ii) applied to the D the device produced,
    the output bitwise ``Aggregator.run_sel`` on the pick with q == 1 / m; the error returns; the
    finaliser of a deferred evaluation."""
import numpy as np
import pytest
import torch

from tests import krum_restatement as KR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def padded(D):
    """D [M, M] in the device layout [M, ldD], the padding columns NaN (they are never read)."""
    M = D.shape[0]
    out = np.full((M, KR.ldd(M)), np.nan, F32)
    out[:, :M] = D
    return out


def gather(W, seed=9):
    """The same rows in the same order, scattered over a buffer of twice as many rows, NaN elsewhere."""
    M, L = W.shape
    sel = np.sort(np.random.RandomState(seed + M).permutation(2 * M)[:M]).astype(np.int32)
    big = np.full((2 * M, L), np.nan, F32)
    big[sel] = W
    return big, sel


# ---- (a) ----

def run_select(amd, D, f, m, sel=None):
    dev = amd.dev
    M = D.shape[0]
    Dd = to_dev(padded(D), dev)
    score = torch.full((M,), -1.0, dtype=torch.float64, device=dev)
    pick = torch.full((m + 2,), -7, dtype=torch.int32, device=dev)
    q = torch.full((m + 2,), 9.0, device=dev)
    amd.engine.krum_select(Dd, M, f, m, score, pick, q, None if sel is None else to_dev(sel, dev))
    pick, q = pick.cpu().numpy(), q.cpu().numpy()
    assert pick[m:].tolist() == [-7, -7] and q[m:].tolist() == [9.0, 9.0]
    return score.cpu().numpy(), pick[:m], q[:m]


def check_select(amd, D, f, m, what, sel=None):
    s, pk, q = run_select(amd, D, f, m, sel)
    rs, rpk, rq = KR.select(D, f, m, sel)
    bad = np.flatnonzero(s.view(np.uint64) != rs.view(np.uint64))
    assert KR.same_bits(s, rs), (what, 'score', len(bad), bad[:4], s[bad[:4]], rs[bad[:4]])
    assert KR.same_bits(pk, rpk), (what, 'pick', pk[:8], rpk[:8])
    assert KR.same_bits(q, rq), (what, 'q')


@pytest.mark.parametrize('name', sorted(KR.hand_made()))
def test_select_hand_made(amd, name):
    D, f, m = KR.hand_made()[name]
    check_select(amd, D, f, m, name)
    M = D.shape[0]
    check_select(amd, D, f, m, name + ' sel', sel=(3 * np.arange(M) + 2).astype(np.int32))


@pytest.mark.parametrize('M', [3, 4, 5, 16, 17, 63, 64, 65, 129, 257, 1262, KR.MAX_M])
def test_select_bitwise_the_restatement(amd, M):
    """Random distances (continuous: no ties; quantised to three values: ties everywhere; a tenth of the
    rows at +Inf) at several (f, m)."""
    fms = KR.fm_cases(M) if M <= 1262 else [(0, 1), (M // 10, M - M // 10), ((M - 3) // 2, 7)]
    for kind in ('continuous', 'quantised', 'inf'):
        D = KR.random_D(M, quantised=kind == 'quantised', n_inf=M // 10 if kind == 'inf' else 0)
        for f, m in (fms if kind == 'continuous' or M <= 257 else fms[:2]):
            check_select(amd, D, f, m, (M, kind, f, m))


# ---- (b) ----

def run_distances(amd, W, x, sel=None, calls=1):
    dev = amd.dev
    M = W.shape[0] if sel is None else len(sel)
    L = W.shape[1]
    agg = amd.engine.Aggregator(M, 1, L, dev)
    Wd, xd = to_dev(W, dev), to_dev(x, dev)
    sd = None if sel is None else to_dev(sel, dev)
    ws = agg.krum_ws()
    out = []
    for _ in range(calls):
        D = torch.full((M, KR.ldd(M)), -3.0, device=dev)
        agg.krum_distances(Wd, xd, D, ws, sel=sd)
        D = D.cpu().numpy()
        assert (D[:, M:] == -3.0).all()                     # the padding columns are not written
        out.append(np.ascontiguousarray(D[:, :M]))
    return out


def check_distances(amd, M, L, worst):
    # Gaussian updates of scale 1e-3 about |x| ~ 1 (the cancellation case), the last row a copy of row 0
    W, x = KR.rows('duplicate', M, L)
    D64, n2 = KR.distances64(W, x)
    bound = KR.dist_bound(D64, n2, M, L)
    d1, d2 = run_distances(amd, W, x, calls=2)
    big, sel = gather(W)
    dg = run_distances(amd, big, x, sel=sel)[0]
    assert KR.same_bits(d2, d1), (M, L, 'second call')
    assert KR.same_bits(dg, d1), (M, L, 'gathered')
    assert KR.same_bits(d1, np.ascontiguousarray(d1.T)), (M, L, 'symmetry')
    assert (np.diag(d1) == 0).all() and not np.signbit(np.diag(d1)).any()
    assert np.isfinite(d1).all() and (d1 >= 0).all()
    err = np.abs(d1.astype(F64) - D64)
    ratio = float((err / bound)[~np.eye(M, dtype=bool)].max())
    print('M %d len %d chain %d: worst |err| / bound %.4f; duplicate pair D = %.3g (bound %.3g)'
          % (M, L, KR.chain(M, L), ratio, d1[0, M - 1], bound[0, M - 1]))
    worst.append(ratio)
    assert (err <= bound).all(), (M, L, ratio)
    assert D64[0, M - 1] == 0.0 or D64[0, M - 1] <= bound[0, M - 1]
    return W, x, d1


@pytest.mark.parametrize('M', [3, 17, 63, 64, 65, 127, 128, 129, 257])
def test_distances_within_the_a_priori_bound(amd, M):
    worst = []
    for L in (4, 64, 260, 4096, 20480):
        W, x, d1 = check_distances(amd, M, L, worst)
        # one NaN row, one Inf row, one 1e30 row (overflow): +Inf in exactly its row and column
        Wb, _ = KR.rows('bad', M, L)
        bad = KR.bad_rows(M)
        good = np.setdiff1d(np.arange(M), bad)
        db = run_distances(amd, Wb, x)[0]
        mask = np.zeros((M, M), dtype=bool)
        mask[bad, :] = True
        mask[:, bad] = True
        mask &= ~np.eye(M, dtype=bool)
        assert np.isposinf(db[mask]).all() and np.isfinite(db[~mask]).all(), (M, L)
        assert KR.same_bits(db, np.ascontiguousarray(db.T)) and (np.diag(db) == 0).all()
        # the other rows are untouched by their neighbours in the tile: the bits of the clean run (the
        # 'bad' family differs from the 'gaussian' one in the bad rows only)
        Wc, _ = KR.rows('gaussian', M, L)
        dc = run_distances(amd, Wc, x)[0]
        assert KR.same_bits(db[np.ix_(good, good)], dc[np.ix_(good, good)]), (M, L, 'good rows')
        assert np.isfinite(db[np.ix_(good, good)]).all()
    print('M %d: worst ratio over the lens %.4f' % (M, max(worst)))


def test_distances_at_max_m(amd):
    check_distances(amd, KR.MAX_M, 64, [])


def test_split_is_the_restatements(amd):
    for M in (3, 100, 257, 1000, KR.MAX_M):
        for L in (4, 260, 4096, 20480, 28672):
            assert amd.engine.krum_split(M, L) == KR.split(M, L)


# ---- (c) ----

def run_chain(amd, W, x, f, m, sel=None, alias=False, chunks=0):
    dev = amd.dev
    M = W.shape[0] if sel is None else len(sel)
    L = W.shape[1]
    agg = amd.engine.Aggregator(M, 1, L, dev, chunks=chunks)
    Wd, xd = to_dev(W, dev), to_dev(x, dev)
    sd = None if sel is None else to_dev(sel, dev)
    ws = agg.krum_ws()
    out = xd if alias else torch.full((L,), 7.0, device=dev)
    pick = torch.full((m + 1,), -7, dtype=torch.int32, device=dev)
    score = torch.full((M,), -1.0, dtype=torch.float64, device=dev)
    agg.run_krum(Wd, xd, f, m, out, pick, score, ws, sel=sd)
    D = ws[:4 * M * KR.ldd(M)].view(torch.float32).view(M, KR.ldd(M))[:, :M].cpu().numpy()
    ref = torch.full((L,), 5.0, device=dev)
    agg.run_sel(Wd, pick[:m].contiguous(), torch.full((m,), float(F32(1.0 / m)), device=dev), ref)
    assert int(pick[m]) == -7
    return np.ascontiguousarray(D), score.cpu().numpy(), pick[:m].cpu().numpy(), out.cpu().numpy(), ref.cpu().numpy()


@pytest.mark.parametrize('M', [3, 17, 65, 129, 600])
def test_chain_is_the_restatement_on_the_devices_own_D(amd, M):
    for L in (4, 260, 4096):
        W, x = KR.rows('bad' if M == 65 else 'gaussian', M, L)
        big, sel = gather(W)
        for f, m in [(0, 1), ((M - 3) // 2, 1), (M // 10, M - M // 10), (M // 10, (M - M // 10 + 1) // 2)]:
            D, s, pk, out, ref = run_chain(amd, W, x, f, m)
            rs, rpk, _ = KR.select(D, f, m)
            assert KR.same_bits(s, rs), (M, L, f, m, 'score')
            assert KR.same_bits(pk, rpk), (M, L, f, m, 'pick', pk[:8], rpk[:8])
            assert KR.same_bits(out, ref), (M, L, f, m, 'out')
            if m == 1 and np.isfinite(W[pk[0]]).all():
                assert KR.same_bits(out, W[pk[0]])           # 1.0f * w is exact: the picked row's bits
            if M == 65:
                assert not set(pk.tolist()) & set(KR.bad_rows(M)) or f < 3
        # gathered from a larger buffer: the same D and scores, the ids of the larger buffer, the same output
        f, m = M // 10, M - M // 10
        D, s, pk, out, ref = run_chain(amd, W, x, f, m)
        Dg, sg, pkg, outg, refg = run_chain(amd, big, x, f, m, sel=sel)
        assert KR.same_bits(Dg, D) and KR.same_bits(sg, s) and KR.same_bits(pkg, sel[KR.pick(s, m)])
        assert KR.same_bits(outg, refg) and KR.same_bits(outg, out)
        # d_out aliasing x, and another chunk count of the fold
        Da, sa, pka, outa, refa = run_chain(amd, W, x, f, m, alias=True)
        assert KR.same_bits(Da, D) and KR.same_bits(pka, pk) and KR.same_bits(outa, out)
        D1, s1, pk1, out1, ref1 = run_chain(amd, W, x, f, m, chunks=1)
        assert KR.same_bits(pk1, pk) and KR.same_bits(out1, ref1)


def test_errors_return_without_a_launch(amd):
    dev = amd.dev
    L = amd.lib.lib()
    p = amd.lib.ptr
    M, ln = 5, 8
    W = torch.zeros(M, ln, device=dev)
    x = torch.zeros(ln, device=dev)
    out = torch.full((ln,), 5.0, device=dev)
    pick = torch.full((M,), -7, dtype=torch.int32, device=dev)
    score = torch.full((M,), -1.0, dtype=torch.float64, device=dev)
    ws = torch.full((int(L.fs_aggregate_krum_ws_bytes(M, ln)),), 3, dtype=torch.uint8, device=dev)
    D = torch.full((M, 8), 2.0, device=dev)
    st = amd.lib.stream_ptr()

    def chain(M=M, f=1, m=1, ln=ln, stride=ln, W=p(W), x=p(x), out=p(out), pick=p(pick), score=p(score), ws=p(ws),
              nbytes=ws.numel()):
        return L.fs_aggregate_krum(W, stride, None, M, ln, x, f, m, out, pick, score, ws, nbytes, None, 0, 0, st)

    assert L.fs_aggregate_krum_max_m() == KR.MAX_M
    for kw in (dict(M=2), dict(f=-1), dict(f=3), dict(m=0), dict(m=5), dict(M=KR.MAX_M + 1), dict(ln=6), dict(stride=6),
               dict(stride=4), dict(ln=0), dict(nbytes=ws.numel() - 1), dict(nbytes=0), dict(W=None), dict(x=None),
               dict(out=None), dict(pick=None), dict(score=None), dict(ws=None)):
        assert chain(**kw) < 0, kw
    rank = torch.full((M,), -9, dtype=torch.int32, device=dev)
    for args in ((None, M, 1, 1, None, p(score), p(pick), None, p(rank), st),
                 (p(D), 2, 0, 1, None, p(score), p(pick), None, p(rank), st),
                 (p(D), M, 3, 1, None, p(score), p(pick), None, p(rank), st),
                 (p(D), M, 1, 5, None, p(score), p(pick), None, p(rank), st),
                 (p(D), M, 1, 1, None, None, p(pick), None, p(rank), st),
                 (p(D), M, 1, 1, None, p(score), None, None, p(rank), st),
                 (p(D), M, 1, 1, None, p(score), p(pick), None, None, st),
                 (p(D), KR.MAX_M + 1, 1, 1, None, p(score), p(pick), None, p(rank), st)):
        assert L.fs_krum_select(*args) < 0, args
    for args in ((p(W), ln, None, 2, ln, p(x), p(D), p(ws), ws.numel(), st),
                 (p(W), ln, None, M, 6, p(x), p(D), p(ws), ws.numel(), st),
                 (p(W), 4, None, M, ln, p(x), p(D), p(ws), ws.numel(), st),
                 (p(W), ln, None, M, ln, None, p(D), p(ws), ws.numel(), st),
                 (p(W), ln, None, M, ln, p(x), None, p(ws), ws.numel(), st),
                 (p(W), ln, None, M, ln, p(x), p(D), p(ws), 8, st)):
        assert L.fs_krum_distances(*args) < 0, args
    agg = amd.engine.Aggregator(KR.MAX_M + 1, 1, 4, dev)
    with pytest.raises(ValueError, match='max_m'):
        agg.run_krum(torch.zeros(KR.MAX_M + 1, 4, device=dev), torch.zeros(4, device=dev), 1, 1,
                     torch.zeros(4, device=dev), pick, torch.zeros(KR.MAX_M + 1, dtype=torch.float64, device=dev), ws)
    with pytest.raises(amd.lib.FedsimError, match=r'm must be in \[1, M - f\]'):
        amd.engine.Aggregator(M, 1, ln, dev).run_krum(W, x, 1, 5, out, pick, score, ws)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((pick == -7).all()) and bool((score == -1.0).all())
    assert bool((ws == 3).all()) and bool((D == 2.0).all()) and bool((rank == -9).all())
    assert chain() == 0                                      # the same arguments, unchanged, do launch
    torch.cuda.synchronize()
    assert bool((score >= 0).all()) and int(pick[0]) == 0 and bool((out == 0).all())


def test_finaliser_rides_and_gives_fs_evals_numbers(amd):
    """A deferred evaluation fused into the next TRAIN launch leaves its finaliser to the Krum chain's
    gathered fold: the models are bitwise the undeferred run's, the test metrics fs_eval's to the 1e-12
    relative the header states for a fused deferral."""
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
            fed = tools.Federation('fedkrum', Xs, ys, Xt, yt, None, 'classification', C, D, 0.5, 1, 32, False, 0.0,
                                   False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False,
                                   options={'defer_eval': defer}, krum=dict(f=0.2, m=None))
            for _ in range(R):
                fed.round()
            fed.results()
            assert fed.plan.eval_blocks() > 0
            runs[defer] = (stats['W_rounds'], fed.eval_hist.cpu().numpy().copy(), stats['krum_selected'])
    assert np.array_equal(runs[False][0], runs[True][0]) and np.isfinite(runs[True][0]).all()
    assert np.isfinite(runs[True][1]).all()
    np.testing.assert_allclose(runs[True][1], runs[False][1], rtol=1e-12, atol=0)
    assert all(len(s) == 8 for s in runs[True][2])

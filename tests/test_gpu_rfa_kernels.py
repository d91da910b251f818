"""fs_rfa_step, fs_rfa_weights and fs_aggregate_rfa at kernel level: bitwise tests/rfa_restatement.py (NaN
as NaN).

M in {1, 2, 3, 5, 8, 9, 63, 64, 65, 257, 1250}, the first M of each narrower stripe (1262: 16 columns, 2524:
8 columns) and fs_aggregate_rfa_max_m() = 5047; M = max_m + 1 is an error without a launch.  len in {4, 32,
36, 132}: one float4 lane, one full 32-column stripe, a ragged last stripe, several stripes.  Contiguous rows
and the same rows gathered from a buffer of twice as many, NaN in the rows outside the sample."""
import numpy as np
import pytest
import torch

from tests import rfa_restatement as RR

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MS = (1, 2, 3, 5, 8, 9, 63, 64, 65, 257, 1250, RR.MAX_M32 + 1, RR.MAX_M16 + 1, RR.MAX_M)
LENS = (4, 32, 36, 132)


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


def gather(W, seed=9):
    """The same rows in the same order, scattered over a buffer of twice as many rows, NaN elsewhere."""
    M, L = W.shape
    sel = np.sort(np.random.RandomState(seed + M).permutation(2 * M)[:M]).astype(np.int32)
    big = np.full((2 * M, L), np.nan, F32)
    big[sel] = W
    return big, sel


def same(got, ref, what):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    ok = (got.view(u) == ref.view(u)) | (np.isnan(got) & np.isnan(ref))
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, (what, len(bad), got[bad[:4]], ref[bad[:4]], bad[:4])


def dv(amd, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(amd.dev)


def some_b(M, seed=0, zeros=True):
    """Weights as a step would get them: positive floats that sum to about 1, some of them 0."""
    rs = np.random.RandomState(5 * M + seed)
    b = rs.dirichlet(np.full(M, 2.0)).astype(F32)
    if zeros and M > 2:
        b[rs.permutation(M)[:max(1, M // 5)]] = 0
    return b


def step(amd, W, v, b=None, flag=0, sel=None, calls=1, alias=False):
    """``calls`` launches of fs_rfa_step (sel: gathered); [(v', part)] as numpy."""
    M = W.shape[0] if sel is None else len(sel)
    L = W.shape[1]
    Wd, sd, bd = dv(amd, W), dv(amd, sel), dv(amd, b)
    fd = None if b is None else torch.tensor([flag], dtype=torch.int32, device=amd.dev)
    S = RR.stripes(M, L)
    res = []
    for _ in range(calls):
        vd = dv(amd, v)
        vo = vd if alias else torch.full((L,), 7.0, device=amd.dev)
        part = torch.full((S, M), -1.0, dtype=torch.float64, device=amd.dev)
        amd.engine.rfa_step(Wd, L, vd, bd, fd, vo, part, sel=sd, M=M)
        res.append((vo.cpu().numpy().copy(), part.cpu().numpy().copy()))
    return res


def weights(amd, part, d2, M, L, alpha, nu, mean=False):
    """fs_rfa_weights: (d2, dist, b, obj, flag) as numpy."""
    dev = amd.dev
    d2d = torch.full((M,), -1.0, dtype=torch.float64, device=dev) if d2 is None else dv(amd, d2)
    dist = torch.full((M,), -1.0, dtype=torch.float64, device=dev)
    b = torch.full((M,), -1.0, device=dev)
    obj = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
    flag = torch.full((1,), -1, dtype=torch.int32, device=dev)
    amd.engine.rfa_weights(dv(amd, part), M, L, dv(amd, alpha), nu, d2d, dist, b, obj, flag, mean=mean)
    return d2d.cpu().numpy(), dist.cpu().numpy(), b.cpu().numpy(), float(obj.item()), int(flag.item())


def chain(amd, W, x, alpha, T, nu, init, sel=None, alias=False, calls=1):
    """fs_aggregate_rfa through Aggregator.run_rfa: [dict(out, dist, b, obj)]."""
    dev = amd.dev
    M = W.shape[0] if sel is None else len(sel)
    L = W.shape[1]
    agg = amd.engine.Aggregator(M, 1, L, dev)
    Wd, sd, ad = dv(amd, W), dv(amd, sel), dv(amd, alpha)
    ws = agg.rfa_ws()
    assert ws.numel() == RR.ws_bytes(M, L)
    res = []
    for _ in range(calls):
        xd = dv(amd, x)
        out = xd if alias else torch.full((L,), 7.0, device=dev)
        dist = torch.full((M,), -1.0, dtype=torch.float64, device=dev)
        b = torch.full((M,), -1.0, device=dev)
        obj = torch.full((T + 2,), -1.0, dtype=torch.float64, device=dev)
        ws.fill_(0xA5)
        agg.run_rfa(Wd, xd, ad, T, nu, init, out, dist, b, obj, ws, sel=sd)
        res.append(dict(out=out.cpu().numpy().copy(), dist=dist.cpu().numpy(), b=b.cpu().numpy(),
                        obj=obj.cpu().numpy()))
    return res


def check_chain(got, ref, what):
    for key in ('out', 'dist', 'b', 'obj'):
        same(got[key], ref[key], what + (key,))


def test_max_m_and_widths(amd):
    assert amd.engine.rfa_max_m() == RR.MAX_M >= 5047 and amd.engine.rfa_max_m() >= amd.engine.robust_max_m()
    for M in MS:
        assert amd.engine.rfa_width(M) == RR.width(M)
        assert amd.engine.rfa_ws_bytes(M, 132) == RR.ws_bytes(M, 132)


@pytest.mark.parametrize('M', MS)
def test_step_bitwise_the_restatement(amd, M):
    """Pass 0 and a fold with given weights at every len, contiguous and gathered, twice: v' and the partial
    table are the restatement's bits, so is the reduced d2; the same bits on the second call and from the
    larger buffer."""
    for L in LENS:
        W, x, alpha = RR.inputs('normal', M, L)
        big, sel = gather(W)
        for b in (None, some_b(M, L)):
            rv, rp = RR.step(W, x, b)
            assert np.isfinite(rv).all() and np.isfinite(rp).all()
            (v1, p1), (v2, p2) = step(amd, W, x, b, calls=2)
            same(v1, rv, (M, L, b is None, 'v'))
            same(p1, rp, (M, L, b is None, 'part'))
            same(v2, v1, (M, L, 'second call v'))
            same(p2, p1, (M, L, 'second call part'))
            vg, pg = step(amd, big, x, b, sel=sel)[0]
            same(vg, rv, (M, L, 'gathered v'))
            same(pg, rp, (M, L, 'gathered part'))
            d2 = weights(amd, p1, None, M, L, alpha, 1e-6)[0]
            same(d2, RR.reduce_d2(rp), (M, L, 'd2'))
        # v_out may be v
        va, pa = step(amd, W, x, some_b(M, L), alias=True)[0]
        same(va, RR.step(W, x, some_b(M, L))[0], (M, L, 'alias'))


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('kind', ['equal', 'zeros', 'mixed'])
def test_step_kinds(amd, M, kind):
    """All-equal rows (every distance 0), +-0 only, magnitudes from 1e-30 to 1e30 -- and one float difference
    that overflows (3e38 - -3e38: a +Inf partial for that row, as the restatement's)."""
    W, x, _ = RR.inputs(kind, M, 36)
    if kind == 'mixed':
        W[M // 2, 33], x[33] = F32(3e38), F32(-3e38)
    for b in (None, some_b(M, 1)):
        rv, rp = RR.step(W, x, b)
        v, p = step(amd, W, x, b)[0]
        same(v, rv, (M, kind, b is None, 'v'))
        same(p, rp, (M, kind, b is None, 'part'))
        if kind == 'equal' and b is None:
            assert (p == 0).all()


@pytest.mark.parametrize('M', [2, 5, 9, 65, 257, 1250, RR.MAX_M16 + 1])
def test_rows_at_weight_zero_are_never_multiplied(amd, M):
    """Rows of NaN and of +-Inf at b_k = 0, gathered: v' is finite and the restatement's bits, their partial
    distances are not finite; with the flag set v' is v bit for bit."""
    rs = np.random.RandomState(M)
    W, x, _ = RR.inputs('normal', M, 132)
    b = some_b(M, 2, zeros=False)
    bad = rs.permutation(M)[:max(1, M // 3)]
    W[bad] = np.where(rs.randint(0, 3, size=(len(bad), 132)) == 0, np.nan,
                      np.where(rs.randint(0, 2, size=(len(bad), 132)) == 0, np.inf, -np.inf)).astype(F32)
    b[bad] = 0
    big, sel = gather(W)
    rv, rp = RR.step(W, x, b)
    v, p = step(amd, big, x, b, sel=sel)[0]
    same(v, rv, (M, 'v'))
    same(p, rp, (M, 'part'))
    assert np.isfinite(v).all() and not np.isfinite(p[:, bad]).any()
    assert np.isfinite(np.delete(p, bad, 1)).all()
    v, p = step(amd, W, x, b, flag=1)[0]
    assert v.tobytes() == x.tobytes()
    same(p, RR.partials(W, x), (M, 'flag part'))


@pytest.mark.parametrize('M', MS)
def test_weights_bitwise_the_restatement(amd, M):
    """fs_rfa_weights from a given d2: zeros, tiny, ordinary and huge values, +Inf and NaN entries; both
    weight rules; nu below, among and above the distances; alpha with zeros.  Also: nothing finite."""
    rs = np.random.RandomState(11 * M)
    d2 = (rs.rand(M) * 10.0 ** rs.uniform(-20, 20, size=M)).astype(F64)
    d2[rs.permutation(M)[:M // 4]] = rs.rand(M // 4)
    if M >= 5:
        d2[rs.permutation(M)[:3]] = [0.0, np.inf, np.nan]
    alpha = rs.dirichlet(np.full(M, 5.0)).astype(F32)
    if M >= 8:
        alpha[rs.permutation(M)[:2]] = 0
    for nu in (1e-6, 0.5, 1e12):
        for mean in (False, True):
            rd, rb, ro, rf = RR.weights(d2, alpha, nu, mean)
            g2, gd, gb, go, gf = weights(amd, None, d2, M, 36, alpha, nu, mean)
            same(g2, d2, (M, nu, mean, 'd2 untouched'))
            same(gd, rd, (M, nu, mean, 'dist'))
            same(gb, rb, (M, nu, mean, 'b'))
            same(np.array([go]), np.array([ro]), (M, nu, mean, 'obj'))
            assert gf == rf == 0
    bad = np.where(rs.rand(M) < 0.5, np.inf, np.nan)
    _, gd, gb, go, gf = weights(amd, None, bad, M, 36, alpha, 1e-6)
    assert gf == 1 and (gb == 0).all() and np.isnan(go) and RR.weights(bad, alpha, 1e-6)[3] == 1
    _, gd, gb, go, gf = weights(amd, None, d2, M, 36, np.zeros(M, F32), 1e-6)
    assert gf == 1 and (gb == 0).all() and RR.weights(d2, np.zeros(M, F32), 1e-6)[3] == 1


@pytest.mark.parametrize('M', MS)
def test_chain_bitwise_the_restatement(amd, M):
    """fs_aggregate_rfa for T in {0, 1, 3} and both inits at every len: d_out, d_dist, d_b and d_obj are the
    restatement's bits, contiguous (d_out = d_x), gathered, and on a second call."""
    for L in LENS:
        W, x, alpha = RR.inputs('normal', M, L)
        big, sel = gather(W)
        for init in RR.INITS:
            for T in (0, 1, 3):
                ref = RR.chain(W, x, alpha, T, 1e-6, init)
                r1, r2 = chain(amd, W, x, alpha, T, 1e-6, init, alias=True, calls=2)
                check_chain(r1, ref, (M, L, init, T, 'aliased'))
                check_chain(r2, r1, (M, L, init, T, 'second call'))
                check_chain(chain(amd, big, x, alpha, T, 1e-6, init, sel=sel)[0], ref, (M, L, init, T, 'gathered'))


@pytest.mark.parametrize('attack', RR.ATTACKS)
@pytest.mark.parametrize('case', RR.ATTACK_CASES)
def test_chain_under_attack(amd, case, attack):
    """The CPU tests' corrupted inputs through the device chain: the restatement's bits, non-finite rows at
    weight 0; every row NaN returns x bit for bit with a NaN objective."""
    M, L, bad = case
    W, x, alpha, ids = RR.attacked(M, L, bad, attack)
    for init in RR.INITS:
        ref = RR.chain(W, x, alpha, 3, 1e-6, init)
        got = chain(amd, W, x, alpha, 3, 1e-6, init)[0]
        check_chain(got, ref, (case, attack, init))
        if attack in ('nan', 'inf'):
            assert (got['b'][ids] == 0).all() and np.isfinite(got['out']).all()
    got = chain(amd, np.full_like(W, np.nan), x, alpha, 2, 1e-6, 'mean')[0]
    assert got['out'].tobytes() == x.tobytes() and np.isnan(got['obj']).all() and (got['b'] == 0).all()
    got = chain(amd, W, x, alpha, 2, 1e6, 'start')[0]                # nu above every finite distance
    check_chain(got, RR.chain(W, x, alpha, 2, 1e6, 'start'), (case, attack, 'large nu'))


def test_output_may_be_a_slice_of_a_larger_buffer(amd):
    M, L = 65, 132
    W, x, alpha = RR.inputs('normal', M, L)
    agg = amd.engine.Aggregator(M, 1, L, amd.dev)
    buf = torch.full((L + 8,), 3.0, device=amd.dev)
    dist, b = torch.zeros(M, dtype=torch.float64, device=amd.dev), torch.zeros(M, device=amd.dev)
    obj = torch.zeros(5, dtype=torch.float64, device=amd.dev)
    agg.run_rfa(dv(amd, W), dv(amd, x), dv(amd, alpha), 3, 1e-6, 'start', buf[:L], dist, b, obj, agg.rfa_ws())
    same(buf[:L].cpu().numpy(), RR.chain(W, x, alpha, 3)['out'], 'out')
    assert bool((buf[L:] == 3.0).all())


def test_errors_return_without_a_launch(amd):
    dev = amd.dev
    L = amd.lib.lib()
    p, st = amd.lib.ptr, amd.lib.stream_ptr()
    W = torch.zeros(4, 8, device=dev)
    x, al = torch.zeros(8, device=dev), torch.full((4,), 0.25, device=dev)
    out = torch.full((8,), 5.0, device=dev)
    dist, b = torch.full((4,), 5.0, dtype=torch.float64, device=dev), torch.full((4,), 5.0, device=dev)
    obj = torch.full((5,), 5.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(RR.ws_bytes(4, 8), dtype=torch.uint8, device=dev)

    def call(M=4, ln=8, stride=8, T=3, nu=1e-6, init=0, nws=ws.numel()):
        return L.fs_aggregate_rfa(p(W), stride, None, M, ln, p(x), p(al), T, nu, init, p(out), p(dist), p(b), p(obj),
                                  p(ws), nws, st)

    for kw in (dict(M=0), dict(M=RR.MAX_M + 1), dict(T=-1), dict(T=33), dict(nu=0.0), dict(nu=float('nan')),
               dict(init=2), dict(ln=6), dict(stride=6), dict(ln=8, stride=4), dict(nws=ws.numel() - 1)):
        assert call(**kw) == -1, kw
    agg = amd.engine.Aggregator(RR.MAX_M + 1, 1, 4, dev)
    with pytest.raises(ValueError, match='max_m'):
        agg.run_rfa(torch.zeros(RR.MAX_M + 1, 4, device=dev), torch.zeros(4, device=dev),
                    torch.zeros(RR.MAX_M + 1, device=dev), 3, 1e-6, 'start', torch.zeros(4, device=dev),
                    torch.zeros(RR.MAX_M + 1, dtype=torch.float64, device=dev), torch.zeros(RR.MAX_M + 1, device=dev),
                    torch.zeros(5, dtype=torch.float64, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev))
    with pytest.raises(amd.lib.FedsimError, match=r'T must be in \[0, 32\]'):
        amd.engine.Aggregator(4, 1, 8, dev).run_rfa(W, x, al, 33, 1e-6, 'start', out, dist, b,
                                                    torch.zeros(40, dtype=torch.float64, device=dev), ws)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((dist == 5.0).all()) and bool((b == 5.0).all()) and bool((obj == 5.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


def test_finaliser_rides_and_gives_fs_evals_numbers(amd):
    """A deferred evaluation fused into the next TRAIN launch leaves its finaliser to the extra last workgroup
    of the chain's last step: the models are bitwise the undeferred run's, the test metrics fs_eval's to the
    1e-12 relative the header states for a fused deferral."""
    from fedamw_amd.functions import tools
    tune = dict(train_form=1, split_mb=-1, split_dbuf=-1, split_pipe=-1, split_teams=-1)
    C, Nc, R, D, n_t = 10, 10, 3, 1024, 16 * 16 + 5
    rs = np.random.RandomState(17)
    sizes = rs.randint(8, 41, size=Nc)
    Xs = [torch.from_numpy((np.cos(rs.normal(size=(n, D))) / np.sqrt(D)).astype(F32)) for n in sizes]
    ys = [torch.from_numpy(rs.randint(0, C, size=n).astype(np.int64)) for n in sizes]
    Xt = torch.from_numpy((np.cos(rs.normal(size=(n_t, D))) / np.sqrt(D)).astype(F32))
    yt = torch.from_numpy(rs.randint(0, C, size=n_t).astype(np.int64))
    for iters in (0, 2):
        runs = {}
        with amd.lib.tuning(**tune):
            for defer in (False, True):
                stats = {'trace': True}
                torch.manual_seed(11)
                fed = tools.Federation('fedrfa', Xs, ys, Xt, yt, None, 'classification', C, D, 0.5, 1, 32, False, 0.0,
                                       False, 0.0, R, 1e-3, 'parallel', stats=stats, verbose=False,
                                       options={'defer_eval': defer}, rfa=dict(iters=iters))
                for _ in range(R):
                    fed.round()
                fed.results()
                assert fed.plan.eval_blocks() > 0
                runs[defer] = (stats['W_rounds'], fed.eval_hist.cpu().numpy().copy())
        assert np.array_equal(runs[False][0], runs[True][0]) and np.isfinite(runs[True][0]).all()
        assert np.isfinite(runs[True][1]).all()
        np.testing.assert_allclose(runs[True][1], runs[False][1], rtol=1e-12, atol=0)

"""fs_dp_norms, fs_dp_coef, fs_dp_noise and fs_aggregate_dp at kernel level against tests/dp_restatement.py.

M in {1, 2, 3, 15, 16, 17, 65, 513, 1250}: both sides of the exact-fold bound (16) and of AG_ONE_MAX_N (512).
len in {4, 36, 132, 1028}, and 1020, 1024, 1028 -- one float4 per thread of a 256-thread workgroup and its two
neighbours -- at M in {1, 3, 17}.  Contiguous rows, and the same rows gathered from a buffer of twice as many with
NaN elsewhere.  The checks are layered: the norms against float64 within the bound csrc/aggregate_dp.hip derives
(10 float roundings), then every later stage bit for bit given the previous stage's device output."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dp_restatement as DP

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MS = (1, 2, 3, 15, 16, 17, 65, 513, 1250)
LENS = (4, 36, 132, 1028)
SHAPES = [(M, L) for M in MS for L in LENS] + [(M, L) for M in (1, 3, 17) for L in (1020, 1024)]
ROUNDINGS = 10                # csrc/aggregate_dp.hip's header: float roundings on a square's path
CLIP = 1.0
SEED, ROUND = 2 ** 32 + 5, 3
ADAPTIVE = dict(quantile=0.6, lr=0.3, count_noise=1.5)


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


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


def ulps(a, b):
    return abs(int(np.array(a, F64).view(np.int64)) - int(np.array(b, F64).view(np.int64)))


def dv(amd, a):
    return None if a is None else torch.from_numpy(np.array(a, order='C')).to(amd.dev)      # (a copy: the inputs are read-only)


@functools.lru_cache(maxsize=None)
def inputs(M, L):
    """(W [M, L], x [L], q [M]); read-only, shared by the tests.  Every update's norm is a factor 2 or more away
    from CLIP: radii in [0.05, 0.45] (even k) or [2.2, 6] (odd k), so no clip decision rests on a rounding."""
    rs = np.random.RandomState(1000 * M + L)
    x = rs.standard_normal(L).astype(F32)
    q = rs.dirichlet(np.full(M, 2.0)).astype(F32)
    u = rs.standard_normal((M, L))
    u /= np.sqrt((u * u).sum(axis=1, keepdims=True))
    rad = np.where(np.arange(M) % 2 == 0, rs.uniform(0.05, 0.45, M), rs.uniform(2.2, 6.0, M))
    W = (x[None, :].astype(F64) + rad[:, None] * u).astype(F32)
    for a in (W, x, q):
        a.setflags(write=False)
    return W, x, q


def gather(W, seed=9):
    """The same rows in the same order scattered over a buffer of twice as many rows, NaN in the others."""
    M, L = W.shape
    sel = np.sort(np.random.RandomState(seed + M).permutation(2 * M)[:M]).astype(np.int32)
    big = np.full((2 * M, L), np.nan, F32)
    big[sel] = W
    return big, sel


def dev_norms(amd, W, x, sel=None, M=None):
    M = (W.shape[0] if sel is None else len(sel)) if M is None else M
    agg = amd.engine.Aggregator(M, 1, W.shape[1], amd.dev)
    n = torch.full((M,), -1.0, dtype=torch.float64, device=amd.dev)
    agg.dp_norms(dv(amd, W), dv(amd, x), n, sel=dv(amd, sel), M=M)
    return n.cpu().numpy()


def dev_coef(amd, n, q, S, z, seed=0, t=0, adaptive=None):
    M = len(n)
    agg = amd.engine.Aggregator(M, 1, 4, amd.dev)
    c = torch.full((M,), -1.0, device=amd.dev)
    r = torch.full((M,), -1.0, dtype=torch.float64, device=amd.dev)
    st = torch.full((amd.engine.DP_STATE,), -1.0, dtype=torch.float64, device=amd.dev)
    clip = torch.full((1,), float(S), dtype=torch.float64, device=amd.dev) if adaptive is not None else None
    agg.dp_coef(dv(amd, np.asarray(n, F64)), dv(amd, q), S, z, c, r, st, seed=seed, t=t, adaptive=adaptive,
                clip_dev=clip)
    return c.cpu().numpy(), r.cpu().numpy(), st.cpu().numpy(), None if clip is None else float(clip.cpu()[0])


def dev_noise(amd, seed, t, L, stream=0):
    g = torch.full((L,), 99.0, device=amd.dev)
    amd.engine.Aggregator(1, 1, 4, amd.dev).dp_noise(seed, t, g, stream=stream)
    return g.cpu().numpy()


def run(amd, W, x, q, S, z, sel=None, chunks=0, seed=SEED, t=ROUND, adaptive=None, cols=None):
    """One fs_aggregate_dp call; dict(out, c, r, state, clip) as numpy, and the partials the workspace holds."""
    M = W.shape[0] if sel is None else len(sel)
    L = W.shape[1]
    agg = amd.engine.Aggregator(M, 1, L, amd.dev, chunks=chunks)
    Wd, xd = dv(amd, W), dv(amd, x)
    c = torch.full((M,), -1.0, device=amd.dev)
    r = torch.full((M,), -1.0, dtype=torch.float64, device=amd.dev)
    st = torch.full((amd.engine.DP_STATE,), -1.0, dtype=torch.float64, device=amd.dev)
    clip = torch.full((1,), float(S), dtype=torch.float64, device=amd.dev) if adaptive is not None else None
    agg.ws.fill_(float('nan'))
    agg.run_dp(Wd, dv(amd, q), S, z, xd, c, r, st, seed=seed, t=t, adaptive=adaptive, clip_dev=clip, sel=dv(amd, sel),
               M=M, cols=cols)
    same(Wd.cpu().numpy(), W, 'W_all is not written')
    return dict(out=xd.cpu().numpy(), c=c.cpu().numpy(), r=r.cpu().numpy(), state=st.cpu().numpy(),
                clip=None if clip is None else float(clip.cpu()[0])), agg.ws.numel() // L


def check_coef(got_c, got_r, got_state, n, q, S, z, seed, t, adaptive, what, got_clip=None):
    """c, r, b, dropped, sigma and the clip bit for bit the restatement on the device's own norms; S_next to 4 ulp
    (the device's and numpy's exp are each specified to 1 ulp; the margin is x 2)."""
    c, r, st = DP.coef(n, q, S, z, seed, t, adaptive)
    same(got_c, c, (what, 'c'))
    same(got_r, r, (what, 'r'))
    ref = DP.state_vector(st)
    same(got_state[:4], ref[:4], (what, 'clip, sigma, b, dropped'))
    assert ulps(got_state[4], ref[4]) <= 4, (what, 'clip_next', got_state[4], ref[4])
    if adaptive is None:
        assert got_state[4] == S
    else:
        assert got_clip == got_state[4] and got_clip != S, (what, got_clip)
    return st


# ---- the norm pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,L', SHAPES)
def test_norms_against_float64(amd, M, L):
    W, x, _ = inputs(M, L)
    exact = DP.norms_exact(W, x)
    n = dev_norms(amd, W, x)
    err = np.abs(n - exact) / exact
    print('norms %d x %d: max relative error %.3g of the bound %.3g' % (M, L, err.max(), ROUNDINGS * 2.0 ** -24))
    assert (err <= ROUNDINGS * 2.0 ** -24).all(), (M, L, err.max())
    same(dev_norms(amd, W, x), n, (M, L, 'second call'))
    big, sel = gather(W)
    same(dev_norms(amd, big, x, sel=sel), n, (M, L, 'gathered'))


def test_norms_of_nonfinite_rows(amd):
    M, L = 9, 132
    W, x, _ = inputs(M, L)
    W = W.copy()
    W[1, 5], W[3, 0], W[4, 131], W[6, 77] = np.nan, np.inf, -np.inf, F32(3e38)
    W[7] = x + F32(1e20)                             # finite values whose squares overflow float
    n = dev_norms(amd, W, x)
    assert not np.isfinite(n[[1, 3, 4, 6, 7]]).any() and np.isfinite(n[[0, 2, 5, 8]]).all()
    ref = DP.norms(W, x)
    assert np.array_equal(np.isfinite(n), np.isfinite(ref))


# ---- the coefficients ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,L', [(M, 132) for M in MS] + [(3, 4), (17, 1028)])
def test_coefficients_bitwise_on_the_device_norms(amd, M, L):
    W, x, q = inputs(M, L)
    r64 = np.sqrt(DP.norms_exact(W, x))
    assert ((r64 <= CLIP / 2) | (r64 >= 2 * CLIP)).all()          # no clip decision rests on a rounding
    n = dev_norms(amd, W, x)
    for qq in (q, None):
        for z, adaptive in ((0.0, None), (1.3, None), (0.7, ADAPTIVE), (0.0, dict(quantile=0.3, lr=0.2))):
            c, r, st, clip = dev_coef(amd, n, qq, CLIP, z, SEED, ROUND, adaptive)
            ref = check_coef(c, r, st, n, qq, CLIP, z, SEED, ROUND, adaptive, (M, L, qq is None, z, adaptive), clip)
            assert ref['b'] == (M + 1) // 2 and ref['dropped'] == 0
            assert (st[1] == 0.0) == (z == 0.0)
    # no clipping at all: c is q
    c, _, st, _ = dev_coef(amd, n, q, float('inf'), 0.0)
    same(c, q, (M, L, 'S = inf'))
    assert st[0] == np.inf and st[2] == M


def test_coefficients_at_special_norms(amd):
    S = 1.5
    n = np.array([0.0, S * S, np.inf, np.nan, 4 * S * S, np.nextafter(S * S, 0.0), 1e300, 5e-324], F64)
    assert np.sqrt(n[1]) == S
    q = np.array([0.3, 0.1, 0.2, 0.05, 0.15, 0.05, 0.1, 0.05], F32)
    for z, adaptive in ((0.0, None), (2.0, None), (1.0, ADAPTIVE)):
        c, r, st, clip = dev_coef(amd, n, q, S, z, 1, 0, adaptive)
        ref = check_coef(c, r, st, n, q, S, z, 1, 0, adaptive, ('special', z), clip)
        assert ref['dropped'] == 2 and ref['b'] == 4 and c[2] == 0 and c[3] == 0 and c[0] == q[0] and c[1] == q[1]
        assert np.isinf(r[2]) and np.isnan(r[3]) and r[0] == 0 and r[1] == S


# ---- the noise field ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [4, 36, 1028, 4100, 28672])
def test_noise_field(amd, L):
    fields = {}
    for t in (0, 1, 2 ** 31 - 1):
        for seed in (0, 1, 2 ** 32 + 5):
            g = dev_noise(amd, seed, t, L)
            ref = DP.noise(seed, t, L)
            differ = bits(g) != bits(ref)
            near = (g == np.nextafter(ref, F32(np.inf))) | (g == np.nextafter(ref, F32(-np.inf)))
            assert (~differ | near).all(), (L, t, seed, g[differ & ~near][:4], ref[differ & ~near][:4])
            print('noise len %d t %d seed %d: %d of %d values are the neighbouring float' % (L, t, seed, differ.sum(), L))
            assert differ.sum() <= 1e-3 * L, (L, t, seed, int(differ.sum()))
            assert np.abs(g).max() <= 6.77
            same(dev_noise(amd, seed, t, L), g, (L, t, seed, 'second call'))
            fields[(t, seed)] = g
    keys = list(fields)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(bits(fields[a]), bits(fields[b])), (L, a, b)
    s1 = dev_noise(amd, 1, 1, L, stream=1)
    assert not np.array_equal(bits(s1), bits(fields[(1, 1)]))
    ref1 = DP.noise(1, 1, L, stream=1)
    assert (np.abs(s1.astype(F64) - ref1) <= np.spacing(np.abs(ref1))).all()


# ---- the aggregate ------------------------------------------------------------------------------------------
def layered(amd, W, x, q, S, z, got, wsp, chunks=0, adaptive=None, cols=None, what=None):
    """The restatement fed the device's n, c and g: every stage bit for bit given the one before."""
    n = dev_norms(amd, W, x)
    check_coef(got['c'], got['r'], got['state'], n, q, S, z, SEED, ROUND, adaptive, what, got['clip'])
    g = dev_noise(amd, SEED, ROUND, W.shape[1]) if z else None
    ref = DP.aggregate(W, x, q, S, z, SEED, ROUND, adaptive, chunks, wsp, n=n, c=got['c'], g=g, cols=cols)
    # (sigma as the device left it: bitwise the restatement's, checked above)
    same(got['out'], ref['out'], (what, 'out'))
    return ref


@pytest.mark.parametrize('M,L', SHAPES)
def test_aggregate_bitwise_contiguous_and_gathered(amd, M, L):
    W, x, q = inputs(M, L)
    big, sel = gather(W)
    for qq, z in ((q, 1.3), (None, 0.0)):
        got, wsp = run(amd, W, x, qq, CLIP, z)
        layered(amd, W, x, qq, CLIP, z, got, wsp, what=(M, L, z))
        gat, _ = run(amd, big, x, qq, CLIP, z, sel=sel)
        for key in ('out', 'c', 'r', 'state'):
            same(gat[key], got[key], (M, L, z, 'gathered', key))
        again, _ = run(amd, W, x, qq, CLIP, z)
        same(again['out'], got['out'], (M, L, z, 'second call'))
    assert not np.array_equal(got['out'], x)


@pytest.mark.parametrize('chunks', [0, 1, 3, 8])
@pytest.mark.parametrize('M', [2, 17, 65, 513, 1250])
def test_forced_chunks(amd, M, chunks):
    L = 132
    W, x, q = inputs(M, L)
    big, sel = gather(W)
    got, wsp = run(amd, W, x, q, CLIP, 0.9, chunks=chunks, adaptive=ADAPTIVE)
    layered(amd, W, x, q, CLIP, 0.9, got, wsp, chunks=chunks, adaptive=ADAPTIVE, what=(M, chunks))
    gat, _ = run(amd, big, x, q, CLIP, 0.9, sel=sel, chunks=chunks, adaptive=ADAPTIVE)
    same(gat['out'], got['out'], (M, chunks, 'gathered'))


@pytest.mark.parametrize('chunks', [0, 1, 4])
@pytest.mark.parametrize('M', [1, 3, 15, 16, 17, 65, 513, 1250])
def test_identity_against_fs_aggregate_opt(amd, M, chunks):
    """S = +Inf, z = 0, q > 0 is fs_aggregate_opt's AVGM step at beta1 = 0, eta = 1 bit for bit."""
    L = 132
    W, x, q = inputs(M, L)
    assert (q > 0).all()
    agg = amd.engine.Aggregator(M, 1, L, amd.dev, chunks=chunks)
    xd, md = dv(amd, x), torch.zeros(L, device=amd.dev)
    agg.run_opt(dv(amd, W), dv(amd, q), 'avgm', xd, md, None, eta=1.0, beta1=0.0)
    got, _ = run(amd, W, x, q, float('inf'), 0.0, chunks=chunks)
    same(got['out'], xd.cpu().numpy(), (M, chunks, 'opt'))
    same(got['c'], q, (M, chunks, 'c'))
    assert got['state'][2] == M and got['state'][3] == 0 and got['state'][1] == 0


@pytest.mark.parametrize('M,L', [(3, 36), (9, 132), (17, 1028), (65, 132), (513, 36)])
def test_nonfinite_rows_are_dropped_and_counted(amd, M, L):
    W, x, q = inputs(M, L)
    W = W.copy()
    bad = sorted({1, M // 2, M - 1} - {0})
    vals = [np.nan, np.inf, F32(3e38)]
    for j, k in enumerate(bad):
        W[k, (7 * k) % L] = vals[j % 3]
    if M >= 9:
        W[4] = x - F32(1e20)                          # finite, the squares overflow
        W[6, 3], W[6, 5] = -np.inf, np.nan
        bad = sorted(set(bad) | {4, 6})
    keep = [k for k in range(M) if k not in bad]
    for z in (0.0, 1.1):
        got, wsp = run(amd, W, x, q, CLIP, z)
        ref = layered(amd, W, x, q, CLIP, z, got, wsp, what=(M, L, z))
        assert got['state'][3] == len(bad) and (got['c'][bad] == 0).all() and (got['c'][keep] != 0).all()
        assert np.isfinite(got['out']).all()
        if M < 16 and z == 0.0:
            # the left-fold regime: the restatement over the other rows alone, the same bits
            c = got['c'][keep]
            same(got['out'], DP.finish(x, DP.fold(W[keep], x, c), 0.0, None, 0.0), (M, L, 'the others alone'))
        assert ref['state']['dropped'] == len(bad)
    # an all-dropped round leaves x + noise
    Wn = np.full((M, L), np.nan, F32)
    got, _ = run(amd, Wn, x, None, CLIP, 2.0)
    sigma = (2.0 * CLIP) * float(F32(1.0 / M))
    assert got['state'][3] == M and got['state'][2] == 0 and got['state'][1] == sigma
    g = dev_noise(amd, SEED, ROUND, L)
    same(got['out'], ((x + np.zeros(L, F32)).astype(F32) + (F32(sigma) * g).astype(F32)).astype(F32), (M, L, 'all dropped'))


def test_padding_columns_take_no_noise(amd):
    M, C, ld, D = 5, 3, 64, 50
    L = C * ld
    W, x, q = inputs(M, L)
    mask = (np.arange(L) % ld) < D
    x = np.where(mask, x, F32(0)).astype(F32)
    W = np.where(mask[None, :], W, F32(0)).astype(F32)
    got, wsp = run(amd, W, x, q, CLIP, 1.5, cols=(ld, D))
    layered(amd, W, x, q, CLIP, 1.5, got, wsp, cols=(ld, D), what='padded')
    assert (got['out'][~mask] == 0).all() and (got['out'][mask] != x[mask]).all()


def test_workspace_size_is_exported(amd):
    assert amd.engine.dp_ws_bytes(100, 4096) == 100 * 8 + 16 * 100 * 4
    assert amd.engine.dp_ws_bytes(1250, 28672) == 1250 * 8 + 112 * 1250 * 4
    assert amd.engine.dp_ws_bytes(0, 4096) == 0


def test_einval_leaves_every_output_unchanged(amd):
    """Every FS_EINVAL case returns before any launch: sentinel-filled outputs keep their bits."""
    lib = amd.lib.lib()
    M, L, stride = 5, 36, 40
    dev = amd.dev
    W = torch.randn(M, stride, device=dev)
    q = torch.full((M,), 0.2, device=dev)
    sel = torch.arange(M, dtype=torch.int32, device=dev)
    need = amd.engine.dp_ws_bytes(M, L)
    inf, nan = float('inf'), float('nan')

    def fresh():
        return dict(x=torch.full((L,), 3.0, device=dev), c=torch.full((M,), -1.0, device=dev),
                    r=torch.full((M,), -2.0, dtype=torch.float64, device=dev),
                    state=torch.full((5,), -3.0, dtype=torch.float64, device=dev),
                    clip=torch.full((1,), 1.0, dtype=torch.float64, device=dev),
                    n=torch.full((M,), -4.0, dtype=torch.float64, device=dev),
                    ws=torch.full((4 * L,), 9.0, device=dev), sws=torch.full((need,), 7, dtype=torch.uint8, device=dev))

    def untouched(out, what):
        torch.cuda.synchronize()
        for key, v in (('x', 3.0), ('c', -1.0), ('r', -2.0), ('state', -3.0), ('clip', 1.0), ('n', -4.0), ('ws', 9.0),
                       ('sws', 7)):
            assert bool((out[key] == v).all()), (what, key)

    def p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    good = dict(W=W, stride=stride, sel=sel, q=q, M=M, L=L, S=1.0, z=1.0, t=0, adaptive=0, gamma=0.5, eta=0.2,
                sigma_b=0.0, ws_floats=4 * L, chunks=0, sws_bytes=need, cols_ld=0, cols_d=0)
    cases = {
        'M < 1': dict(M=0),
        'S = 0': dict(S=0.0),
        'S < 0': dict(S=-1.0),
        'S NaN': dict(S=nan),
        'z < 0': dict(z=-0.5),
        'z Inf': dict(z=inf),
        'z NaN': dict(z=nan),
        'z > 0 with S = Inf': dict(S=inf),
        't < 0': dict(t=-1),
        'len no multiple of 4': dict(L=34),
        'stride no multiple of 4': dict(stride=38),
        'stride < len': dict(stride=32),
        'null W_all': dict(W=None),
        'null W_g': dict(x=None),
        'null c': dict(c=None),
        'null r': dict(r=None),
        'null state': dict(state=None),
        'null workspace': dict(sws=None),
        'workspace too small': dict(sws_bytes=need - 1),
        'adaptive without d_clip': dict(adaptive=1, clip=None),
        'adaptive quantile > 1': dict(adaptive=1, gamma=1.5),
        'adaptive lr < 0': dict(adaptive=1, eta=-0.1),
        'adaptive count noise NaN': dict(adaptive=1, sigma_b=nan),
        'adaptive with S = Inf': dict(adaptive=1, S=inf, z=0.0),
        'cols_ld does not divide len': dict(cols_ld=8, cols_d=4),
        'cols_d > cols_ld': dict(cols_ld=12, cols_d=13),
    }
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, change in cases.items():
        a = dict(good)
        out = fresh()
        bufs = dict(out)
        for k, v in change.items():
            if k in bufs:
                bufs[k] = v
            else:
                a[k] = v
        rc = lib.fs_aggregate_dp(p(a['W']), a['stride'], p(a['sel']), p(a['q']), a['M'], a['L'], a['S'], a['z'], 7,
                                 a['t'], a['adaptive'], a['gamma'], a['eta'], a['sigma_b'], p(bufs['clip']),
                                 a['cols_ld'], a['cols_d'], p(bufs['x']), p(bufs['c']), p(bufs['r']), p(bufs['state']),
                                 p(out['ws']), a['ws_floats'], a['chunks'], p(bufs['sws']), a['sws_bytes'], st)
        assert rc == -1, (name, rc)                                   # FS_EINVAL
        assert lib.fs_last_error(), name
        untouched(out, (name, 'aggregate'))
        if name in ('M < 1', 'len no multiple of 4', 'stride no multiple of 4', 'stride < len', 'null W_all', 'null W_g',
                    'null workspace', 'workspace too small'):
            rc = lib.fs_dp_norms(p(a['W']), a['stride'], p(a['sel']), a['M'], a['L'], p(bufs['x']), p(bufs['n']),
                                 p(bufs['sws']), a['sws_bytes'], st)
            assert rc == -1, (name, 'norms', rc)
            untouched(out, (name, 'norms'))
        if 'S' in name or name.startswith(('z ', 'adaptive', 'M <', 't <')) or name in ('null c', 'null r', 'null state'):
            rc = lib.fs_dp_coef(p(bufs['n']), p(a['q']), a['M'], a['S'], a['z'], 7, a['t'], a['adaptive'], a['gamma'],
                                a['eta'], a['sigma_b'], p(bufs['clip']), p(bufs['c']), p(bufs['r']), p(bufs['state']), st)
            assert rc == -1, (name, 'coef', rc)
            untouched(out, (name, 'coef'))
    out = fresh()
    for a in (dict(L=34, g=out['x']), dict(L=L, g=None), dict(L=L, g=out['x'], t=-1)):
        assert lib.fs_dp_noise(7, a.get('t', 0), 0, a['L'], p(a['g']), st) == -1
    rc = lib.fs_dp_norms(p(W), stride, p(sel), M, L, p(out['x']), None, p(out['sws']), need, st)
    assert rc == -1
    untouched(out, 'noise, null n')
    # d_sel and d_q may be NULL, d_clip unless adaptive; S = +Inf is allowed with z = 0
    rc = lib.fs_aggregate_dp(p(W), stride, None, None, M, L, inf, 0.0, 7, 0, 0, 0.0, 0.0, 0.0, None, 0, 0, p(out['x']),
                             p(out['c']), p(out['r']), p(out['state']), None, 0, 0, p(out['sws']), need, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out['c'] == np.float32(0.2)).all()) and not bool((out['x'] == 3.0).all())
    assert float(out['state'][0]) == inf and float(out['clip'][0]) == 1.0

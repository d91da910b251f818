"""fs_local_train_scaffold at kernel level: N = 5 clients (sizes include 1, one below B and one with a
short last batch), E = 2, one shape per instance (RT x CT) plus the shape whose W does not fit LDS.

Bitwise: zero variates against the parent's single form, the epilogue against its own formula in
numpy float32 from the GPU's W_out, subset launches against the full launch.  Against the
restatement (tests/scaffold_restatement.py): W within 2e-5 max|W|, losses within 1e-5 max(1, |l|)
-- the kernel-level bounds of test_gpu_mse.py and test_gpu_fednova.py (the recorded drift of
scaffold_drift.json, <= 2e-7 in W, is far below half of either)."""
import functools

import numpy as np
import pytest
import torch

from tests import scaffold_restatement as SR

pytestmark = pytest.mark.gpu

#         B   C    D    ld
SHAPES = [(5, 3, 70, 128),        # <1, 1>, D padded
          (32, 10, 256, 256),     # <2, 1>
          (64, 17, 192, 192),     # <4, 2>
          (16, 20, 64, 64),       # <1, 2>
          (32, 32, 2048, 2048)]   # <2, 2>, W (32 x 2052 floats) does not fit the LDS budget
E, LR, LAM = 2, 0.3, 0.01
W_TOL, LOSS_TOL = 2e-5, 1e-5
SENTINEL = -7.25


def sizes(B):
    return [1, B - 1, 2 * B + 3, B, max(2, B // 2)]


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine, rng
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, rng=rng, dev=torch.device('cuda')))


@functools.lru_cache(maxsize=None)
def case(B, C, D, ld):
    """Host inputs of one shape, built once and read-only: features, labels, start model, variates
    at the scale of the gradients (0.1 * normal), pass seeds."""
    rs = np.random.RandomState(B * 1000 + C)
    ns = sizes(B)
    Xs = [(np.cos(rs.normal(size=(n, D))) / np.sqrt(D)).astype(np.float32) for n in ns]
    ys = [rs.randint(0, C, size=n).astype(np.int64) for n in ns]
    W0 = (rs.normal(size=(C, D)) * 0.2).astype(np.float32)
    c = (0.1 * rs.normal(size=(C, D))).astype(np.float32)
    ci = (0.1 * rs.normal(size=(len(ns), C, D))).astype(np.float32)
    for a in Xs + ys + [W0, c, ci]:
        a.setflags(write=False)
    return dict(B=B, C=C, D=D, ld=ld, ns=ns, Xs=Xs, ys=ys, W0=W0, c=c, ci=ci, seed=B + C)


def pad(a, ld, dev, fill=0.0):
    out = torch.full(a.shape[:-1] + (ld,), fill, dtype=torch.float32, device=dev)
    out[..., :a.shape[-1]] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return out


def setup(amd, cs):
    feats = amd.engine.Features([torch.from_numpy(x) for x in cs['Xs']], [torch.from_numpy(y) for y in cs['ys']],
                                cs['D'], amd.dev, ld=cs['ld'])
    tr = amd.engine.LocalTrainer(feats, cs['C'], cs['B'], E, split=1)
    torch.manual_seed(cs['seed'])
    tr.upload_perms(amd.rng.draw_pass_seeds(tr.N * E))
    return tr


def launch(amd, cs, c=None, ci=None, reg=True, sel=None, fill=None):
    """One fs_local_train_scaffold launch -> (W_out, loss, ci) as numpy (ld wide)."""
    tr = setup(amd, cs)
    dev, ld = amd.dev, cs['ld']
    c = cs['c'] if c is None else c
    ci = cs['ci'] if ci is None else ci
    cd, cid = pad(c, ld, dev), pad(ci, ld, dev)
    if fill is not None:
        tr.W_out.fill_(fill)
        tr.loss.fill_(fill)
    tr.run_scaffold(pad(cs['W0'], ld, dev), LR, reg, LAM, cd, cid, sel=sel)
    torch.cuda.synchronize()
    assert np.array_equal(cd.cpu().numpy()[:, :cs['D']], c)           # the server variate is only read
    return tr.W_out.cpu().numpy(), tr.loss.cpu().numpy(), cid.cpu().numpy()


@functools.lru_cache(maxsize=None)
def restated(shape, reg):
    """The restatement's (W, loss, ci) of every client of a shape, computed once."""
    cs = case(*shape)
    torch.manual_seed(cs['seed'])
    out = [SR.train_client(cs['Xs'][j], cs['ys'][j], cs['W0'], LR, E, cs['B'], reg, LAM, cs['c'], cs['ci'][j])
           for j in range(len(cs['ns']))]
    return [np.stack([o[k] for o in out]) for k in range(3)]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('reg', [False, True])
def test_zero_variates_are_the_single_form(amd, shape, reg):
    cs = case(*shape)
    z = np.zeros_like(cs['c']), np.zeros_like(cs['ci'])
    W, loss, ci = launch(amd, cs, z[0], z[1], reg=reg)
    tr = setup(amd, cs)
    tr.run(pad(cs['W0'], cs['ld'], amd.dev), LR, False, 0.0, reg, LAM, False)
    torch.cuda.synchronize()
    assert amd.lib.LT_KERNELS[amd.lib.lib().fs_local_train_last_kernel()] == 'single'
    assert W.tobytes() == tr.W_out.cpu().numpy().tobytes()
    assert loss.tobytes() == tr.loss.cpu().numpy().tobytes()
    assert np.isfinite(W).all() and (loss > 0).all() and ci.any()


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('reg', [False, True])
def test_epilogue_is_its_formula_bitwise(amd, shape, reg):
    """d_ci after the launch is the float32 numpy evaluation of
    fl(fl(c_i - c) + fl(fl(x - y) * inv)), inv = 1 / fl(K_i lr), on the GPU's own W_out."""
    cs = case(*shape)
    W, _, ci = launch(amd, cs, reg=reg)
    ld, D = cs['ld'], cs['D']
    x, c, ci0 = (pad(a, ld, 'cpu').numpy() for a in (cs['W0'], cs['c'], cs['ci']))
    for j, n in enumerate(cs['ns']):
        K = E * -(-n // cs['B'])
        ref = SR.variate(ci0[j], c, x, W[j], K, LR)
        assert ci[j].tobytes() == ref.tobytes(), (j, np.abs(ci[j] - ref).max())
    assert not np.array_equal(ci[..., :D], cs['ci'])


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('reg', [False, True])
def test_nonzero_variates_against_the_restatement(amd, shape, reg):
    cs = case(*shape)
    W, loss, ci = launch(amd, cs, reg=reg)
    Wr, lr_, cir = restated(shape, reg)
    D = cs['D']
    errW = np.abs(W[..., :D] - Wr).max() / np.abs(Wr).max()
    errL = (np.abs(loss - lr_) / np.maximum(1.0, np.abs(lr_))).max()
    print('shape %s reg %d: W %.3g of %.3g, loss %.3g of %.3g' % (shape, reg, errW, W_TOL, errL, LOSS_TOL))
    assert errW <= W_TOL and errL <= LOSS_TOL
    assert (W[..., D:] == 0).all()
    # the correction moved the models: the same launch without variates is far outside the tolerance
    assert np.abs(Wr - SR_plain(shape, reg)).max() > 100 * W_TOL * np.abs(Wr).max()
    # the variate: a model difference over K lr, so the model tolerance propagates with that factor
    kmin = E * 1.0
    assert np.abs(ci[..., :D] - cir).max() <= W_TOL * np.abs(cir).max() + W_TOL * np.abs(Wr).max() / (kmin * LR)


@functools.lru_cache(maxsize=None)
def SR_plain(shape, reg):
    cs = case(*shape)
    torch.manual_seed(cs['seed'])
    z = np.zeros_like(cs['c'])
    return np.stack([SR.train_client(cs['Xs'][j], cs['ys'][j], cs['W0'], LR, E, cs['B'], reg, LAM, z, z)[0]
                     for j in range(len(cs['ns']))])


def _grad(X, y, W):
    z = X.astype(np.float64) @ W.astype(np.float64).T
    z -= z.max(axis=1, keepdims=True)
    g = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    g[np.arange(len(y)), y] -= 1.0
    return g.T @ X.astype(np.float64) / len(y)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2]])
def test_drift_cancels_on_the_gpu(amd, shape):
    """E = 1, full-batch steps (clients no larger than B), c_i = grad F_i(x), c = sum p_i c_i, float32:
    every client returns x - lr c, so all rows of W_out agree within 2e-5 max|W|."""
    B, C, D, ld = shape
    rs = np.random.RandomState(B)
    ns = [B, 1, B - 1, max(1, B // 2), B]
    Xs = [((np.cos(rs.normal(size=(n, D))) + 0.4 * i) / np.sqrt(D)).astype(np.float32) for i, n in enumerate(ns)]
    ys = [rs.randint(0, C, size=n).astype(np.int64) for n in ns]
    W0 = (rs.normal(size=(C, D)) * 0.2).astype(np.float32)
    ci = np.stack([_grad(X, y, W0) for X, y in zip(Xs, ys)])
    c = np.tensordot(SR.weights(ns), ci, 1)
    dev = amd.dev
    feats = amd.engine.Features([torch.from_numpy(x) for x in Xs], [torch.from_numpy(y) for y in ys], D, dev, ld=ld)
    tr = amd.engine.LocalTrainer(feats, C, B, 1, split=1)
    torch.manual_seed(3)
    tr.upload_perms(amd.rng.draw_pass_seeds(tr.N))
    cid = pad(ci.astype(np.float32), ld, dev)
    tr.run_scaffold(pad(W0, ld, dev), LR, False, 0.0, pad(c.astype(np.float32), ld, dev), cid)
    W = tr.W_out.cpu().numpy()[..., :D].astype(np.float64)
    ref = W0 - LR * c
    spread = np.abs(W - W[0]).max()
    print('spread %.3g, to x - lr c %.3g, bound %.3g' % (spread, np.abs(W - ref).max(), W_TOL * np.abs(ref).max()))
    assert spread <= W_TOL * np.abs(ref).max() and np.abs(W - ref).max() <= W_TOL * np.abs(ref).max()
    assert np.abs(ci - c).max() > 1e-2                      # while the clients' own gradients differ


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[1], SHAPES[4]])
def test_subset_launch(amd, shape):
    """Rows of W_out, d_ci and d_loss outside d_order keep their fill bit for bit; a sampled client's
    three results are bitwise those of the full launch -- independent of N and position."""
    cs = case(*shape)
    D = cs['D']
    Wf, lf, cif = launch(amd, cs)
    for sel in ([3], [0, 4], [1, 2, 4]):
        out = [j for j in range(len(cs['ns'])) if j not in sel]
        ci_in = cs['ci'].copy()
        ci_in[out] = np.nan                                   # never read, never written
        W, loss, ci = launch(amd, cs, ci=ci_in, sel=np.array(sel), fill=SENTINEL)
        assert W[sel].tobytes() == Wf[sel].tobytes() and loss[sel].tobytes() == lf[sel].tobytes()
        assert ci[sel].tobytes() == cif[sel].tobytes()
        assert (W[out] == SENTINEL).all() and (loss[out] == SENTINEL).all()
        assert np.isnan(ci[out][..., :D]).all() and (ci[out][..., D:] == 0).all()


def test_rejections_leave_the_outputs_untouched(amd):
    """prox cannot be passed; B = 65, C = 33, ld = 96, lr = 0 and a null d_ci each return their code
    (-1 FS_EINVAL, -3 FS_EUNSUPPORTED for the batch size the missing wide form would take)."""
    import inspect
    assert 'prox' not in inspect.signature(amd.engine.LocalTrainer.run_scaffold).parameters
    L, P, dev = amd.lib.lib(), amd.lib.ptr, amd.dev
    N, C, B, ld, n = 2, 3, 8, 64, 6
    phi = torch.randn(N * n, ld, device=dev)
    row_off = torch.tensor([0, n, 2 * n], dtype=torch.int64, device=dev)
    labels = torch.zeros(N * n, dtype=torch.int32, device=dev)
    perms = torch.arange(n, dtype=torch.int32, device=dev).repeat(N)
    W0 = torch.zeros(40 * 128, device=dev)                  # flat, large enough for every shape tried
    c = torch.zeros(40 * 128, device=dev)
    ci = torch.full((N * 40 * 128,), SENTINEL, device=dev)
    W_out = torch.full((N * 40 * 128,), SENTINEL, device=dev)
    loss = torch.full((N,), SENTINEL, dtype=torch.float64, device=dev)

    def call(C_=C, B_=B, ld_=ld, lr=0.1, ci_=ci, E_=1):
        return L.fs_local_train_scaffold(P(phi), ld_, P(row_off), P(labels), P(perms), None, N, C_, B_, E_, lr, 0.0, 0,
                                         P(W0), P(c), None if ci_ is None else P(ci_), P(W_out), P(loss),
                                         amd.lib.stream_ptr())

    EINVAL, EUNSUPPORTED = -1, -3
    for kw, code in ((dict(B_=65), EUNSUPPORTED), (dict(C_=33), EINVAL), (dict(ld_=96), EINVAL), (dict(lr=0.0), EINVAL),
                     (dict(ci_=None), EINVAL), (dict(B_=0), EINVAL), (dict(E_=-1), EINVAL)):
        assert call(**kw) == code, kw
        assert 'fs_local_train_scaffold' in L.fs_last_error().decode() or 'local_train_scaffold' in L.fs_last_error().decode()
    torch.cuda.synchronize()
    assert bool((W_out == SENTINEL).all()) and bool((ci == SENTINEL).all()) and bool((loss == SENTINEL).all())
    assert call() == 0                                       # (and the good call does write them)
    torch.cuda.synchronize()
    assert bool((W_out[:N * C * ld] != SENTINEL).all()) and bool((W_out[N * C * ld:] == SENTINEL).all())
    assert bool((loss != SENTINEL).all()) and bool((ci[:N * C * ld] != SENTINEL).all())
    # E = 0: no steps -- x, loss 0 and an unchanged c_i
    ci.fill_(SENTINEL)
    W0[:C * ld] = 0.5
    assert call(E_=0) == 0
    torch.cuda.synchronize()
    assert bool((W_out[:N * C * ld] == 0.5).all()) and bool((loss == 0).all()) and bool((ci == SENTINEL).all())

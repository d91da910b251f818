"""The capped shuffle replay (csrc/randperm.hip randperm_capped_kernel, csrc/randperm_geom.h),
reached as the round plan reaches it (csrc/round.hip): beside a parallel split training launch
that leaves CUs idle, a chunk's shuffles are replayed by a persistent launch of a few workgroups
per XCD (rp_cap_blocks: at most half the idle CUs) of up to 16 waves, wave w taking passes w,
w + total, ...

The replay only decides WHERE a permutation is computed, never which: every run here must give
BITWISE the global model, every client's weights and the loss histories of the same run with the
shuffles replayed on the host (shuffle_device=False: csrc/mt_replay.h, itself pinned to torch's
randperm in test_gpu_parity.py) and of the run with one uncapped-or-capped launch per round
(shuffle_chunk = 1).  Reference: the DataLoader shuffles of the reference's train_loop
(functions/tools.py:179).

Shapes (D = 2048, C = 10, B = 32, E = 2, chunks of 8 rounds, R = 20 unless noted):
  base     100 clients: G = 2, 200 of 256 CUs train, 56 idle; chunks 1 and 2 are launched beside
           training.  Of 65-72 rows: one wave per pass, 16 workgroups of 16 waves = 256 waves for a
           chunk's 1,600 passes, so waves replay six and seven passes.  Of 33-40 rows: no pass is
           longer than 64 rows, so the per-lane form, 8 workgroups looping over 25 blocks of 64
  mixed    the same with clients of 0, 1, 2, 65, 512 and 700 rows mixed in (every kind of pass a
           wave meets: empty, no draw, one draw, just above the per-lane form, the headline's
           length, and a second twist of the generator: more than 624 draws)
  lanes    300 clients of at most 64 rows: the per-lane form (75 blocks of 64 passes per chunk)
  lanes120 120 clients of at most 64 rows: 16 CUs idle -> 8 workgroups loop over 30 blocks
  short    R = 19: the last chunk holds 3 rounds and is launched by flush()
  full     2 * CUs / G + 5 clients: no idle CU, the uncapped geometry

The plan-level cases compare results only, so the capped kernels are also held directly, through
the internal entry the plan calls (fs::randperm_device; engine.Shuffler's ``max_blocks``): capped
against uncapped against the host replay, bitwise, and the length contract -- a pass longer than
the launch's max_n, placed in a later turn of its wave, must come out as the identity permutation
and set the error word without touching the LDS regions of the waves beside it.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, C, B, E, K = 2048, 10, 32, 2, 8
NT = 1024            # test rows: at least 16 per idle CU, so the plan's evaluation blocks count the idle CUs


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine, rng
    from fedamw_amd.functions import tools
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, tools=tools, rng=rng))


def _data(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    Xs = [torch.cos(torch.randn(n, D, generator=g)) / np.sqrt(D) for n in sizes]
    ys = [torch.randint(0, C, (n,), generator=g) for n in sizes]
    Xt = torch.cos(torch.randn(NT, D, generator=g)) / np.sqrt(D)
    yt = torch.randint(0, C, (NT,), generator=g)
    return Xs, ys, Xt, yt


def _run(amd, data, R, shuffle_device, chunk):
    Xs, ys, Xt, yt = data
    torch.manual_seed(23)
    fed = amd.tools.Federation('fedavg', Xs, ys, Xt, yt, None, 'classification', C, D, 0.5, E, B, False, 0.0,
                               True, 1e-4, R, None, 'parallel', verbose=False, shuffle_device=shuffle_device,
                               options={'shuffle_chunk': chunk})
    for _ in range(R):
        fed.round()
    tr, tl, ta = fed.results()
    torch.cuda.synchronize()
    out = dict(W_g=fed.W_g.cpu().numpy(), W_out=fed.trainer.W_out[:len(Xs)].cpu().numpy(),
               loss=fed.loss_hist.cpu().numpy(), ev=fed.eval_hist.cpu().numpy(), tr=tr.numpy(), tl=tl.numpy(),
               ta=ta.numpy())
    return fed, out


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert np.isfinite(a['W_g']).all() and np.isfinite(a['loss']).all()


@pytest.fixture
def empty_clients_ok(amd, monkeypatch):
    """The drop-ins reject a client without rows, as the reference's RandomSampler does; the round
    plan and the kernels take one (a pass of no rows), and the replay must too: these cases step
    over the drop-in's input check to reach it."""
    monkeypatch.setattr(amd.tools, '_check_inputs', lambda *a, **k: None)


def _check(amd, sizes, seed, R, idle):
    """chunks of K rounds on the device == host replay == one device launch per round, bitwise;
    ``idle``: the CUs the training launch must leave idle for the case to mean what it says."""
    data = _data(sizes, seed)
    fed, dev = _run(amd, data, R, True, K)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert fed.trainer.width == 2          # (whichever exchanging form the planner picks at this N)
    assert fed.chunk == K
    if cus == 256:
        assert fed.plan.eval_blocks() == idle, fed.plan.eval_blocks()
    del fed
    _, host = _run(amd, data, R, False, K)
    _same(dev, host, 'host replay')
    _, per_round = _run(amd, data, R, True, 1)
    _same(dev, per_round, 'shuffle_chunk = 1')


ROWS = [(33, 41), (65, 73)]       # the per-lane form (every pass <= 64 rows); one wave per pass


@pytest.mark.parametrize('rows', ROWS)
def test_capped_replay_base(amd, rows):
    rs = np.random.RandomState(1)
    _check(amd, list(rs.randint(*rows, size=100)), 1, 20, 56)


def test_capped_replay_mixed_lengths(amd, empty_clients_ok):
    rs = np.random.RandomState(2)
    sizes = list(rs.randint(33, 41, size=100))
    for j, n in zip(range(3, 100, 9), [0, 1, 2, 65, 512, 700, 0, 65, 2, 1, 512]):
        sizes[j] = n
    _check(amd, sizes, 2, 20, 56)


def test_capped_replay_lanes_form(amd, empty_clients_ok):
    rs = np.random.RandomState(3)
    sizes = list(rs.randint(0, 65, size=300))
    sizes[7], sizes[150] = 64, 0
    _check(amd, sizes, 3, 20, 0)


def test_capped_replay_lanes_form_loops(amd, empty_clients_ok):
    """120 clients: 16 idle CUs, so the per-lane form's 8 workgroups each loop over three or four of a
    chunk's 30 blocks of 64 passes (with 300 clients no CU is idle and the launch is uncapped)."""
    rs = np.random.RandomState(4)
    sizes = list(rs.randint(0, 65, size=120))
    sizes[5], sizes[60] = 64, 0
    _check(amd, sizes, 4, 20, 16)


@pytest.mark.parametrize('rows', ROWS)
def test_capped_replay_short_last_chunk(amd, rows):
    rs = np.random.RandomState(5)
    _check(amd, list(rs.randint(*rows, size=100)), 5, 19, 56)


def test_uncapped_when_no_cu_is_idle(amd):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rs = np.random.RandomState(6)
    _check(amd, list(rs.randint(33, 41, size=2 * cus // 2 + 5)), 6, 20, 0)


def _direct(amd, ns, max_n, max_blocks, seeds):
    """One replay of the passes ``ns`` through the Shuffler; returns (shuffler, output, offsets)."""
    offs = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    sh = amd.engine.Shuffler(ns, offs, int(ns.sum()), torch.device('cuda'), max_n=max_n, max_blocks=max_blocks)
    return sh, sh.run(seeds).cpu().numpy()[:int(ns.sum())], offs


# (max_n, passes, max_blocks): the per-lane form, 10 blocks of 64 passes (the last ragged) on 3
# workgroups; one wave per pass on 2 workgroups of 16 waves (ten turns, the last ragged); LDS
# regions of 10,000 rows (3 waves per workgroup), 2 workgroups, seven turns
DIRECT = [(64, 600, 3), (200, 300, 2), (10000, 40, 2)]


@pytest.mark.parametrize('max_n,P,max_blocks', DIRECT)
def test_capped_kernel_equals_uncapped_and_host(amd, max_n, P, max_blocks):
    rs = np.random.RandomState(max_n)
    torch.manual_seed(max_n)
    seeds = amd.rng.draw_pass_seeds(P)
    ns = rs.randint(0, max_n + 1, size=P).astype(np.int64)
    ns[[1, 2, 3, P - 1]] = [0, 1, 2, max_n]
    sh, capped, offs = _direct(amd, ns, max_n, max_blocks, seeds)
    sh.check_errors()
    sh0, uncapped, _ = _direct(amd, ns, max_n, 0, seeds)
    sh0.check_errors()
    host = np.empty(int(ns.sum()), np.int32)
    amd.rng.randperms(seeds, ns, offs, host)
    assert np.array_equal(capped, host)
    assert np.array_equal(capped, uncapped)


# (max_n, length of the long pass, passes, max_blocks, index of the long pass): the per-lane form,
# the long pass in block 7, its workgroup's third turn; one wave per pass, 32 waves, the long pass
# in its wave's fifth turn and 50 times its LDS row (shuffled, it would run over the regions of the
# 15 waves beside it)
CONTRACT = [(40, 70, 600, 3, 500), (100, 5000, 200, 2, 150)]


@pytest.mark.parametrize('max_n,long_n,P,max_blocks,at', CONTRACT)
def test_capped_contract_violation_raises(amd, max_n, long_n, P, max_blocks, at):
    """test_gpu_parity.py::test_device_randperm_contract_violation_raises through the capped
    geometry: the long pass is the identity, every other pass is still the host's draw, the error
    word is set and check_errors raises once."""
    rs = np.random.RandomState(long_n)
    torch.manual_seed(long_n)
    seeds = amd.rng.draw_pass_seeds(P)
    ns = rs.randint(1, max_n + 1, size=P).astype(np.int64)
    ns[at] = long_n
    sh, out, offs = _direct(amd, ns, max_n, max_blocks, seeds)
    np.testing.assert_array_equal(out[offs[at]:offs[at] + long_n], np.arange(long_n, dtype=np.int32))
    host = np.empty(int(ns.sum()), np.int32)
    amd.rng.randperms(seeds, ns, offs, host)
    keep = np.ones(len(out), bool)
    keep[offs[at]:offs[at] + long_n] = False
    assert np.array_equal(out[keep], host[keep])
    with pytest.raises(amd.lib.FedsimError, match='longer than max_n'):
        sh.check_errors()
    sh.check_errors()                                   # cleared: a second check passes
    ns[at] = max_n                                      # a clean launch of the same geometry
    sh2, out2, offs2 = _direct(amd, ns, max_n, max_blocks, seeds)
    sh2.check_errors()
    host2 = np.empty(int(ns.sum()), np.int32)
    amd.rng.randperms(seeds, ns, offs2, host2)
    assert np.array_equal(out2, host2)

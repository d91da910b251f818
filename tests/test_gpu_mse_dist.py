"""The regression task sharded over two ranks: 2 gloo ranks share the one GPU (as
test_gpu_dist.py), parallel-client FedAvg and FedAMW on the fixture data must match the
single-process run within 4 * 2e-5 relative (the round-level bound of test_gpu_mb.py:200).
FedAMW all-gathers Z in the standard layout: the MSE p-solver has no rank-blocked form."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.mse_fixtures import load_case, split_clients

pytestmark = pytest.mark.gpu

RTOL = 4 * 2e-5


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(algo):
    import fedamw_amd  # noqa: F401
    from fedamw_amd.functions import tools
    d = load_case('mse_fedamw_par' if algo == 'fedamw' else 'mse_fedavg_par')
    Xs, ys = split_clients(d)
    T = torch.from_numpy
    args = ([T(x) for x in Xs], [T(y) for y in ys], T(d['X_test']), T(d['y_test']))
    hp = (float(d['lr']), int(d['epoch']), int(d['batch_size']), bool(d['prox']), float(d['mu']), bool(d['reg']),
          float(d['lam']), int(d['R']))
    torch.manual_seed(int(d['torch_seed']))
    if algo == 'fedamw':
        vl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(T(d['X_val']), T(d['y_val'])),
                                         batch_size=int(d['Bv']), shuffle=True)
        fed = tools.Federation('fedamw', *args, vl, 'regression', 1, int(d['D']), *hp, float(d['lr_p']), 'parallel',
                               verbose=False)
    else:
        fed = tools.Federation('fedavg', *args, None, 'regression', 1, int(d['D']), *hp, None, 'parallel',
                               verbose=False)
    for _ in range(fed.R):
        fed.round()
    out = [o.numpy().astype(np.float64) for o in fed.results()]
    blocks = fed.mixture.blocks if fed.mixture is not None else 0
    return out, fed.W_g[:, :int(d['D'])].cpu().numpy(), blocks


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    try:
        out[rank] = {algo: _run(algo) for algo in ('fedavg', 'fedamw')}
    finally:
        torch.distributed.destroy_process_group()


@pytest.fixture(scope='module')
def sharded():
    """One spawn of two ranks runs both algorithms (no more than two processes in all)."""
    mgr = mp.get_context('spawn').Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    return {r: out[r] for r in range(2)}


@pytest.mark.parametrize('algo', ['fedavg', 'fedamw'])
def test_sharded_regression_matches_single_process(sharded, algo):
    ref, Wref, _ = _run(algo)
    for r in range(2):
        res, W, blocks = sharded[r][algo]
        assert blocks in (0, 1)                        # never the rank-blocked layout under MSE
        err = np.abs(W - Wref).max() / np.abs(Wref).max()
        assert err <= RTOL, (algo, r, err)
        for a, b in zip(res[:2], ref[:2]):
            assert (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max() <= RTOL, (algo, r)
        assert np.abs(res[2] - ref[2]).max() <= 1e-4   # 100 * #{y == 0} / n: independent of the model

"""bench.py's timed path shows its work: ``--dump-outputs DIR`` (bench.dump_outputs, called by
bench.run_workload right after the timed rounds) writes what the last timed round handed back,
and a plain run (no ``--full``) measures the headline only.  Run in-process on a small custom
workload (12 clients x 70 rows, D = 160: one ragged 32-row batch per epoch, D no multiple of 64).

Checks: every array is float32 / float64 with the documented shape and finite; the histories have
warm-up + steps entries (``--steps`` sets the timed rounds); the dumped global model is the
p-weighted sum of the dumped client models (tools.py:345-350 / 455-460: so W_clients and p are the
last round's own), within the aggregate's fp32 tolerance W_RTOL * max|W| (tests/fixtures.py); a
second run with the same arguments writes the same arrays within the parity tolerances of
tests/fixtures.py (same seeded inputs, same code; only the order of a launch's fp32 sums may
differ between runs): W_RTOL * max|.| for models and p, LOSS_RTOL for the losses, one test sample
for the accuracy.
"""
import os

import numpy as np
import pytest
import torch

import bench
from tests.fixtures import LOSS_RTOL, W_RTOL

pytestmark = pytest.mark.gpu

WL = dict(clients=12, rows=70, D=160, C=5, test=90, shape='a9a', config=2)
STEPS, WARMUP = 3, 2


def _run(algo, out_dir, full=False):
    import fedamw_amd  # noqa: F401
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    line = bench.run_workload(dict(WL, algo=algo), 1, 0, dev, STEPS, WARMUP, 100, 0.0, custom=True, full=full,
                              dump_dir=str(out_dir))
    return line, {f[:-4]: np.load(os.path.join(str(out_dir), f)) for f in sorted(os.listdir(str(out_dir)))}


@pytest.mark.parametrize('algo', ['fedavg', 'fedamw'])
def test_dump_outputs_of_the_last_timed_round(algo, tmp_path):
    N, C, D = WL['clients'], WL['C'], WL['D']
    line, a = _run(algo, tmp_path / 'a')
    assert line['steps'] == STEPS and line['ms_per_step'] > 0
    assert abs(line['value'] - N * 1e3 / line['ms_per_step']) <= 1e-6 * line['value']
    assert 'aggregate' not in line and 'cpu_baseline' not in line          # a plain run: the headline only
    want = {'W_global': (C, D), 'train_loss': (WARMUP + STEPS,), 'test_loss': (WARMUP + STEPS,),
            'test_acc': (WARMUP + STEPS,), 'W_clients': (N, C, D), 'W_clients_index': (N,)}
    if algo == 'fedamw':
        want['p'] = (N,)
    assert sorted(a) == sorted(want)
    for k, shape in want.items():
        assert a[k].shape == shape and a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all(), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.array_equal(a['W_clients_index'], np.arange(N))
    p = a['p'] if algo == 'fedamw' else np.full(N, 1.0 / N, np.float32)
    Wsum = np.einsum('n,ncd->cd', p.astype(np.float64), a['W_clients'].astype(np.float64))
    scale = np.abs(a['W_global']).max()
    assert scale > 0 and np.abs(Wsum - a['W_global']).max() <= W_RTOL * scale
    _, b = _run(algo, tmp_path / 'b')
    for k in want:
        tol = {'test_acc': 100.0 / WL['test'] + 1e-4, 'train_loss': LOSS_RTOL * max(1.0, np.abs(a[k]).max()),
               'test_loss': LOSS_RTOL * max(1.0, np.abs(a[k]).max())}.get(k, W_RTOL * np.abs(a[k]).max())
        assert np.abs(a[k] - b[k]).max() <= tol, k


def test_full_adds_the_aggregate_timing(tmp_path):
    line, _ = _run('fedavg', tmp_path / 'c', full=True)
    assert line['aggregate']['kernel'] == 'fs_aggregate' and line['aggregate']['ms'] > 0


def test_client_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """More client models than the budget holds: a fixed sample, the same on every run."""
    monkeypatch.setattr(bench, 'DUMP_CLIENT_BYTES', 5 * 4 * WL['C'] * WL['D'])
    _, a = _run('fedavg', tmp_path / 'd')
    _, b = _run('fedavg', tmp_path / 'e')
    idx = a['W_clients_index']
    assert idx.shape == (5,) and np.array_equal(idx, b['W_clients_index'])
    assert np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < WL['clients']
    assert a['W_clients'].shape == (5, WL['C'], WL['D'])
    assert np.abs(a['W_clients'] - b['W_clients']).max() <= W_RTOL * np.abs(a['W_clients']).max()

"""qffl_drift.json: the float32-versus-float64 distance of tests/qffl_restatement.py over the drop-in
cases of tests/test_gpu_qffl.py (``qffl_restatement.CASES``: q in {0, 1, 5}) -- the method of
fedopt_drift.json.  ``python tests/golden/make_golden_qffl.py``; needs torch and numpy only (q-FedAvg is
not in the reference, so there is no reference run to record).

Per case: delta_W = max over rounds of max|W32 - W64| / max|W64|; delta_loss = the larger of the
train and test loss distances, absolute / max(1, |l|); delta_F, delta_n and delta_H = the relative
distances of the clients' losses, the update norms and H.  The GPU tests use max(bound, 2 delta).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import qffl_restatement as QR  # noqa: E402


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a, b))


def _loss_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def _elem_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    keep = np.isfinite(b) & (b != 0)
    return float((np.abs(a - b)[keep] / np.abs(b)[keep]).max())


def drift(name):
    a, b = QR.run_case(name, np.float32), QR.run_case(name, np.float64)
    out = {'delta_W': _rel(a[3]['W'], b[3]['W']), 'delta_loss': max(_loss_rel(a[0], b[0]), _loss_rel(a[1], b[1])),
           'delta_F': _elem_rel(a[3]['F'], b[3]['F']), 'delta_n': _elem_rel(a[3]['n'], b[3]['n']),
           'delta_H': _elem_rel(a[3]['hc'][:, 0], b[3]['hc'][:, 0])}
    print(name, out, flush=True)
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    res = {name: drift(name) for name in sorted(QR.CASES)}
    with open(os.path.join(HERE, 'qffl_drift.json'), 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)

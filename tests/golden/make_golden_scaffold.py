"""scaffold_drift.json: the float32-versus-float64 distance of tests/scaffold_restatement.py over the
drop-in cases of tests/test_gpu_scaffold.py (``scaffold_restatement.CASES``) -- the method of
mse_drift.json.  ``python tests/golden/make_golden_scaffold.py``; needs torch and numpy only
(SCAFFOLD is not in the reference, so there is no reference run to record).

Per case: delta_W = max over rounds of max|W32 - W64| / max|W64|; delta_c = max over rounds of
max|c32 - c64| / (max|c64| + max|W64| / (K_min lr_t)) -- c is a difference of models divided by
K lr, so a model distance reaches it with that factor (at R = 3 the last round runs at lr0 / 1000)
and the GPU test's tolerance has the same two terms; delta_loss = the larger of the train and test loss distances, absolute / max(1, |l|).
The GPU tests use max(bound, 2 delta) where a recorded delta exceeds half of a bound.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import scaffold_restatement as SR  # noqa: E402


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a, b))


def _loss_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def drift(name):
    a, b = SR.run_case(name, np.float32), SR.run_case(name, np.float64)
    lr, dc = SR.LR, 0.0
    kmin = float(SR.steps(SR.SIZES, SR.E, SR.B).min())
    for t in range(SR.R):
        lr = SR.O.lr_schedule(t, lr, SR.R)
        c32, c64, W64 = a[3]['c'][t].astype(np.float64), b[3]['c'][t], b[3]['W'][t]
        dc = max(dc, float(np.abs(c32 - c64).max() / (np.abs(c64).max() + np.abs(W64).max() / (kmin * lr))))
    out = {'delta_W': _rel(a[3]['W'], b[3]['W']), 'delta_c': dc,
           'delta_loss': max(_loss_rel(a[0], b[0]), _loss_rel(a[1], b[1]))}
    print(name, out, flush=True)
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    res = {name: drift(name) for name in sorted(SR.CASES)}
    with open(os.path.join(HERE, 'scaffold_drift.json'), 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)

"""fedopt_drift.json: the float32-versus-float64 distance of tests/fedopt_restatement.py over the
drop-in cases of tests/test_gpu_fedopt.py (``fedopt_restatement.CASES``) -- the method of
scaffold_drift.json.  ``python tests/golden/make_golden_fedopt.py``; needs torch and numpy only (the
server optimizers are not in the reference, so there is no reference run to record).

Per case: delta_W = max over rounds of max|W32 - W64| / max|W64|; delta_loss = the larger of the
train and test loss distances, absolute / max(1, |l|).  The GPU tests use max(bound, 2 delta).

A condition on the inputs, asserted here in float64: no YOGI case has an element with
|v - d2| <= 4e-5 max|W| |delta| in any round (v the second moment the round meets, d2 = delta^2).
A model error within the GPU test's tolerance (2e-5 max|W| per client model, so at most that in
delta, and 2 |delta| times that in d2) then cannot flip YOGI's sign, and a sign flip cannot hide
under the tolerance.  A case that violates it gets another data seed, never another bound.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import fedopt_restatement as FO  # noqa: E402

SIGN_MARGIN = 4e-5


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a, b))


def _loss_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def yogi_sign_margin(res64):
    """min over rounds and elements of |v - d2| / (max|W| |delta|) in a float64 run (inf where
    delta = 0)."""
    h = res64[3]
    worst = np.inf
    for t in range(len(h['W'])):
        d, v = h['delta'][t], h['v_prev'][t]
        wmax = np.abs(h['W'][t]).max()
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(d != 0, np.abs(v - d * d) / (wmax * np.abs(d)), np.inf)
        worst = min(worst, float(r.min()))
    return worst


def drift(name):
    a, b = FO.run_case(name, np.float32), FO.run_case(name, np.float64)
    out = {'delta_W': _rel(a[3]['W'], b[3]['W']), 'delta_loss': max(_loss_rel(a[0], b[0]), _loss_rel(a[1], b[1]))}
    if FO.CASES[name]['rule'] == 'yogi':
        margin = yogi_sign_margin(b)
        assert margin > SIGN_MARGIN, (name, margin)
        out['yogi_sign_margin'] = margin
    print(name, out, flush=True)
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    res = {name: drift(name) for name in sorted(FO.CASES)}
    with open(os.path.join(HERE, 'fedopt_drift.json'), 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)

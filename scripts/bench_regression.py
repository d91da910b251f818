#!/usr/bin/env python
"""Measure the regression kernels against the classification kernels at C = 1 (one JSON line).

Local training: fs_local_train_mse vs fs_local_train (C = 1, the planner's form) on the same
features, shuffles and shapes -- the per-launch shapes of BASELINE configs 2, 4 and 5 with the
benchmark's E = 2, B = 32, parallel clients.  fs_local_train is the parent's kernel, so its time
in the same process is the baseline.  fs_timer_* events; per repetition 5 warm-up launches then
20 timed launches back to back; three repetitions, the median reported; 100 ms of the kernel's
own launches first so the clocks have settled.  GB/s counts E reads of every
feature row (what has to come from HBM) against the 8 TB/s peak.

p-solve: fs_mix_solve_mse vs fs_mix_solve (C = 1) on the same Z and shuffles, us per step at
N = 100 and N = 1000 with Bv = 16.

Pass condition (the line's "pass"): at the config-4 shape the MSE median is at most 1.05 x the
C = 1 cross-entropy median.  Everything else is recorded only.

    python scripts/bench_regression.py [--out profiles/regression/bench.json] [--shapes 2,4,5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fedamw_amd import _lib, engine  # noqa: E402

SHAPES = {'2': dict(clients=100, rows=512, D=2048), '4': dict(clients=1250, rows=64, D=2048),
          '5': dict(clients=1000, rows=128, D=16384)}
E, B = 2, 32
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
HBM_PEAK_GBS = 8000.0


def time_launches(fn):
    """Median over REPS of the mean per-launch time (ms) of TIMED back-to-back launches."""
    t0 = time.time()
    while (time.time() - t0) * 1e3 < SETTLE_MS:
        fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        for _ in range(WARMUP):
            fn()
        a, b = _lib.Timer(), _lib.Timer()
        a.record()
        for _ in range(TIMED):
            fn()
        b.record()
        out.append(a.elapsed_time(b) / TIMED)
    return float(np.median(out)), [float(v) for v in out]


def bench_train(shape, dev):
    N, rows, D = shape['clients'], shape['rows'], shape['D']
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.cos(torch.randn(N * rows, D, device=dev, generator=g)) / D ** 0.5
    y = 3.0 * torch.randn(N * rows, 1, device=dev, generator=g)
    feats = engine.Features([X[j * rows:(j + 1) * rows] for j in range(N)],
                            [y[j * rows:(j + 1) * rows] for j in range(N)], D, dev, float_targets=True)
    del X
    feats.labels = torch.zeros(N * rows, dtype=torch.int32, device=dev)       # the C = 1 class index
    W0 = torch.zeros(1, feats.ld, device=dev)
    W0[0, :D] = 0.01 * torch.randn(D, device=dev, generator=g)
    seeds = np.arange(1, N * E + 1, dtype=np.int64) * 7919
    res = {}
    for name, loss in (('ce_c1', 'ce'), ('mse', 'mse')):
        tr = engine.LocalTrainer(feats, 1, B, E, chained=False, loss=loss)
        tr.upload_perms(seeds)
        ms, reps = time_launches(lambda: tr.run(W0, 0.05, False, 0.0, False, 0.0, chained=False))
        tr.check_errors()
        res[name] = {'ms': ms, 'reps_ms': reps, 'G': tr.G,
                     'gbs': E * N * rows * feats.ld * 4 / (ms * 1e-3) / 1e9}
        res[name]['hbm_peak_fraction'] = res[name]['gbs'] / HBM_PEAK_GBS
        if loss == 'ce':
            res[name]['kernel'] = _lib.LT_KERNELS.get(_lib.lib().fs_local_train_last_kernel(), '?')
    res['mse_over_ce'] = res['mse']['ms'] / res['ce_c1']['ms']
    res.update(clients=N, rows=rows, D=D, E=E, B=B)
    return res


def bench_solve(N, dev, n_val=2000, Bv=16, epochs=4):
    g = torch.Generator(device=dev).manual_seed(2)
    D = 64
    Xv = torch.zeros(n_val, D)
    yv = 3.0 * torch.randn(n_val, 1, generator=torch.Generator().manual_seed(3))
    p0 = torch.full((N,), 1.0 / N)
    steps = epochs * ((n_val + Bv - 1) // Bv)
    seeds = np.arange(1, epochs + 1, dtype=np.int64) * 104729
    res = {}
    Z = None
    for name, loss in (('ce_c1', 'ce'), ('mse', 'mse')):
        yy = yv if loss == 'mse' else torch.zeros(n_val, dtype=torch.int64)
        mix = engine.Mixture(Xv, yy, D, 1, N, Bv, p0, dev, loss=loss)
        if Z is None:
            Z = torch.randn(mix.Z.shape, device=dev, generator=g)
            Z[:, N:] = 0
        mix.Z.copy_(Z)
        lr_p = 0.1 / float((Z ** 2).sum(dim=1).max())
        mix.prepare(seeds)

        def one():
            mix.solve(None, None, lr_p, slot=0, z=False)
        ms, reps = time_launches(one)
        mix.check_errors()
        res[name] = {'us_per_step': ms * 1e3 / steps, 'reps_us_per_step': [r * 1e3 / steps for r in reps]}
        if loss == 'ce':
            res[name]['solver'] = _lib.SOLVER_NAMES[_lib.lib().fs_mix_solve_last_mode()]
    res.update(N=N, n_val=n_val, Bv=Bv, steps=steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='2,4,5')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    line = {'metric': 'regression_kernels', 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed': TIMED,
            'reps': REPS, 'settle_ms': SETTLE_MS, 'train': {}, 'solve': {},
            'source_revision': {k: _lib.source_revision(k) for k in ('local_train', 'local_train_mse', 'mix_solve_mse')}}
    for s in a.shapes.split(','):
        line['train']['config%s' % s] = bench_train(SHAPES[s], dev)
        torch.cuda.empty_cache()
    for N in (100, 1000):
        line['solve']['N%d' % N] = bench_solve(N, dev)
    if 'config4' in line['train']:
        line['pass'] = bool(line['train']['config4']['mse_over_ce'] <= 1.05)
    text = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(line, indent=1) + '\n')
    print(text)
    return 0 if line.get('pass', True) else 1


if __name__ == '__main__':
    sys.exit(main())

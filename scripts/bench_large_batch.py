#!/usr/bin/env python
"""Measure the wide form of fs_local_train (batch sizes above 64) against the single form at
B = 64, the largest batch that form runs (one JSON line).

Both legs train the same features with the same shuffles (C = 10, E = 2, D = 2048, parallel
clients) and read the same bytes; the wide form at B = 256 runs a quarter of the dependent steps.
fs_timer_* events; 100 ms of the kernel's own launches first so the clocks have settled
(DESIGN.md 5); three repetitions of 5 warm-up + 20 timed launches back to back, the two legs
alternating inside each repetition; the median reported.  GB/s counts E reads of every feature
row (what has to come from HBM) against the 8 TB/s peak.

Shapes: config 4 (1250 clients of 64 rows: B = 64 is one step per epoch for both legs, the wide
form on request) and 100 clients of 512 rows, where the wide form also runs at B = 65, 128, 256,
1024 and the full batch.

Pass condition (the line's "pass"): at 100 x 512 the wide form at B = 256 takes no longer than the
baseline plus the baseline's own run-to-run spread, (max - min) / median over its repetitions.

As recorded in profiles/large_batch/bench.json the condition is MISSED: 0.868 ms for the wide form
at B = 256 against 0.760 ms for the single form at B = 64 (1.14 x, spread 0.09 %); DESIGN.md 4.1 says
what the measurements show about the cause.  The script exits 1 while that holds.

    python scripts/bench_large_batch.py [--out profiles/large_batch/bench.json]
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

SHAPES = {'config4': dict(clients=1250, rows=64, wide_B=(64,)),
          '100x512': dict(clients=100, rows=512, wide_B=(65, 128, 256, 512, 1024))}
D, C, E, BASE_B = 2048, 10, 2, 64
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
HBM_PEAK_GBS = 8000.0


def settle(fn):
    t0 = time.time()
    while (time.time() - t0) * 1e3 < SETTLE_MS:
        fn()
        torch.cuda.synchronize()


def one_rep(fn):
    """Mean per-launch time (ms) of TIMED back-to-back launches after WARMUP."""
    for _ in range(WARMUP):
        fn()
    a, b = _lib.Timer(), _lib.Timer()
    a.record()
    for _ in range(TIMED):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / TIMED


def bench_shape(shape, dev):
    N, rows = shape['clients'], shape['rows']
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.cos(torch.randn(N * rows, D, device=dev, generator=g)) / D ** 0.5
    y = torch.randint(0, C, (N * rows,), device=dev, generator=g)
    feats = engine.Features([X[j * rows:(j + 1) * rows] for j in range(N)],
                            [y[j * rows:(j + 1) * rows] for j in range(N)], D, dev)
    del X
    W0 = torch.zeros(C, feats.ld, device=dev)
    W0[:, :D] = 0.01 * torch.randn(C, D, device=dev, generator=g)
    seeds = np.arange(1, N * E + 1, dtype=np.int64) * 7919
    legs = {}

    def leg(name, B, split):
        tr = engine.LocalTrainer(feats, C, B, E, split=split, chained=False)
        tr.upload_perms(seeds)
        fn = lambda: tr.run(W0, 0.05, False, 0.0, False, 0.0, chained=False)   # noqa: E731
        fn()
        torch.cuda.synchronize()
        legs[name] = dict(fn=fn, tr=tr, B=B, kernel=_lib.LT_KERNELS.get(_lib.lib().fs_local_train_last_kernel(), '?'),
                          reps_ms=[])

    leg('single_B64', BASE_B, 1)
    for B in shape['wide_B']:
        leg('wide_B%d' % B, B, (1 | _lib.G_WIDE) if B <= 64 else None)
    for v in legs.values():
        settle(v['fn'])
    for _ in range(REPS):                 # the legs alternate inside every repetition
        for v in legs.values():
            v['reps_ms'].append(float(one_rep(v['fn'])))
    res = {'clients': N, 'rows': rows, 'D': D, 'C': C, 'E': E, 'legs': {}}
    for name, v in legs.items():
        v['tr'].check_errors()
        ms = float(np.median(v['reps_ms']))
        gbs = E * N * rows * feats.ld * 4 / (ms * 1e-3) / 1e9
        res['legs'][name] = {'B': v['B'], 'kernel': v['kernel'], 'ms': ms, 'reps_ms': v['reps_ms'], 'gbs': gbs,
                             'hbm_peak_fraction': gbs / HBM_PEAK_GBS,
                             'steps_per_epoch': (rows + min(v['B'], rows) - 1) // min(v['B'], rows)}
    base = res['legs']['single_B64']
    res['baseline_spread'] = (max(base['reps_ms']) - min(base['reps_ms'])) / base['ms']
    for name, v in res['legs'].items():
        v['over_baseline'] = v['ms'] / base['ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    line = {'metric': 'large_batch_local_train', 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP,
            'timed': TIMED, 'reps': REPS, 'settle_ms': SETTLE_MS, 'shapes': {},
            'source_revision': {k: _lib.source_revision(k) for k in ('local_train', 'local_train_wide')}}
    for name, shape in SHAPES.items():
        line['shapes'][name] = bench_shape(shape, dev)
        torch.cuda.empty_cache()
    s = line['shapes']['100x512']
    line['pass'] = bool(s['legs']['wide_B256']['over_baseline'] <= 1.0 + s['baseline_spread'])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(line, indent=1) + '\n')
    print(json.dumps(line))
    return 0 if line['pass'] else 1


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python
"""Measure fs_aggregate_nova against fs_aggregate (one JSON line).

The clients x params buffers of BASELINE configs 3, 4 and 5 (N x C*ld = 1000 x 7*4096,
1250 x 10*2048, 1000 x 10*16384), the shapes fs_aggregate folds once per round there.  fs_aggregate
is the parent's kernel, unchanged, so its time in the same process on the same buffers is the
baseline; fs_aggregate_nova runs in both modes (1: the reference form with its correctly rounded
division, 2: the update-normalised form) with the regime fs_aggregate takes (chunks = 0).
fs_timer_* events; 100 ms of the kernel's own launches first so the clocks have settled, then per
repetition 5 warm-up launches and 20 timed launches back to back; three repetitions, the median
reported with all three.  GB/s counts N*len floats read plus len written (mode 2:
plus the base, once per chunk) against the 8 TB/s peak.  Nothing is asserted: the ratios are
recorded.

    python scripts/bench_fednova.py [--out profiles/fednova/bench.json] [--shapes 3,4,5]
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

SHAPES = {'3': dict(clients=1000, C=7, ld=4096), '4': dict(clients=1250, C=10, ld=2048),
          '5': dict(clients=1000, C=10, ld=16384)}
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


def bench_shape(shape, dev):
    N, C, ld = shape['clients'], shape['C'], shape['ld']
    length = C * ld
    g = torch.Generator(device=dev).manual_seed(1)
    W = torch.randn(N, length, device=dev, generator=g)
    n = torch.randint(8, 513, (N,), generator=torch.Generator().manual_seed(2)).double()
    q = (n / n.sum()).float().to(dev)
    b = (n * 2 / 32).float().to(dev)                       # Tau_j = n_j E / B
    te = float((q.double().cpu() * n * 2 / 32).sum())
    base = torch.randn(length, device=dev, generator=g)
    out = torch.empty(length, device=dev)
    agg = engine.Aggregator(N, C, ld, dev)
    # the C entry points with their pointers resolved once: the enqueue must stay shorter than the
    # shortest kernel here (config 4: ~20 us), so no per-call Python checks
    L, P = _lib.lib(), _lib.ptr
    st = _lib.stream_ptr()
    Wp, qp, bp, basep, outp, wsp, wsn = P(W), P(q), P(b), P(base), P(out), P(agg.ws), agg.ws.numel()
    s0 = float(q[0]) * te / float(b[0])

    def plain():
        _lib.check(L.fs_aggregate(Wp, length, qp, N, length, outp, wsp, wsn, 0, st), 'fs_aggregate')

    def nova(mode):
        _lib.check(L.fs_aggregate_nova(Wp, length, None, qp, bp if mode == 1 else None, te, s0, mode,
                                       basep if mode == 2 else None, N, length, outp, wsp, wsn, 0, st),
                   'fs_aggregate_nova')
    runs = (('fs_aggregate', plain), ('nova_reference', lambda: nova(_lib.NOVA_REFERENCE)),
            ('nova_updates', lambda: nova(_lib.NOVA_UPDATES)))
    res = {}
    for name, fn in runs:
        ms, reps = time_launches(fn)
        assert bool(torch.isfinite(out).all()), name
        res[name] = {'us': ms * 1e3, 'reps_us': [r * 1e3 for r in reps],
                     'gbs': 4.0 * (N + 1) * length / (ms * 1e-3) / 1e9}
        res[name]['hbm_peak_fraction'] = res[name]['gbs'] / HBM_PEAK_GBS
    for name in ('nova_reference', 'nova_updates'):
        res[name + '_over_fs_aggregate'] = res[name]['us'] / res['fs_aggregate']['us']
    spread = res['fs_aggregate']['reps_us']
    res['fs_aggregate_rep_spread'] = max(spread) / min(spread)
    res.update(clients=N, C=C, ld=ld, megabytes=4.0 * N * length / 2 ** 20)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='3,4,5')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    line = {'metric': 'fednova_aggregate', 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed': TIMED,
            'reps': REPS, 'settle_ms': SETTLE_MS, 'shapes': {},
            'source_revision': _lib.source_revision('aggregate_nova')}
    for s in a.shapes.split(','):
        line['shapes']['config%s' % s] = bench_shape(SHAPES[s], dev)
        torch.cuda.empty_cache()
    text = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(line, indent=1) + '\n')
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())

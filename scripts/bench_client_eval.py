#!/usr/bin/env python
"""Measure the per-client evaluation (engine.ClientEvaluator: fs_mix_z + fs_z_eval_*; one JSON line).

The capability against what a user could do before it: ``ClientEvaluator.run`` on N resident
client models against the loop of N ``Evaluator.run`` calls (fs_eval, unchanged) on the same
weights and test rows, in the same process -- at config 2's shape (N = 100, C = 10, D = 2048,
10,000 test rows) and at config 3's (N = 1000, C = 7, D = 4096, 50,000 test rows; its 1.4 GB of
logits go through the 256 MB scratch in chunks).  Pass condition (the line's "pass"): the new
path is faster than the loop at both shapes; the ratios are recorded.

The reduction alone: fs_z_eval_add + fs_z_eval_finish on a Z that already exists, us and GB/s of
the one Z read (4 n C ldN bytes), at the Z sizes of config 2 (test rows: 40 MB) and config 5
(pooled validation rows, 32,000 x 10 x 1000: 1.28 GB), and beside each fs_aggregate in the same
process on a clients x params buffer of the same byte count -- both are single-pass streams.  A
record, not a gate.

fs_timer_* events; 100 ms of the measured call's own launches first so the clocks have settled;
per repetition 5 warm-up calls then 20 timed calls back to back; three repetitions, the median
reported (scripts/bench_regression.py's method).

    python scripts/bench_client_eval.py [--out profiles/client_eval/bench.json] [--shapes 2,3]
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

SHAPES = {'2': dict(clients=100, C=10, D=2048, test=10000), '3': dict(clients=1000, C=7, D=4096, test=50000)}
STREAMS = {'config2': dict(n=10000, N=100, C=10), 'config5': dict(n=32000, N=1000, C=10)}
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
HBM_PEAK_GBS = 8000.0


def time_launches(fn):
    """Median over REPS of the mean per-call time (ms) of TIMED back-to-back calls."""
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


def bench_capability(shape, dev):
    N, C, D, n = shape['clients'], shape['C'], shape['D'], shape['test']
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.cos(torch.randn(n, D, device=dev, generator=g)) / D ** 0.5
    y = torch.randint(0, C, (n,), device=dev, generator=g)
    ev = engine.Evaluator(X, y.cpu(), D, C, dev)
    del X
    W = torch.zeros(N, C, ev.f.ld, device=dev)
    W[:, :, :D] = torch.randn(N, C, D, device=dev, generator=g)
    ce = engine.ClientEvaluator(ev.f, C, N)
    out_new = torch.empty(N, 2, dtype=torch.float64, device=dev)
    out_loop = torch.empty(N, 2, dtype=torch.float64, device=dev)

    def loop():
        for j in range(N):
            ev.run(W[j], out_loop[j])

    new_ms, new_reps = time_launches(lambda: ce.run(W, N, out_new))
    loop_ms, loop_reps = time_launches(loop)
    torch.cuda.synchronize()
    dl = float((out_new[:, 0] - out_loop[:, 0]).abs().max())
    same_acc = bool(torch.equal(out_new[:, 1], out_loop[:, 1]))
    ldN = (N + 3) // 4 * 4
    return {'clients': N, 'C': C, 'D': D, 'rows': n, 'chunk_rows': ce.chunk_rows,
            'chunks': -(-n // ce.chunk_rows), 'new_ms': new_ms, 'new_reps_ms': new_reps, 'loop_ms': loop_ms,
            'loop_reps_ms': loop_reps, 'loop_over_new': loop_ms / new_ms,
            'new_gemm_tflops': 2.0 * n * C * ldN * ev.f.ld / (new_ms * 1e-3) / 1e12,
            'loop_feature_bytes': 4.0 * N * n * ev.f.ld, 'z_bytes': 4.0 * n * C * ldN,
            'max_abs_loss_difference': dl, 'accuracies_equal': same_acc}


def bench_stream(s, dev):
    n, N, C = s['n'], s['N'], s['C']
    g = torch.Generator(device=dev).manual_seed(2)
    ldN = (N + 3) // 4 * 4
    Z = torch.randn(n, C * ldN, device=dev, generator=g)
    feats = engine.Features([torch.zeros(n, 64)], [torch.randint(0, C, (n,))], 64, dev)
    ce = engine.ClientEvaluator(feats, C, N)
    out = torch.empty(N, 2, dtype=torch.float64, device=dev)
    ms, reps = time_launches(lambda: ce.run_z(Z, N, out))
    zbytes = 4.0 * n * C * ldN
    res = {'n': n, 'N': N, 'C': C, 'z_bytes': zbytes, 'ws_bytes': 8.0 * ce.ws.numel(), 'us': ms * 1e3,
           'reps_us': [r * 1e3 for r in reps], 'gbs': zbytes / (ms * 1e-3) / 1e9}
    res['hbm_peak_fraction'] = res['gbs'] / HBM_PEAK_GBS
    del ce, feats
    # fs_aggregate on the same bytes: N models of n * C * ldN / N floats (reusing Z's storage)
    length = n * C * ldN // N
    agg = engine.Aggregator(N, 1, length, dev)
    p = torch.full((N,), 1.0 / N, device=dev)
    W_bar = torch.empty(length, device=dev)
    Wv = Z.view(-1)[:N * length].view(N, 1, length)
    ams, areps = time_launches(lambda: agg.run(Wv, p, W_bar))
    res['aggregate'] = {'N': N, 'len': length, 'bytes': 4.0 * N * length, 'us': ams * 1e3,
                        'reps_us': [r * 1e3 for r in areps], 'gbs': 4.0 * N * length / (ams * 1e-3) / 1e9}
    res['z_eval_over_aggregate_rate'] = res['gbs'] / res['aggregate']['gbs']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='2,3')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    line = {'metric': 'client_eval', 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed': TIMED,
            'reps': REPS, 'settle_ms': SETTLE_MS, 'capability': {}, 'stream': {},
            'source_revision': {k: _lib.source_revision(k) for k in ('z_eval', 'mix_z')}}
    for name, s in STREAMS.items():
        line['stream'][name] = bench_stream(s, dev)
        torch.cuda.empty_cache()
    for s in filter(None, a.shapes.split(',')):      # --shapes '': the reduction alone
        line['capability']['config%s' % s] = bench_capability(SHAPES[s], dev)
        torch.cuda.empty_cache()
    line['pass'] = all(c['loop_over_new'] > 1.0 for c in line['capability'].values())
    text = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(line, indent=1) + '\n')
    print(text)
    return 0 if line['pass'] else 1


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python
"""Measure the local evaluation (engine.LocalEvaluator: fs_eval_clients; one JSON line).

On resident features of N equal clients, in one process, at the shapes of config 2 (100 x 512 rows,
D = 2048, C = 10), config 3 (1000 x 465, D = 4096, C = 7) and config 4 (1250 x 64, D = 2048, C = 10):

  (a) fs_eval_clients, w_stride = 0      one model on every client's rows
  (b) fs_eval_clients, w_stride = C ld   W_out[j] on client j
  (c) the loop of N fs_eval calls on the row slices: the only way to these numbers before
  (d) one fs_eval over all rows pooled: the same feature bytes in one launch pair, the rate yardstick
  (e) the smallest fs_eval (1 row, ld = 64, C = 1): a launch pair with next to no work, the price of
      extra launches

Recorded: ms, GB/s of the one feature read (rows ld 4 bytes), (c) / (a) and (a) / (d).  (a) and (c)
are compared bitwise (contract A, include/fedsim.h).  Pass condition (the line's "pass"), at
config 3, whose ragged tails cost most (465 rows = 30 groups per client, 3.2 % more groups than
pooled): the same feature stream may cost only its extra tail groups and its extra launches,

  (a) <= (d) * [sum_j ceil(n_j / 16) / ceil(sum_j n_j / 16)] + (e) + spread of (d)

with spread = max - min of (d)'s three repetitions.

fs_timer_* events; 100 ms of the measured call's own launches first so the clocks have settled;
per repetition 5 warm-up calls then 20 timed calls back to back; three repetitions, the median
reported (scripts/bench_client_eval.py's method).

    python scripts/bench_local_eval.py [--out profiles/local_eval/bench.json] [--shapes 2,3,4]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fedamw_amd import _lib, engine  # noqa: E402

SHAPES = {'2': dict(clients=100, rows=512, D=2048, C=10), '3': dict(clients=1000, rows=465, D=4096, C=7),
          '4': dict(clients=1250, rows=64, D=2048, C=10)}
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
GATE = '3'


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


def bench_empty_pair(dev):
    """(e): fs_eval on one row of 64 columns at one class -- two launches, next to no work."""
    ev = engine.Evaluator(torch.zeros(1, 64), torch.zeros(1, dtype=torch.int64), 64, 1, dev)
    W = torch.zeros(1, 64, device=dev)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    ms, reps = time_launches(lambda: ev.run(W, out))
    return {'ms': ms, 'reps_ms': reps}


def bench_shape(shape, dev):
    N, n_j, D, C = shape['clients'], shape['rows'], shape['D'], shape['C']
    rows = N * n_j
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randint(0, C, (rows,), device=dev, generator=g).cpu()
    # the features generated in place (no second copy of a 7.6 GB buffer): a one-row-per-client
    # Features, then its buffers replaced
    f = engine.Features([torch.zeros(1, D)] * N, [torch.zeros(1, dtype=torch.int64)] * N, D, dev)
    ld = f.ld
    f.ns = np.full(N, n_j, dtype=np.int64)
    f.row_off = np.concatenate([[0], np.cumsum(f.ns)]).astype(np.int64)
    f.rows = rows
    f.phi = torch.zeros(rows, ld, device=dev)
    for r0 in range(0, rows, 1 << 15):           # cos(normal) / sqrt(D), as the feature map's range
        r1 = min(rows, r0 + (1 << 15))
        f.phi[r0:r1, :D] = torch.cos(torch.randn(r1 - r0, D, device=dev, generator=g)) / D ** 0.5
    f.labels = f.targets = y.to(torch.int32).to(dev)
    f.row_off_dev = torch.from_numpy(f.row_off).to(dev)
    W = torch.zeros(N, C, ld, device=dev)
    W[:, :, :D] = torch.randn(N, C, D, device=dev, generator=g)
    le = engine.LocalEvaluator(f, C)
    out_a = torch.empty(N, 2, dtype=torch.float64, device=dev)
    out_b = torch.empty(N, 2, dtype=torch.float64, device=dev)
    out_c = torch.empty(N, 2, dtype=torch.float64, device=dev)
    out_d = torch.empty(2, dtype=torch.float64, device=dev)
    L = _lib.lib()
    ws_c = torch.empty(int(L.fs_eval_ws_doubles(n_j)), dtype=torch.float64, device=dev)
    ws_d = torch.empty(int(L.fs_eval_ws_doubles(rows)), dtype=torch.float64, device=dev)
    vp = ctypes.c_void_p
    phi_j = [vp(f.phi.data_ptr() + 4 * ld * n_j * j) for j in range(N)]
    y_j = [vp(f.labels.data_ptr() + 4 * n_j * j) for j in range(N)]
    out_j = [vp(out_c.data_ptr() + 16 * j) for j in range(N)]
    Wp, wsp = _lib.ptr(W), _lib.ptr(ws_c)

    def loop():
        st = _lib.stream_ptr()
        for j in range(N):
            _lib.check(L.fs_eval(phi_j[j], ld, y_j[j], n_j, Wp, C, out_j[j], wsp, st), 'fs_eval')

    def pooled():
        _lib.check(L.fs_eval(_lib.ptr(f.phi), ld, _lib.ptr(f.labels), rows, Wp, C, _lib.ptr(out_d), _lib.ptr(ws_d),
                             _lib.stream_ptr()), 'fs_eval')

    res = {'clients': N, 'rows_per_client': n_j, 'rows': rows, 'D': D, 'ld': ld, 'C': C,
           'feature_bytes': 4.0 * rows * ld, 'ws_bytes': 8.0 * le.ws.numel()}
    for key, fn in (('a_shared', lambda: le.run(W, 0, out_a)), ('b_own', lambda: le.run(W, C * ld, out_b)),
                    ('d_pooled', pooled), ('c_loop', loop)):
        ms, reps = time_launches(fn)
        res[key] = {'ms': ms, 'reps_ms': reps, 'gbs': res['feature_bytes'] / (ms * 1e-3) / 1e9}
    torch.cuda.synchronize()
    res['a_equals_c_bitwise'] = bool(torch.equal(out_a, out_c))
    # pooled mean = the n_j-weighted sum of the client losses (equal clients: their mean)
    res['objective_vs_pooled_rel'] = float(abs(out_a[:, 0].mean() - out_d[0]) / out_d[0])
    groups = N * ((n_j + 15) // 16)
    res['groups'], res['groups_pooled'] = groups, (rows + 15) // 16
    res['loop_over_new'] = res['c_loop']['ms'] / res['a_shared']['ms']
    res['new_over_pooled'] = res['a_shared']['ms'] / res['d_pooled']['ms']
    res['own_over_shared'] = res['b_own']['ms'] / res['a_shared']['ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='2,3,4')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    line = {'metric': 'local_eval', 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed': TIMED,
            'reps': REPS, 'settle_ms': SETTLE_MS, 'shapes': {}}
    line['e_empty_pair'] = bench_empty_pair(dev)
    for s in filter(None, a.shapes.split(',')):
        line['shapes']['config%s' % s] = bench_shape(SHAPES[s], dev)
        torch.cuda.empty_cache()
    gate = line['shapes'].get('config%s' % GATE)
    if gate is not None:
        d = gate['d_pooled']
        spread = max(d['reps_ms']) - min(d['reps_ms'])
        budget = d['ms'] * gate['groups'] / gate['groups_pooled'] + line['e_empty_pair']['ms'] + spread
        line['gate'] = {'shape': 'config%s' % GATE, 'a_ms': gate['a_shared']['ms'], 'budget_ms': budget,
                        'd_ms': d['ms'], 'group_ratio': gate['groups'] / gate['groups_pooled'],
                        'e_ms': line['e_empty_pair']['ms'], 'd_spread_ms': spread}
        line['pass'] = bool(gate['a_shared']['ms'] <= budget and gate['a_equals_c_bitwise'])
    text = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(line, indent=1) + '\n')
    print(text)
    return 0 if line.get('pass', True) else 1


if __name__ == '__main__':
    sys.exit(main())

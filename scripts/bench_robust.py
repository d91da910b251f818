#!/usr/bin/env python
"""Measure fs_aggregate_robust against the one-read floor and against the torch path.

Part b (``--out``): M rows of len floats at the shapes of BASELINE configs 2 (M = 100, len = 4,096),
3 (M = 1,000, len = 28,672) and 4 (M = 1,250, len = 4,096), and a 10 % sample of config 3 (100 gathered
rows of its 1,000).  For the median and for trim = 0.1, on the same buffer:
  (a) fs_aggregate_sel on the same rows (uniform weights): one read of every row element, a fold --
      the floor of any aggregate that reads the rows once;
  (b) the torch path, what the rule costs today: ``W_all[sel].sort(0)``, the slice, the float64 mean
      (for the median also ``torch.median``; the faster of the two is leg (b));
  the new kernel.
The method of scripts/bench_qffl.py: fs_timer_* events, 100 ms of the leg's own launches first, then
per repetition 5 warm-up and 20 timed launches back to back; three repetitions, the median reported
with all three.  ONE condition is asserted (exit status 1 otherwise): at every shape and rule the
kernel's median time is below leg (b)'s by more than leg (b)'s own (max - min) / median spread.  The
ratio to (a) is recorded only.

Part c (``--round-out``): a whole round, ``FedMedian`` against ``FedAvg(clients='parallel')``, each measured
twice in turn, host-timed over 10 rounds after 3.  Nothing is asserted.

    python scripts/bench_robust.py [--out profiles/robust/bench.json] [--round-out profiles/robust/round.json]
                                   [--round-shapes 2,4] [--parts b,c]
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
from fedamw_amd.functions import tools  # noqa: E402

FOLD_SHAPES = {'config2': dict(M=100, of=100, len=4096), 'config3': dict(M=1000, of=1000, len=28672),
               'config4': dict(M=1250, of=1250, len=4096), 'config3_tenth': dict(M=100, of=1000, len=28672)}
ROUND_SHAPES = {'2': dict(clients=100, rows=512, D=2048, C=10), '3': dict(clients=1000, rows=465, D=4096, C=7),
                '4': dict(clients=1250, rows=64, D=2048, C=10)}
E, B, LR = 2, 32, 0.05
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
ROUNDS_WARM, ROUNDS_TIMED = 3, 10
TRIM = 0.1


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


def entry(ms, reps):
    return {'us': ms * 1e3, 'reps_us': [r * 1e3 for r in reps], 'spread': (max(reps) - min(reps)) / ms}


def bench_fold(shape, dev):
    M, N, length = shape['M'], shape['of'], shape['len']
    gen = torch.Generator(device=dev).manual_seed(5)
    W = torch.randn(N, length, device=dev, generator=gen)
    sel = None if M == N else torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(6))[:M])[0] \
        .to(torch.int32).to(dev)
    sel_all = torch.arange(M, dtype=torch.int32, device=dev) if sel is None else sel
    sel64 = None if sel is None else sel.to(torch.int64)
    q = torch.full((M,), 1.0 / M, device=dev)
    out, out_a = torch.empty(length, device=dev), torch.empty(length, device=dev)
    agg = engine.Aggregator(M, 1, length, dev)
    res = dict(M=M, of=N, len=length, megabytes=4.0 * M * length / 2 ** 20)
    keep = {}

    def floor():
        agg.run_sel(W, sel_all, q, out_a, check=False)

    for rule, b in (('median', (M - 1) // 2), ('trimmed_mean', int(np.floor(TRIM * M)))):
        def kernel():
            agg.run_robust(W, b, out, sel=sel, check=False)

        def torch_sort():
            rows = W if sel64 is None else W[sel64]
            keep['sort'] = rows.sort(0)[0][b:M - b].double().mean(0).float()

        def torch_median():
            rows = W if sel64 is None else W[sel64]
            keep['median'] = rows.median(0)[0]

        one = {'b': b}
        legs = [('fs_aggregate_sel', floor), ('fs_aggregate_robust', kernel), ('torch_sort', torch_sort)]
        if rule == 'median':     # (even M: torch.median is the lower middle value, not the rule; timed all the same)
            legs.append(('torch_median', torch_median))
        for name, fn in legs + [('fs_aggregate_sel_again', floor)]:
            ms, reps = time_launches(fn)
            one[name] = entry(ms, reps)
        # (the two paths agree: the kernel's float64 sum against torch's, one float rounding apart at most)
        one['max_abs_diff_to_torch'] = float((out - keep['sort']).abs().max())
        torch_legs = [k for k in ('torch_sort', 'torch_median') if k in one]
        leg_b = min(torch_legs, key=lambda k: one[k]['us'])
        one['leg_b'] = leg_b
        one['robust_over_floor'] = one['fs_aggregate_robust']['us'] / one['fs_aggregate_sel']['us']
        one['torch_over_robust'] = one[leg_b]['us'] / one['fs_aggregate_robust']['us']
        one['floor_session_spread'] = one['fs_aggregate_sel_again']['us'] / one['fs_aggregate_sel']['us']
        one['gbs'] = 4.0 * M * length / (one['fs_aggregate_robust']['us'] * 1e-6) / 1e9
        one['condition_met'] = bool(one['fs_aggregate_robust']['us'] < one[leg_b]['us'] * (1.0 - one[leg_b]['spread']))
        res[rule] = one
    return res


def clients_of(shape, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    N, n, D, C = shape['clients'], shape['rows'], shape['D'], shape['C']
    Xs = [torch.cos(torch.randn(n, D, device=dev, generator=g)) / D ** 0.5 for _ in range(N)]
    gy = torch.Generator().manual_seed(2)
    ys = [torch.randint(0, C, (n,), generator=gy) for _ in range(N)]
    return Xs, ys


def bench_round(shape, dev):
    D, C = shape['D'], shape['C']
    Xs, ys = clients_of(shape, dev)
    g = torch.Generator(device=dev).manual_seed(7)
    Xt = torch.cos(torch.randn(2000, D, device=dev, generator=g)) / D ** 0.5
    yt = torch.randint(0, C, (2000,), generator=torch.Generator().manual_seed(8))
    R = ROUNDS_WARM + ROUNDS_TIMED
    res = {}
    for algo in ('fedavg', 'fedmedian', 'fedavg_again', 'fedmedian_again'):
        torch.manual_seed(9)
        med = algo.startswith('fedmedian')
        kw = dict(robust=dict(rule='median')) if med else {}
        fed = tools.Federation('fedrobust' if med else 'fedavg', Xs, ys, Xt, yt, None, 'classification', C, D, LR, E, B,
                               False, 0.0, True, 1e-3, R, 1e-3, 'parallel', verbose=False, **kw)
        for _ in range(ROUNDS_WARM):
            fed.round()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ROUNDS_TIMED):
            fed.round()
        torch.cuda.synchronize()
        res[algo] = {'ms_per_round': (time.perf_counter() - t0) * 1e3 / ROUNDS_TIMED,
                     'train_form': _lib.LT_KERNELS.get(_lib.lib().fs_local_train_last_kernel()), 'G': int(fed.trainer.G)}
        tr, tl, ta = fed.results()
        assert bool(torch.isfinite(tl).all())
        del fed
        torch.cuda.empty_cache()
    res['fedmedian_over_fedavg'] = res['fedmedian']['ms_per_round'] / res['fedavg']['ms_per_round']
    res['fedmedian_over_fedavg_again'] = res['fedmedian_again']['ms_per_round'] / res['fedavg_again']['ms_per_round']
    res['fedavg_session_spread'] = res['fedavg_again']['ms_per_round'] / res['fedavg']['ms_per_round']
    return res


def write(path, line):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(json.dumps(line, indent=1) + '\n')
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--round-out', default=None)
    ap.add_argument('--shapes', default=','.join(FOLD_SHAPES))
    ap.add_argument('--round-shapes', default='2,3,4')
    ap.add_argument('--parts', default='b,c')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    parts = a.parts.split(',')
    head = {'device': torch.cuda.get_device_name(0),
            'source_revision': {k: _lib.source_revision(k) for k in ('aggregate_robust', 'aggregate_nova', 'local_train')}}
    ok = True
    if 'b' in parts:
        line = dict(head, metric='robust_aggregate', warmup=WARMUP, timed=TIMED, reps=REPS, settle_ms=SETTLE_MS,
                    trim=TRIM, shapes={})
        for s in a.shapes.split(','):
            line['shapes'][s] = bench_fold(FOLD_SHAPES[s], dev)
            torch.cuda.empty_cache()
        line['condition_met'] = all(line['shapes'][s][r]['condition_met'] for s in line['shapes']
                                    for r in ('median', 'trimmed_mean'))
        ok = line['condition_met']
        write(a.out, line)
    if 'c' in parts:
        line = dict(head, metric='robust_round', E=E, B=B, rounds_warm=ROUNDS_WARM, rounds_timed=ROUNDS_TIMED, shapes={})
        for s in a.round_shapes.split(','):
            line['shapes']['config%s' % s] = bench_round(ROUND_SHAPES[s], dev)
            torch.cuda.empty_cache()
        write(a.round_out, line)
    if not ok:
        print('FAILED: fs_aggregate_robust is not below the torch path by more than its spread', file=sys.stderr)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python
"""Measure rounds with partial client participation (one JSON line; nothing is asserted).

Shape: config 4's per-GPU shape (1250 clients of 64 rows, D = 2048, C = 10, B = 32, E = 2), FedAvg
with parallel clients through ``Federation``, the code path of the drop-ins.

Legs: the existing path (no ``participation``: every client, fs_plan_round, shuffles in chunks of 8
rounds) and the subset path (fs_plan_round_subset, per-round shuffle slots, fs_aggregate_sel) at
participation 1.0, 0.5 and 0.1.  Whole rounds -- seed draws, shuffle replay, training, aggregate,
deferred evaluation -- between two fs_timer_* events: 100 ms of rounds first so the clocks have
settled, then three repetitions of 5 warm-up + 20 timed rounds, the legs alternating
inside each repetition; the median reported, and each leg's spread (max - min) / median.

The one thing to look at: participation 1.0 through the subset path beside the existing path
(``subset_full_over_default``) against the existing path's own spread.

Also fs_aggregate_sel over the M sampled rows at each M against fs_aggregate over all N rows with
zero weights on the unsampled ones (what a caller without the gathered fold would launch): 5 + 20
back-to-back launches per repetition, GB/s counting the rows each has to read.

    python scripts/bench_participation.py [--out profiles/participation/bench.json]
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
from fedamw_amd.functions import participation, tools  # noqa: E402

N, ROWS, D, C, B, E, N_TEST = 1250, 64, 2048, 10, 32, 2, 10000
FRACTIONS = (1.0, 0.5, 0.1)
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
MAX_ROUNDS = 4000                      # rounds a leg's Federation is sized for (settling included)
HBM_PEAK_GBS = 8000.0
SAMPLE_SEED = 1


def timed_ms(fn, count):
    a, b = _lib.Timer(), _lib.Timer()
    a.record()
    for _ in range(count):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / count


def settle(fn, limit=None):
    """SETTLE_MS of back-to-back calls (at most ``limit`` of them)."""
    t0, calls = time.time(), 0
    while (time.time() - t0) * 1e3 < SETTLE_MS and (limit is None or calls < limit):
        fn()
        torch.cuda.synchronize()
        calls += 1


def one_rep(fn):
    for _ in range(WARMUP):
        fn()
    return float(timed_ms(fn, TIMED))


def summary(reps):
    ms = float(np.median(reps))
    return {'ms': ms, 'reps_ms': reps, 'spread': (max(reps) - min(reps)) / ms}


def bench_rounds(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.cos(torch.randn(N * ROWS, D, device=dev, generator=g)) / D ** 0.5
    y = torch.randint(0, C, (N * ROWS,), device=dev, generator=g).cpu()
    Xs = [X[j * ROWS:(j + 1) * ROWS] for j in range(N)]
    ys = [y[j * ROWS:(j + 1) * ROWS] for j in range(N)]
    Xt = torch.cos(torch.randn(N_TEST, D, device=dev, generator=g)) / D ** 0.5
    yt = torch.randint(0, C, (N_TEST,), device=dev, generator=g).cpu()
    legs = {}

    def leg(name, part):
        torch.manual_seed(100)
        fed = tools.Federation('fedavg', Xs, ys, Xt, yt, None, 'classification', C, D, 0.05, E, B, False, 0.0, False,
                               0.0, MAX_ROUNDS, 1e-3, 'parallel', verbose=False, participation=part,
                               sample_seed=SAMPLE_SEED)
        fed.round()
        torch.cuda.synchronize()
        legs[name] = dict(fed=fed, M=N if part is None else participation.sample_size(N, part), reps=[],
                          kernel=_lib.LT_KERNELS.get(_lib.lib().fs_local_train_last_kernel(), '?'))

    leg('default', None)
    for f in FRACTIONS:
        leg('subset_%g' % f, f)
    # a leg never runs past the MAX_ROUNDS its Federation is sized for: the settling takes what
    # the repetitions leave, however short the round
    need = REPS * (WARMUP + TIMED)
    for v in legs.values():
        settle(v['fed'].round, limit=MAX_ROUNDS - v['fed'].t - need)
    for _ in range(REPS):
        for v in legs.values():
            v['reps'].append(one_rep(v['fed'].round))
    out = {}
    for name, v in legs.items():
        fed = v['fed']
        fed.results()                          # completes the deferred evaluation, checks the error words
        out[name] = dict(summary(v['reps']), M=v['M'], kernel=v['kernel'], G=fed.trainer.G, rounds_run=fed.t,
                         shuffle_chunk=fed.chunk, eval_blocks=fed.plan.eval_blocks(),
                         client_rounds_per_s=v['M'] / (float(np.median(v['reps'])) * 1e-3))
    return out


def bench_aggregate(dev):
    length = C * D
    g = torch.Generator(device=dev).manual_seed(2)
    W = torch.randn(N, length, device=dev, generator=g)
    out = torch.empty(length, device=dev)
    res = {}
    for f in FRACTIONS:
        M = participation.sample_size(N, f)
        sel = participation.make_schedule(N, 1, M, SAMPLE_SEED)[0]
        q = torch.rand(M, generator=torch.Generator().manual_seed(3))
        q /= q.sum()
        p = torch.zeros(N)
        p[torch.from_numpy(sel)] = q                       # zero weights on the unsampled rows
        sel_d, q_d, p_d = torch.from_numpy(sel.astype(np.int32)).to(dev), q.to(dev), p.to(dev)
        full, gat = engine.Aggregator(N, C, D, dev), engine.Aggregator(M, C, D, dev)
        gat.run_sel(W, sel_d, q_d, out)                    # (validates sel once; the timed calls do not)
        fns = {'aggregate_all_zero_weights': (lambda: full.run(W, p_d, out), N),
               'aggregate_sel': (lambda: gat.run_sel(W, sel_d, q_d, out, check=False), M)}
        reps = {k: [] for k in fns}
        for fn, _ in fns.values():
            settle(fn)
        for _ in range(REPS):
            for k, (fn, _) in fns.items():
                reps[k].append(one_rep(fn))
        r = {'M': M}
        for k, (_, rows) in fns.items():
            s = summary(reps[k])
            s['bytes'] = 4.0 * (rows + 1) * length
            s['gbs'] = s['bytes'] / (s['ms'] * 1e-3) / 1e9
            s['hbm_peak_fraction'] = s['gbs'] / HBM_PEAK_GBS
            r[k] = s
        r['sel_over_all'] = r['aggregate_sel']['ms'] / r['aggregate_all_zero_weights']['ms']
        res['%g' % f] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    line = {'metric': 'partial_participation', 'device': torch.cuda.get_device_name(0),
            'shape': dict(clients=N, rows=ROWS, D=D, C=C, B=B, E=E, n_test=N_TEST), 'warmup': WARMUP, 'timed': TIMED,
            'reps': REPS, 'settle_ms': SETTLE_MS, 'sample_seed': SAMPLE_SEED,
            'source_revision': dict({k: _lib.source_revision(k) for k in ('local_train',)}, all=_lib.source_revision())}
    line['rounds'] = bench_rounds(dev)
    torch.cuda.empty_cache()
    line['aggregate'] = bench_aggregate(dev)
    r = line['rounds']
    line['subset_full_over_default'] = r['subset_1']['ms'] / r['default']['ms']
    line['default_spread'] = r['default']['spread']
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(line, indent=1) + '\n')
    print(json.dumps(line))
    return 0


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python
"""Measure fs_aggregate_dp and its stages against the dense fs_aggregate_opt (AVGM) on the same buffers.

Part b (``--out``): M rows of len floats at the aggregate shapes 100 x 4,096 (config 2), 1,000 x 28,672
(config 3) and 1,250 x 4,096 (config 4); rows = x + 1e-3 N(0, 1), q = positive weights summing to 1, the clip
at the median update norm (half the rows are scaled), noise multiplier 1.  Timed on the same buffers:
  fs_aggregate_dp (the three stages), fs_dp_norms alone (stage A), fs_dp_coef alone (stage B; the fold is the
  difference), fs_aggregate_dp without noise (z = 0), fs_dp_noise alone, and the dense fs_aggregate_opt AVGM call
  (beta1 = 0, eta = 1), the yardstick.
The method of scripts/bench_topk.py: fs_timer_* events, 100 ms of the leg's own launches first, then per
repetition 5 warm-up and 20 timed launches back to back; three repetitions, the median reported with all
three.  The clipped and the dense leg alternate: dense, clipped, dense again, and the ratio is taken against the
mean of the two dense legs.  The calls update W_g in place, so later launches see the state the earlier ones
left (a random walk of the noise's size: the norms move, the data flow does not).  Bytes/s are against the data
flow's own count (include/fedsim.h): stage A reads M len floats, the fold reads them again; the dense fold M
len.  Nothing is asserted.

Part c (``--round-out``): a whole round at config 3, ``DPFedAvg`` against ``FedAvgM(server_lr=1, beta1=0)``, each
measured twice in turn, host-timed over 10 rounds after 3.  Nothing is asserted.

    python scripts/bench_dp.py [--out profiles/dp/bench.json] [--round-out profiles/dp/round.json]
                               [--shapes config2,config3,config4] [--round-shapes 3] [--parts b,c]
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

FOLD_SHAPES = {'config2': dict(M=100, len=4096), 'config3': dict(M=1000, len=28672), 'config4': dict(M=1250, len=4096)}
ROUND_SHAPES = {'2': dict(clients=100, rows=512, D=2048, C=10), '3': dict(clients=1000, rows=465, D=4096, C=7),
                '4': dict(clients=1250, rows=64, D=2048, C=10)}
E, B, LR = 2, 32, 0.05
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
ROUNDS_WARM, ROUNDS_TIMED = 3, 10
PEAK_HBM_TBS = 8.0


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
    M, length = shape['M'], shape['len']
    gen = torch.Generator(device=dev).manual_seed(5)
    x0 = torch.randn(length, device=dev, generator=gen)
    W = x0[None, :] + 1e-3 * torch.randn(M, length, device=dev, generator=gen)
    q = torch.rand(M, device=dev, generator=gen) + 0.5
    q = (q / q.sum()).contiguous()
    agg = engine.Aggregator(M, 1, length, dev)
    x, xd, m = x0.clone(), x0.clone(), torch.zeros(length, device=dev)
    c = torch.zeros(M, device=dev)
    r = torch.zeros(M, dtype=torch.float64, device=dev)
    n = torch.zeros(M, dtype=torch.float64, device=dev)
    state = torch.zeros(engine.DP_STATE, dtype=torch.float64, device=dev)
    g = torch.zeros(length, device=dev)
    ws = agg.dp_ws()
    agg.dp_norms(W, x, n, ws=ws, check=False)
    clip = float(n.sqrt().median())
    one = dict(M=M, len=length, clip=clip, megabytes=4.0 * M * length / 2 ** 20, ws_bytes=int(ws.numel()))

    def dense():
        agg.run_opt(W, q, 'avgm', xd, m, None, eta=1.0, beta1=0.0, check=False)

    def clipped():
        agg.run_dp(W, q, clip, 1.0, x, c, r, state, seed=1, t=0, ws=ws, check=False)

    def clipped_quiet():
        agg.run_dp(W, q, clip, 0.0, x, c, r, state, seed=1, t=0, ws=ws, check=False)

    def stage_a():
        agg.dp_norms(W, x, n, ws=ws, check=False)

    def stage_b():
        agg.dp_coef(n, q, clip, 1.0, c, r, state, seed=1, t=0)

    def field():
        agg.dp_noise(1, 0, g)

    for name, fn in [('fs_aggregate_opt', dense), ('fs_aggregate_dp', clipped), ('fs_aggregate_opt_again', dense),
                     ('fs_dp_norms', stage_a), ('fs_dp_coef', stage_b), ('fs_aggregate_dp_no_noise', clipped_quiet),
                     ('fs_dp_noise', field)]:
        ms, reps = time_launches(fn)
        one[name] = entry(ms, reps)
    one['clipped_rows'] = float(M - state[2].item() - state[3].item())
    dense_us = 0.5 * (one['fs_aggregate_opt']['us'] + one['fs_aggregate_opt_again']['us'])
    a_us, b_us, all_us = one['fs_dp_norms']['us'], one['fs_dp_coef']['us'], one['fs_aggregate_dp']['us']
    rows_bytes = 4.0 * M * length
    one['fold_us_by_difference'] = all_us - a_us - b_us
    one['dense_us'] = dense_us
    one['dp_over_dense'] = all_us / dense_us
    one['no_noise_over_dense'] = one['fs_aggregate_dp_no_noise']['us'] / dense_us
    one['byte_model_over_dense'] = 2.0                                   # the rows read twice against once
    one['dense_tb_per_s'] = rows_bytes / (dense_us * 1e-6) / 1e12
    one['norms_tb_per_s'] = rows_bytes / (a_us * 1e-6) / 1e12
    one['fold_tb_per_s'] = rows_bytes / (max(all_us - a_us - b_us, 1e-3) * 1e-6) / 1e12
    one['dp_tb_per_s'] = 2.0 * rows_bytes / (all_us * 1e-6) / 1e12
    one['dp_fraction_of_hbm_peak'] = one['dp_tb_per_s'] / PEAK_HBM_TBS
    one['dense_session_spread'] = one['fs_aggregate_opt_again']['us'] / one['fs_aggregate_opt']['us']
    return one


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
    for algo in ('fedavgm', 'dpfedavg', 'fedavgm_again', 'dpfedavg_again', 'dpfedavg_adaptive'):
        torch.manual_seed(9)
        dp = algo.startswith('dpfedavg')
        if dp:
            ad = dict(quantile=0.5, lr=0.2, count_noise=0.0) if algo.endswith('adaptive') else None
            kw = dict(weighting='uniform', dp=dict(clip=0.05, noise_multiplier=1.0, noise_seed=3, adaptive=ad))
        else:
            kw = dict(server_opt=dict(rule='avgm', server_lr=1.0, beta1=0.0))
        fed = tools.Federation('dpfedavg' if dp else 'fedopt', Xs, ys, Xt, yt, None, 'classification', C, D, LR, E, B,
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
    res['dpfedavg_over_fedavgm'] = res['dpfedavg']['ms_per_round'] / res['fedavgm']['ms_per_round']
    res['dpfedavg_over_fedavgm_again'] = res['dpfedavg_again']['ms_per_round'] / res['fedavgm_again']['ms_per_round']
    res['adaptive_over_fedavgm'] = res['dpfedavg_adaptive']['ms_per_round'] / res['fedavgm_again']['ms_per_round']
    res['fedavgm_session_spread'] = res['fedavgm_again']['ms_per_round'] / res['fedavgm']['ms_per_round']
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
    ap.add_argument('--round-shapes', default='3')
    ap.add_argument('--parts', default='b,c')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    parts = a.parts.split(',')
    head = {'device': torch.cuda.get_device_name(0),
            'source_revision': {k: _lib.source_revision(k) for k in ('aggregate_dp', 'aggregate_opt', 'local_train')}}
    if 'b' in parts:
        line = dict(head, metric='dp_aggregate', warmup=WARMUP, timed=TIMED, reps=REPS, settle_ms=SETTLE_MS,
                    peak_hbm_tb_per_s=PEAK_HBM_TBS, shapes={})
        for s in a.shapes.split(','):
            line['shapes'][s] = bench_fold(FOLD_SHAPES[s], dev)
            torch.cuda.empty_cache()
        write(a.out, line)
    if 'c' in parts:
        line = dict(head, metric='dp_round', E=E, B=B, clip=0.05, noise_multiplier=1.0, rounds_warm=ROUNDS_WARM,
                    rounds_timed=ROUNDS_TIMED, shapes={})
        for s in a.round_shapes.split(','):
            line['shapes']['config%s' % s] = bench_round(ROUND_SHAPES[s], dev)
            torch.cuda.empty_cache()
        write(a.round_out, line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python
"""Measure fs_aggregate_topk and its two stages against the dense fs_aggregate_opt (AVGM) on the same buffers.

Part b (``--out``): M rows of len floats at the aggregate shapes 100 x 4,096 (config 2), 1,000 x 28,672
(config 3) and 1,250 x 4,096 (config 4); rows = x + 1e-3 N(0, 1), q = positive weights summing to 1, the
residuals from zero; ratios 0.01 and 0.1 (kcount = floor(ratio * len)).  Timed on the same buffers:
  fs_aggregate_topk with memory (both stages), fs_topk_threshold alone (stage A; the fold is the difference),
  fs_aggregate_topk without memory, and the dense fs_aggregate_opt AVGM call (beta1 = 0, eta = 1), the yardstick.
The method of scripts/bench_rfa.py: fs_timer_* events, 100 ms of the leg's own launches first, then per
repetition 5 warm-up and 20 timed launches back to back; three repetitions, the median reported with all
three.  The sparse and the dense leg alternate: dense, sparse, dense again, and the ratio is taken against the
mean of the two dense legs.  The calls update W_g and the residuals in place, so later launches see the state
the earlier ones left (updates of the same size: the rows do not move).  Bytes/s are against the data flow's
own count (include/fedsim.h): stage A 3 M len floats of HBM traffic (W_k and e_k read, a_k written; the
three re-reads of a_k counted apart as cache traffic), stage B M len read; the dense fold M len.  Nothing is
asserted.

Part c (``--round-out``): a whole round at config 3, ``FedTopK`` against ``FedAvgM(server_lr=1, beta1=0)``, each
measured twice in turn, host-timed over 10 rounds after 3.  Nothing is asserted.

    python scripts/bench_topk.py [--out profiles/topk/bench.json] [--round-out profiles/topk/round.json]
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
RATIOS = (0.01, 0.1)
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


def bench_fold(shape, ratio, dev):
    M, length = shape['M'], shape['len']
    kc = max(1, int(ratio * length))
    gen = torch.Generator(device=dev).manual_seed(5)
    x0 = torch.randn(length, device=dev, generator=gen)
    W = x0[None, :] + 1e-3 * torch.randn(M, length, device=dev, generator=gen)
    q = torch.rand(M, device=dev, generator=gen) + 0.5
    q = (q / q.sum()).contiguous()
    agg = engine.Aggregator(M, 1, length, dev)
    x, e = x0.clone(), torch.zeros(M, length, device=dev)
    xd, m = x0.clone(), torch.zeros(length, device=dev)
    tau = torch.zeros(M, device=dev)
    kept = torch.zeros(M, dtype=torch.int32, device=dev)
    one = dict(M=M, len=length, ratio=ratio, kcount=kc, megabytes=4.0 * M * length / 2 ** 20)

    def dense():
        agg.run_opt(W, q, 'avgm', xd, m, None, eta=1.0, beta1=0.0, check=False)

    def sparse():
        agg.run_topk(W, q, kc, x, e, tau, kept, check=False)

    def stage_a():
        agg.topk_threshold(W, x, e, kc, tau, kept, M=M, check=False)

    def sparse_nomem():
        agg.run_topk(W, q, kc, x, None, tau, kept, check=False)

    sparse()
    one['kept_mean'] = float(kept.double().mean())
    for name, fn in [('fs_aggregate_opt', dense), ('fs_aggregate_topk', sparse), ('fs_aggregate_opt_again', dense),
                     ('fs_topk_threshold', stage_a), ('fs_aggregate_topk_no_memory', sparse_nomem)]:
        if name == 'fs_topk_threshold':
            e.zero_()                       # (stage A alone leaves a_k in e_k: from a zero residual each session)
        ms, reps = time_launches(fn)
        one[name] = entry(ms, reps)
    dense_us = 0.5 * (one['fs_aggregate_opt']['us'] + one['fs_aggregate_opt_again']['us'])
    a_us, all_us = one['fs_topk_threshold']['us'], one['fs_aggregate_topk']['us']
    rows_bytes = 4.0 * M * length
    one['fold_us_by_difference'] = all_us - a_us
    one['dense_us'] = dense_us
    one['topk_over_dense'] = all_us / dense_us
    one['no_memory_over_dense'] = one['fs_aggregate_topk_no_memory']['us'] / dense_us
    one['byte_model_over_dense'] = 4.0                                   # (3 + 1) M len against M len
    one['dense_tb_per_s'] = rows_bytes / (dense_us * 1e-6) / 1e12
    one['stage_a_hbm_tb_per_s'] = 3.0 * rows_bytes / (a_us * 1e-6) / 1e12
    one['stage_a_with_rereads_tb_per_s'] = 6.0 * rows_bytes / (a_us * 1e-6) / 1e12
    one['fold_tb_per_s'] = rows_bytes / (max(all_us - a_us, 1e-3) * 1e-6) / 1e12
    one['topk_tb_per_s'] = 4.0 * rows_bytes / (all_us * 1e-6) / 1e12
    one['topk_fraction_of_hbm_peak'] = one['topk_tb_per_s'] / PEAK_HBM_TBS
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
    for algo in ('fedavgm', 'fedtopk', 'fedavgm_again', 'fedtopk_again', 'fedtopk_no_memory'):
        torch.manual_seed(9)
        tk = algo.startswith('fedtopk')
        if tk:
            kw = dict(topk=dict(ratio=0.01, error_feedback=not algo.endswith('no_memory')))
        else:
            kw = dict(server_opt=dict(rule='avgm', server_lr=1.0, beta1=0.0))
        fed = tools.Federation('fedtopk' if tk else 'fedopt', Xs, ys, Xt, yt, None, 'classification', C, D, LR, E, B,
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
    res['fedtopk_over_fedavgm'] = res['fedtopk']['ms_per_round'] / res['fedavgm']['ms_per_round']
    res['fedtopk_over_fedavgm_again'] = res['fedtopk_again']['ms_per_round'] / res['fedavgm_again']['ms_per_round']
    res['no_memory_over_fedavgm'] = res['fedtopk_no_memory']['ms_per_round'] / res['fedavgm_again']['ms_per_round']
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
            'source_revision': {k: _lib.source_revision(k) for k in ('aggregate_topk', 'aggregate_opt', 'local_train')}}
    if 'b' in parts:
        line = dict(head, metric='topk_aggregate', warmup=WARMUP, timed=TIMED, reps=REPS, settle_ms=SETTLE_MS,
                    peak_hbm_tb_per_s=PEAK_HBM_TBS, shapes={})
        for s in a.shapes.split(','):
            for ratio in RATIOS:
                line['shapes']['%s_ratio%g' % (s, ratio)] = bench_fold(FOLD_SHAPES[s], ratio, dev)
                torch.cuda.empty_cache()
        write(a.out, line)
    if 'c' in parts:
        line = dict(head, metric='topk_round', E=E, B=B, ratio=0.01, rounds_warm=ROUNDS_WARM,
                    rounds_timed=ROUNDS_TIMED, shapes={})
        for s in a.round_shapes.split(','):
            line['shapes']['config%s' % s] = bench_round(ROUND_SHAPES[s], dev)
            torch.cuda.empty_cache()
        write(a.round_out, line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

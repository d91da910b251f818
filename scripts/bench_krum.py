#!/usr/bin/env python
"""Measure fs_aggregate_krum and its stages against the one-read floor and against the torch path.

Part b (``--out``): M rows of len floats at the shapes of BASELINE configs 2 (M = 100, len = 4,096),
3 (M = 1,000, len = 28,672) and 4 (M = 1,250, len = 4,096), and a 10 % sample of config 3 (100 gathered
rows of its 1,000); rows = x + 1e-3 N(0, 1), f = floor(0.1 M), m = M - f.  On the same buffer:
  the distance stage (fs_krum_distances), the select stage (fs_krum_select on that D), the whole chain;
  (a) fs_aggregate_sel on the same rows (uniform weights): one read of every row element, a fold;
  (b) the torch path on the same device: ``U = W[sel] - x; G = U @ U.T; D = diag + diag' - 2 G`` clamped,
      the diagonal masked, ``topk`` of the n smallest, their sum, ``argsort``, the mean of the picked rows.
The method of scripts/bench_robust.py: fs_timer_* events, 100 ms of the leg's own launches first, then
per repetition 5 warm-up and 20 timed launches back to back; three repetitions, the median reported
with all three.  ONE condition is asserted (exit status 1 otherwise): at every shape the chain's
median time is at or below leg (b)'s, the only margin leg (b)'s own (max - min) / median spread.  The
distance stage's TFLOP/s count the triangle's flops, M (M + 1) / 2 * 2 len.

Part c (``--round-out``): a whole round, ``MultiKrum`` against ``FedAvg(clients='parallel')``, each measured
twice in turn, host-timed over 10 rounds after 3.  Nothing is asserted.

    python scripts/bench_krum.py [--out profiles/krum/bench.json] [--round-out profiles/krum/round.json]
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
F_FRAC = 0.1
PEAK_TFLOPS = 157.0


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
    x = torch.randn(length, device=dev, generator=gen)
    W = x[None, :] + 1e-3 * torch.randn(N, length, device=dev, generator=gen)
    sel = None if M == N else torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(6))[:M])[0] \
        .to(torch.int32).to(dev)
    sel_all = torch.arange(M, dtype=torch.int32, device=dev) if sel is None else sel
    sel64 = None if sel is None else sel.to(torch.int64)
    f = int(np.floor(F_FRAC * M))
    m, n = M - f, M - f - 2
    q = torch.full((M,), 1.0 / M, device=dev)
    out, out_a = torch.empty(length, device=dev), torch.empty(length, device=dev)
    agg = engine.Aggregator(M, 1, length, dev)
    ws = agg.krum_ws()
    D = torch.empty(M, engine.krum_ldd(M), device=dev)
    pick = torch.zeros(M, dtype=torch.int32, device=dev)
    score = torch.zeros(M, dtype=torch.float64, device=dev)
    S, kc = engine.krum_split(M, length)
    res = dict(M=M, of=N, len=length, f=f, m=m, megabytes=4.0 * M * length / 2 ** 20, slices=S, ksteps=kc,
               ws_megabytes=ws.numel() / 2 ** 20)
    keep = {}

    def floor():
        agg.run_sel(W, sel_all, q, out_a, check=False)

    def distances():
        agg.krum_distances(W, x, D, ws, sel=sel, check=False)

    def select():
        engine.krum_select(D, M, f, m, score, pick, None, sel)

    def chain():
        agg.run_krum(W, x, f, m, out, pick, score, ws, sel=sel, check=False)

    eye = torch.eye(M, dtype=torch.bool, device=dev)

    def torch_path():
        rows = W if sel64 is None else W[sel64]
        U = rows - x
        G = U @ U.T
        d = G.diagonal()
        Dt = (d[:, None] + d[None, :] - 2.0 * G).clamp_min(0.0).masked_fill(eye, float('inf'))
        sc = Dt.topk(n, dim=1, largest=False)[0].double().sum(1)
        best = torch.argsort(sc, stable=True)[:m]
        keep['out'] = rows[best].mean(0)
        keep['pick'] = best

    one = res
    for name, fn in [('fs_aggregate_sel', floor), ('fs_krum_distances', distances), ('fs_krum_select', select),
                     ('fs_aggregate_krum', chain), ('torch_path', torch_path), ('fs_aggregate_sel_again', floor)]:
        ms, reps = time_launches(fn)
        one[name] = entry(ms, reps)
    picked = torch.sort(pick[:m].to(torch.int64))[0]
    ref = torch.sort(keep['pick'] if sel64 is None else sel64[keep['pick']])[0]
    one['picks_differing_from_torch'] = int((picked != ref).sum())
    one['max_abs_diff_to_torch'] = float((out - keep['out']).abs().max())
    flops = M * (M + 1) / 2 * 2.0 * length
    one['distance_tflops'] = flops / (one['fs_krum_distances']['us'] * 1e-6) / 1e12
    one['distance_fraction_of_peak'] = one['distance_tflops'] / PEAK_TFLOPS
    one['chain_over_floor'] = one['fs_aggregate_krum']['us'] / one['fs_aggregate_sel']['us']
    one['torch_over_chain'] = one['torch_path']['us'] / one['fs_aggregate_krum']['us']
    one['floor_session_spread'] = one['fs_aggregate_sel_again']['us'] / one['fs_aggregate_sel']['us']
    one['condition_met'] = bool(one['fs_aggregate_krum']['us'] <= one['torch_path']['us'] * (1.0 + one['torch_path']['spread']))
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
    for algo in ('fedavg', 'multikrum', 'fedavg_again', 'multikrum_again'):
        torch.manual_seed(9)
        kr = algo.startswith('multikrum')
        kw = dict(krum=dict(f=F_FRAC, m=None)) if kr else {}
        fed = tools.Federation('fedkrum' if kr else 'fedavg', Xs, ys, Xt, yt, None, 'classification', C, D, LR, E, B,
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
    res['multikrum_over_fedavg'] = res['multikrum']['ms_per_round'] / res['fedavg']['ms_per_round']
    res['multikrum_over_fedavg_again'] = res['multikrum_again']['ms_per_round'] / res['fedavg_again']['ms_per_round']
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
    ap.add_argument('--round-shapes', default='2,4')
    ap.add_argument('--parts', default='b,c')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    parts = a.parts.split(',')
    head = {'device': torch.cuda.get_device_name(0),
            'source_revision': {k: _lib.source_revision(k) for k in ('aggregate_krum', 'aggregate_nova', 'local_train')}}
    ok = True
    if 'b' in parts:
        line = dict(head, metric='krum_aggregate', warmup=WARMUP, timed=TIMED, reps=REPS, settle_ms=SETTLE_MS,
                    f_frac=F_FRAC, peak_tflops=PEAK_TFLOPS, shapes={})
        for s in a.shapes.split(','):
            line['shapes'][s] = bench_fold(FOLD_SHAPES[s], dev)
            torch.cuda.empty_cache()
        line['condition_met'] = all(line['shapes'][s]['condition_met'] for s in line['shapes'])
        ok = line['condition_met']
        write(a.out, line)
    if 'c' in parts:
        line = dict(head, metric='krum_round', E=E, B=B, rounds_warm=ROUNDS_WARM, rounds_timed=ROUNDS_TIMED, shapes={})
        for s in a.round_shapes.split(','):
            line['shapes']['config%s' % s] = bench_round(ROUND_SHAPES[s], dev)
            torch.cuda.empty_cache()
        write(a.round_out, line)
    if not ok:
        print('FAILED: fs_aggregate_krum is not at or below the torch path at every shape', file=sys.stderr)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())

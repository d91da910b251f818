#!/usr/bin/env python
"""Measure SCAFFOLD's kernels against the parent's (one JSON line), at the shapes of BASELINE
configs 2, 3 and 4.

(a) training   fs_local_train_scaffold against fs_local_train at G = 1 (the parent's single form) in
               the same process on the same features and shuffles.  The added work is 2*C*ld*4 bytes
               of L2 reads per step plus one epilogue pass per client; the ratio is reported.
(b) dual fold  fs_aggregate_scaffold against two back-to-back fs_aggregate_nova mode-2 launches (the
               parent's kernel; what folding W_g and c separately would cost), over all N clients and
               over M = N / 10 sampled rows.  Algorithmic bytes (M + 4) / (2M + 4) ~ 0.5.
(c) round      a whole Scaffold round against a FedAvg(clients='parallel') round in the planner's
               form (host-timed over back-to-back rounds after a synchronise, shuffles and evaluation
               included): the full cost of SCAFFOLD as built, the missing split / pipe forms included.

(a) and (b): fs_timer_* events; 100 ms of the kernel's own launches first, then per repetition 5
warm-up and 20 timed launches back to back; three repetitions, the median reported with all three
(the method of scripts/bench_regression.py).  Nothing is asserted: the ratios are recorded.

    python scripts/bench_scaffold.py [--out profiles/scaffold/bench.json] [--shapes 2,3,4] [--parts a,b,c]
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
from fedamw_amd import _lib, engine, rng  # noqa: E402
from fedamw_amd.functions import tools  # noqa: E402

SHAPES = {'2': dict(clients=100, rows=512, D=2048, C=10), '3': dict(clients=1000, rows=465, D=4096, C=7),
          '4': dict(clients=1250, rows=64, D=2048, C=10)}
E, B, LR = 2, 32, 0.05
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
ROUNDS_WARM, ROUNDS_TIMED = 3, 10


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
    return {'us': ms * 1e3, 'reps_us': [r * 1e3 for r in reps]}


def clients_of(shape, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    N, n, D, C = shape['clients'], shape['rows'], shape['D'], shape['C']
    Xs = [torch.cos(torch.randn(n, D, device=dev, generator=g)) / D ** 0.5 for _ in range(N)]
    gy = torch.Generator().manual_seed(2)
    ys = [torch.randint(0, C, (n,), generator=gy) for _ in range(N)]
    return Xs, ys


def bench_train(shape, dev, Xs, ys):
    N, D, C = shape['clients'], shape['D'], shape['C']
    feats = engine.Features(Xs, ys, D, dev)
    tr = engine.LocalTrainer(feats, C, B, E, split=1)
    torch.manual_seed(3)
    tr.upload_perms(rng.draw_pass_seeds(N * E))
    g = torch.Generator(device=dev).manual_seed(4)
    W0 = 0.1 * torch.randn(C, feats.ld, device=dev, generator=g)
    c = 0.01 * torch.randn(C, feats.ld, device=dev, generator=g)
    ci = 0.01 * torch.randn(N, C, feats.ld, device=dev, generator=g)
    res = {}
    ms, reps = time_launches(lambda: tr.run(W0, LR, False, 0.0, True, 1e-3, False))
    res['fs_local_train_G1'] = entry(ms, reps)
    ms, reps = time_launches(lambda: tr.run_scaffold(W0, LR, True, 1e-3, c, ci))
    res['fs_local_train_scaffold'] = entry(ms, reps)
    assert bool(torch.isfinite(tr.W_out).all())
    res['scaffold_over_G1'] = res['fs_local_train_scaffold']['us'] / res['fs_local_train_G1']['us']
    steps = E * -(-shape['rows'] // B)
    res.update(steps_per_client=steps, added_l2_bytes_per_step=2 * C * feats.ld * 4,
               batch_bytes_per_step=B * feats.ld * 4)
    return res


def bench_fold(shape, dev):
    N, C, ld = shape['clients'], shape['C'], engine.pad_ld(shape['D'])
    length = C * ld
    g = torch.Generator(device=dev).manual_seed(5)
    W = torch.randn(N, length, device=dev, generator=g)
    res = {}
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    for label, M in (('all', N), ('tenth', N // 10)):
        sel = None if M == N else torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(6))[:M])[0] \
            .to(torch.int32).to(dev)
        q = torch.full((M,), 1.0 / M, device=dev)
        r = torch.full((M,), 0.37 / M, device=dev)
        Wg = torch.randn(length, device=dev, generator=g)
        cg = torch.randn(length, device=dev, generator=g)
        agg = engine.Aggregator(M, C, ld, dev)
        Wp, qp, rp, Wgp, cgp, wsp, wsn = P(W), P(q), P(r), P(Wg), P(cg), P(agg.ws), agg.ws.numel()
        selp = None if sel is None else P(sel)

        def dual():
            _lib.check(L.fs_aggregate_scaffold(Wp, length, selp, qp, rp, 0.9, M, length, Wgp, cgp, wsp, wsn, 0, st),
                       'fs_aggregate_scaffold')

        def two():
            for out, coef in ((Wgp, qp), (cgp, rp)):
                _lib.check(L.fs_aggregate_nova(Wp, length, selp, coef, None, 1.0, 1.0, _lib.NOVA_UPDATES, out, M, length,
                                               out, wsp, wsn, 0, st), 'fs_aggregate_nova')
        one = {}
        ms, reps = time_launches(two)
        one['two_nova_mode2'] = entry(ms, reps)
        one['two_nova_mode2']['gbs'] = 4.0 * 2 * (M + 2) * length / (ms * 1e-3) / 1e9
        ms, reps = time_launches(dual)
        one['fs_aggregate_scaffold'] = entry(ms, reps)
        one['fs_aggregate_scaffold']['gbs'] = 4.0 * (M + 4) * length / (ms * 1e-3) / 1e9
        one['dual_over_two'] = one['fs_aggregate_scaffold']['us'] / one['two_nova_mode2']['us']
        one.update(M=M, of=N, bytes_ratio=(M + 4) / (2 * M + 4), megabytes=4.0 * M * length / 2 ** 20)
        res[label] = one
    return res


def bench_round(shape, dev, Xs, ys):
    D, C = shape['D'], shape['C']
    g = torch.Generator(device=dev).manual_seed(7)
    Xt = torch.cos(torch.randn(2000, D, device=dev, generator=g)) / D ** 0.5
    yt = torch.randint(0, C, (2000,), generator=torch.Generator().manual_seed(8))
    R = ROUNDS_WARM + ROUNDS_TIMED
    res = {}
    for algo in ('fedavg', 'scaffold'):
        torch.manual_seed(9)
        fed = tools.Federation(algo, Xs, ys, Xt, yt, None, 'classification', C, D, LR, E, B, False, 0.0, True, 1e-3, R,
                               1e-3, 'parallel', verbose=False)
        for _ in range(ROUNDS_WARM):
            fed.round()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ROUNDS_TIMED):
            fed.round()
        torch.cuda.synchronize()
        res[algo] = {'ms_per_round': (time.perf_counter() - t0) * 1e3 / ROUNDS_TIMED,
                     'train_form': _lib.LT_KERNELS.get(_lib.lib().fs_local_train_last_kernel()) if algo == 'fedavg'
                     else 'scaffold (one workgroup per client)', 'G': int(fed.trainer.G)}
        tr, tl, ta = fed.results()
        assert bool(torch.isfinite(tl).all())
        del fed
        torch.cuda.empty_cache()
    res['scaffold_over_fedavg'] = res['scaffold']['ms_per_round'] / res['fedavg']['ms_per_round']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='2,3,4')
    ap.add_argument('--parts', default='a,b,c')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    parts = a.parts.split(',')
    line = {'metric': 'scaffold', 'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'timed': TIMED, 'reps': REPS,
            'settle_ms': SETTLE_MS, 'E': E, 'B': B, 'rounds_warm': ROUNDS_WARM, 'rounds_timed': ROUNDS_TIMED,
            'train': {}, 'fold': {}, 'round': {}, 'source_revision': {k: _lib.source_revision(k) for k in ('local_train', 'local_train_scaffold', 'aggregate_nova', 'aggregate_scaffold')}}
    for s in a.shapes.split(','):
        shape, key = SHAPES[s], 'config%s' % s
        Xs, ys = clients_of(shape, dev) if ('a' in parts or 'c' in parts) else (None, None)
        if 'a' in parts:
            line['train'][key] = bench_train(shape, dev, Xs, ys)
            torch.cuda.empty_cache()
        if 'b' in parts:
            line['fold'][key] = bench_fold(shape, dev)
            torch.cuda.empty_cache()
        if 'c' in parts:
            line['round'][key] = bench_round(shape, dev, Xs, ys)
        del Xs, ys
        torch.cuda.empty_cache()
        print(key, json.dumps({k: line[k].get(key) for k in ('train', 'fold', 'round')}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(line, indent=1) + '\n')
    print(json.dumps(line))
    return 0


if __name__ == '__main__':
    sys.exit(main())

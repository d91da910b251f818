#!/usr/bin/env python
"""Measure fs_aggregate_opt against fs_aggregate_nova's mode 2 and against the unfused server step.

Part b (``--out``): the clients x params buffers of BASELINE configs 2, 3, 4 and 5, with all N rows
and with M = N/10 gathered rows.  Per rule, on the same buffers: fs_aggregate_opt; fs_aggregate_nova
mode 2 alone (the parent's kernel: what FedAvg's own update-form aggregate costs, the floor); and the
unfused path, mode 2 into a scratch model plus the torch element-wise step.  The method of
scripts/bench_fednova.py: fs_timer_* events, 100 ms of the kernel's own launches first, then per
repetition 5 warm-up and 20 timed launches back to back; three repetitions, the median reported with
all three.  The bytes predict fused / mode 2 = (M + 6)/(M + 2) where HBM-bound ((M + 4)/(M + 2) for
avgm); the record holds that prediction and mode 2's own repetition spread beside every ratio.

Part c (``--round-out``): a whole round, ``FedAdam`` against ``FedAvg(clients='parallel')`` at configs 2-4,
host-timed over 10 rounds after 3 (scripts/bench_scaffold.py's method).  Nothing is asserted.

    python scripts/bench_fedopt.py [--out profiles/fedopt/bench.json] [--round-out profiles/fedopt/round.json]
                                   [--shapes 2,3,4,5] [--parts b,c]
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

SHAPES = {'2': dict(clients=100, rows=512, D=2048, C=10), '3': dict(clients=1000, rows=465, D=4096, C=7),
          '4': dict(clients=1250, rows=64, D=2048, C=10), '5': dict(clients=1000, rows=0, D=16384, C=10)}
E, B, LR = 2, 32, 0.05
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
ROUNDS_WARM, ROUNDS_TIMED = 3, 10
RULES = ('avgm', 'adagrad', 'adam', 'yogi')


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
    return {'us': ms * 1e3, 'reps_us': [r * 1e3 for r in reps], 'rep_spread': max(reps) / min(reps)}


def torch_step(rule, sc, scratch, Wg, m, v, d):
    """The unfused server step on a folded model in ``scratch`` (= Wg + delta): torch element-wise ops."""
    eta, b1, o1, b2, o2, tau = sc
    torch.sub(scratch, Wg, out=d)
    if rule == 'avgm':
        m.mul_(b1).add_(d)
        Wg.add_(m, alpha=eta)
        return
    m.mul_(b1).add_(d, alpha=o1)
    if rule == 'adagrad':
        v.addcmul_(d, d)
    elif rule == 'adam':
        v.mul_(b2).addcmul_(d, d, value=o2)
    else:
        d.mul_(d)
        v.sub_(torch.sign(v - d).mul_(d), alpha=o2)
    Wg.addcdiv_(m, v.sqrt().add_(tau), value=eta)


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
        Wg = torch.randn(length, device=dev, generator=g)
        m = torch.zeros(length, device=dev)
        v = torch.full((length,), 1e-2, device=dev)
        scratch, d = torch.empty(length, device=dev), torch.empty(length, device=dev)
        agg = engine.Aggregator(M, C, ld, dev)
        Wp, qp, Wgp, mp, vp, sp, wsp, wsn = P(W), P(q), P(Wg), P(m), P(v), P(scratch), P(agg.ws), agg.ws.numel()
        selp = None if sel is None else P(sel)

        def mode2(out=Wgp):
            _lib.check(L.fs_aggregate_nova(Wp, length, selp, qp, None, 1.0, 1.0, _lib.NOVA_UPDATES, Wgp, M, length, out,
                                           wsp, wsn, 0, st), 'fs_aggregate_nova')
        one = {}
        ms, reps = time_launches(mode2)
        one['nova_mode2'] = entry(ms, reps)
        one['nova_mode2']['gbs'] = 4.0 * (M + 2) * length / (ms * 1e-3) / 1e9
        for rule in RULES:
            rid, *sc = tools.server_opt_scalars(rule, 0.1, 0.9, 0.99, 1e-3)
            sc = [float(a) for a in sc]
            Wg.normal_(generator=g)
            m.zero_()
            v.fill_(1e-2)

            def fused():
                _lib.check(L.fs_aggregate_opt(Wp, length, selp, qp, rid, *sc, M, length, Wgp, mp,
                                              None if rule == 'avgm' else vp, wsp, wsn, 0, st), 'fs_aggregate_opt')

            def unfused():
                mode2(sp)
                torch_step(rule, sc, scratch, Wg, m, v, d)
            extra = 4 if rule == 'avgm' else 6
            r = {}
            ms, reps = time_launches(fused)
            r['fs_aggregate_opt'] = entry(ms, reps)
            r['fs_aggregate_opt']['gbs'] = 4.0 * (M + extra) * length / (ms * 1e-3) / 1e9
            assert bool(torch.isfinite(Wg).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all()), rule
            ms, reps = time_launches(unfused)
            r['unfused'] = entry(ms, reps)
            assert bool(torch.isfinite(Wg).all()), rule
            r['fused_over_mode2'] = r['fs_aggregate_opt']['us'] / one['nova_mode2']['us']
            r['predicted_fused_over_mode2'] = (M + extra) / (M + 2.0)
            r['unfused_over_fused'] = r['unfused']['us'] / r['fs_aggregate_opt']['us']
            one[rule] = r
        one.update(M=M, of=N, megabytes=4.0 * M * length / 2 ** 20)
        res[label] = one
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
    for algo in ('fedavg', 'fedopt', 'fedavg_again', 'fedopt_again'):
        torch.manual_seed(9)
        kw = dict(server_opt=dict(rule='adam')) if algo.startswith('fedopt') else {}
        fed = tools.Federation(algo.split('_')[0], Xs, ys, Xt, yt, None, 'classification', C, D, LR, E, B, False, 0.0,
                               True, 1e-3, R, 1e-3, 'parallel', verbose=False, **kw)
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
    res['fedadam_over_fedavg'] = res['fedopt']['ms_per_round'] / res['fedavg']['ms_per_round']
    res['fedadam_over_fedavg_again'] = res['fedopt_again']['ms_per_round'] / res['fedavg_again']['ms_per_round']
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
    ap.add_argument('--shapes', default='2,3,4,5')
    ap.add_argument('--parts', default='b,c')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    parts = a.parts.split(',')
    head = {'device': torch.cuda.get_device_name(0),
            'source_revision': {k: _lib.source_revision(k) for k in ('aggregate_opt', 'aggregate_nova', 'local_train')}}
    if 'b' in parts:
        line = dict(head, metric='fedopt_aggregate', warmup=WARMUP, timed=TIMED, reps=REPS, settle_ms=SETTLE_MS, shapes={})
        for s in a.shapes.split(','):
            line['shapes']['config%s' % s] = bench_fold(SHAPES[s], dev)
            torch.cuda.empty_cache()
        write(a.out, line)
    if 'c' in parts:
        line = dict(head, metric='fedopt_round', E=E, B=B, rounds_warm=ROUNDS_WARM, rounds_timed=ROUNDS_TIMED, shapes={})
        for s in a.shapes.split(','):
            if SHAPES[s]['rows']:
                line['shapes']['config%s' % s] = bench_round(SHAPES[s], dev)
                torch.cuda.empty_cache()
        write(a.round_out, line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python
"""Measure fs_aggregate_qffl against fs_aggregate_nova's mode 2 and against the unfused q-FedAvg step.

Part b (``--out``): the clients x params buffers of BASELINE configs 2, 3, 4 and 5, with all N rows
and with M = N/10 gathered rows.  On the same buffers: fs_aggregate_qffl (the pass, the norm reduce
and the step: three launches, four in the two-stage form); fs_aggregate_nova mode 2 alone (the
parent's kernel: what FedAvg's own update-form aggregate costs, the floor); fs_aggregate_opt's AVGM
(the same fold with a fused element-wise finish and no norms: the difference to it is what the norms
and the two small launches cost); and the unfused path, mode 2 into a scratch model plus torch's
per-row norms plus the torch element-wise step.  The method of scripts/bench_fedopt.py: fs_timer_*
events, 100 ms of the kernel's own launches first, then per repetition 5 warm-up and 20 timed launches
back to back; three repetitions, the median reported with all three.  The bytes predict
qffl / mode 2 = (M + 3)/(M + 2) where HBM-bound; the record holds that prediction and mode 2's own
repetition spread beside the ratio.

Part c (``--round-out``): a whole round, ``QFedAvg`` against ``FedAvg(clients='parallel')`` at configs 2-4,
each measured twice in turn, host-timed over 10 rounds after 3.  Nothing is asserted.

    python scripts/bench_qffl.py [--out profiles/qffl/bench.json] [--round-out profiles/qffl/round.json]
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
LC = 20.0


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


def bench_fold(shape, dev):
    N, C, ld = shape['clients'], shape['C'], engine.pad_ld(shape['D'])
    length = C * ld
    gen = torch.Generator(device=dev).manual_seed(5)
    W = torch.randn(N, length, device=dev, generator=gen)
    res = {}
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    for label, M in (('all', N), ('tenth', N // 10)):
        sel = None if M == N else torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(6))[:M])[0] \
            .to(torch.int32).to(dev)
        sel64 = None if sel is None else sel.to(torch.int64)
        u = torch.full((M,), 1.0 / M, device=dev)
        g = torch.full((M,), 0.5 / M, device=dev)
        Wg = torch.randn(length, device=dev, generator=gen)
        S, m, scratch = (torch.empty(length, device=dev) for _ in range(3))
        n = torch.empty(M, dtype=torch.float64, device=dev)
        hc = torch.empty(2, dtype=torch.float64, device=dev)
        agg = engine.Aggregator(M, C, ld, dev)
        nws = agg.qffl_ws(M)
        Wp, up, gp, Wgp, Sp, mp, sp, wsp, wsn = P(W), P(u), P(g), P(Wg), P(S), P(m), P(scratch), P(agg.ws), agg.ws.numel()
        selp = None if sel is None else P(sel)

        def mode2(out=Wgp):
            _lib.check(L.fs_aggregate_nova(Wp, length, selp, up, None, 1.0, 1.0, _lib.NOVA_UPDATES, Wgp, M, length, out,
                                           wsp, wsn, 0, st), 'fs_aggregate_nova')

        def qffl():
            _lib.check(L.fs_aggregate_qffl(Wp, length, selp, up, gp, LC, M, length, Wgp, Sp, P(n), P(hc), wsp, wsn, 0,
                                           P(nws), nws.numel(), st), 'fs_aggregate_qffl')

        def avgm():
            _lib.check(L.fs_aggregate_opt(Wp, length, selp, up, _lib.OPT_AVGM, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, M, length, Wgp,
                                          mp, None, wsp, wsn, 0, st), 'fs_aggregate_opt')

        def unfused():
            mode2(sp)
            rows = W if sel64 is None else W.index_select(0, sel64)
            nn = torch.linalg.vector_norm(rows - Wg, dim=1).double().square_()
            H = LC * u.double().sum() + (g.double() * nn).sum()
            Wg.add_((scratch - Wg) * (LC / H).float())

        one = {}
        for name, fn in (('nova_mode2', mode2), ('fs_aggregate_qffl', qffl), ('fs_aggregate_opt_avgm', avgm),
                         ('nova_mode2_again', mode2), ('unfused', unfused)):
            Wg.normal_(generator=gen)
            ms, reps = time_launches(fn)
            one[name] = entry(ms, reps)
            assert bool(torch.isfinite(Wg).all()), name
        one['nova_mode2']['gbs'] = 4.0 * (M + 2) * length / (one['nova_mode2']['us'] * 1e-6) / 1e9
        one['fs_aggregate_qffl']['gbs'] = 4.0 * (M + 3) * length / (one['fs_aggregate_qffl']['us'] * 1e-6) / 1e9
        one['H_coef'] = [float(v) for v in hc.cpu()]
        one['qffl_over_mode2'] = one['fs_aggregate_qffl']['us'] / one['nova_mode2']['us']
        one['predicted_qffl_over_mode2'] = (M + 3.0) / (M + 2.0)
        one['mode2_session_spread'] = one['nova_mode2_again']['us'] / one['nova_mode2']['us']
        one['qffl_minus_avgm_us'] = one['fs_aggregate_qffl']['us'] - one['fs_aggregate_opt_avgm']['us']
        one['unfused_over_qffl'] = one['unfused']['us'] / one['fs_aggregate_qffl']['us']
        one.update(M=M, of=N, megabytes=4.0 * M * length / 2 ** 20, table_floats=int(nws.numel()) * 2)
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
    for algo in ('fedavg', 'qfedavg', 'fedavg_again', 'qfedavg_again'):
        torch.manual_seed(9)
        kw = dict(qffl=dict(q=1.0)) if algo.startswith('qfedavg') else {}
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
        if algo == 'qfedavg':
            # the evaluation pass alone on the same model: the expected extra of a round
            out2 = torch.empty(fed.N, 2, dtype=torch.float64, device=dev)
            ms, reps = time_launches(lambda: fed.qf_eval.run(fed.W_g, 0, out2))
            res['local_eval_pass'] = entry(ms, reps)
        tr, tl, ta = fed.results()
        assert bool(torch.isfinite(tl).all())
        del fed
        torch.cuda.empty_cache()
    res['qfedavg_over_fedavg'] = res['qfedavg']['ms_per_round'] / res['fedavg']['ms_per_round']
    res['qfedavg_over_fedavg_again'] = res['qfedavg_again']['ms_per_round'] / res['fedavg_again']['ms_per_round']
    res['qfedavg_minus_fedavg_ms'] = res['qfedavg']['ms_per_round'] - res['fedavg']['ms_per_round']
    res['qfedavg_minus_fedavg_again_ms'] = res['qfedavg_again']['ms_per_round'] - res['fedavg_again']['ms_per_round']
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
            'source_revision': {k: _lib.source_revision(k) for k in ('aggregate_qffl', 'aggregate_nova', 'local_train')}}
    if 'b' in parts:
        line = dict(head, metric='qffl_aggregate', warmup=WARMUP, timed=TIMED, reps=REPS, settle_ms=SETTLE_MS, shapes={})
        for s in a.shapes.split(','):
            line['shapes']['config%s' % s] = bench_fold(SHAPES[s], dev)
            torch.cuda.empty_cache()
        write(a.out, line)
    if 'c' in parts:
        line = dict(head, metric='qffl_round', E=E, B=B, rounds_warm=ROUNDS_WARM, rounds_timed=ROUNDS_TIMED, shapes={})
        for s in a.shapes.split(','):
            if SHAPES[s]['rows']:
                line['shapes']['config%s' % s] = bench_round(SHAPES[s], dev)
                torch.cuda.empty_cache()
        write(a.round_out, line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

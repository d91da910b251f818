#!/usr/bin/env python
"""Measure fs_aggregate_rfa and one fs_rfa_step against the one-read fold and against the torch path.

Part b (``--out``): M rows of len floats at the aggregate shapes of BASELINE configs 2 (100 x 20,480), 3 (1,000 x
28,672), 4 (1,250 x 20,480) and 5 (1,000 x 163,840), each contiguous and as a 10 % sample (M / 10 gathered rows
of the same buffer); rows = x + 1e-3 N(0, 1), alpha = Dirichlet-like positive weights, T = 3, nu = 1e-6,
init = 'start'.  On the same buffer:
  the whole chain (fs_aggregate_rfa), one fused step (fs_rfa_step with the chain's last weights) and one
  fs_rfa_weights (the reduction of the partial table and the weights);
  (a) fs_aggregate_sel on the same rows and weights: one read of every row element, a fold;
  (b) the torch path on the same device, per iteration ``d = (W[sel] - v).norm(dim=1)``, the weights
      ``alpha / max(nu, d)`` (0 where d is not finite) normalised, and ``v = (b[:, None] * W[sel]).sum(0)``.
Before anything is timed the torch path's result is checked against tests/rfa_restatement.py at a small
shape (65 x 132, T = 3), and at every shape the chain's output against the torch path's.
The method of scripts/bench_krum.py: fs_timer_* events, 100 ms of the leg's own launches first, then per
repetition 5 warm-up and 20 timed launches back to back; three repetitions, the median reported with all
three.  ONE condition is asserted (exit status 1 otherwise): at every shape the chain's median time is at or
below leg (b)'s, the only margin leg (b)'s own (max - min) / median spread.  The step's share of the HBM
peak counts one read of the rows, 4 M len bytes.

Part c (``--round-out``): a whole round, ``FedRFA`` against ``FedAvg(clients='parallel')``, each measured twice
in turn, host-timed over 10 rounds after 3.  Nothing is asserted.

    python scripts/bench_rfa.py [--out profiles/rfa/bench.json] [--round-out profiles/rfa/round.json]
                                [--round-shapes 2,3,4] [--parts b,c]
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
from tests import rfa_restatement as RR  # noqa: E402

BASE = {'config2': dict(M=100, len=20480), 'config3': dict(M=1000, len=28672), 'config4': dict(M=1250, len=20480),
        'config5': dict(M=1000, len=163840)}
FOLD_SHAPES = {}
for _k, _v in BASE.items():
    FOLD_SHAPES[_k] = dict(M=_v['M'], of=_v['M'], len=_v['len'])
    FOLD_SHAPES[_k + '_tenth'] = dict(M=_v['M'] // 10, of=_v['M'], len=_v['len'])
ROUND_SHAPES = {'2': dict(clients=100, rows=512, D=2048, C=10), '3': dict(clients=1000, rows=465, D=4096, C=7),
                '4': dict(clients=1250, rows=64, D=2048, C=10)}
E, B, LR = 2, 32, 0.05
WARMUP, TIMED, REPS, SETTLE_MS = 5, 20, 3, 100
ROUNDS_WARM, ROUNDS_TIMED = 3, 10
T_ITERS, NU = 3, 1e-6
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


def torch_rfa(W, sel64, x, alpha, T, nu):
    """The torch path: T iterations from x."""
    v = x
    for _ in range(T):
        rows = W if sel64 is None else W[sel64]
        d = (rows - v).norm(dim=1)
        beta = torch.where(torch.isfinite(d), alpha / d.clamp_min(nu), torch.zeros_like(d))
        b = beta / beta.sum()
        rows = W if sel64 is None else W[sel64]
        v = (b[:, None] * rows).sum(0)
    return v


def check_torch_path(dev):
    """The torch path against the restatement at 65 x 132, T = 3: float32 sums in another order, so to
    len * 2^-24 of the rows' largest magnitude, not bit for bit."""
    W, x, alpha = RR.inputs('normal', 65, 132)
    ref = RR.chain(W, x, alpha, T_ITERS, NU, 'start')['out']
    got = torch_rfa(torch.from_numpy(W).to(dev), None, torch.from_numpy(x).to(dev), torch.from_numpy(alpha).to(dev),
                    T_ITERS, NU).cpu().numpy()
    err, tol = float(np.abs(got - ref).max()), 132 * 2.0 ** -24 * float(np.abs(W).max())
    assert err <= tol, ('the torch path is not the rule', err, tol)
    return err


def bench_fold(shape, dev):
    M, N, length = shape['M'], shape['of'], shape['len']
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(length, device=dev, generator=gen)
    W = x[None, :] + 1e-3 * torch.randn(N, length, device=dev, generator=gen)
    sel = None if M == N else torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(6))[:M])[0] \
        .to(torch.int32).to(dev)
    sel_all = torch.arange(M, dtype=torch.int32, device=dev) if sel is None else sel
    sel64 = None if sel is None else sel.to(torch.int64)
    alpha = torch.rand(M, device=dev, generator=gen) + 0.5
    alpha = (alpha / alpha.sum()).contiguous()
    out, out_a, v1 = torch.empty(length, device=dev), torch.empty(length, device=dev), torch.empty(length, device=dev)
    agg = engine.Aggregator(M, 1, length, dev)
    ws = agg.rfa_ws()
    dist = torch.zeros(M, dtype=torch.float64, device=dev)
    b = torch.zeros(M, device=dev)
    obj = torch.zeros(T_ITERS + 2, dtype=torch.float64, device=dev)
    stripes = -(-length // engine.rfa_width(M))
    part = torch.empty(stripes, M, dtype=torch.float64, device=dev)
    d2, dist1 = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    b1, obj1 = torch.empty(M, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    res = dict(M=M, of=N, len=length, T=T_ITERS, megabytes=4.0 * M * length / 2 ** 20, width=engine.rfa_width(M),
               stripes=stripes, ws_megabytes=ws.numel() / 2 ** 20)
    keep = {}

    def floor():
        agg.run_sel(W, sel_all, alpha, out_a, check=False)

    def chain():
        agg.run_rfa(W, x, alpha, T_ITERS, NU, 'start', out, dist, b, obj, ws, sel=sel, check=False)

    def one_step():
        engine.rfa_step(W, length, x, b, flag, v1, part, sel=sel, M=M)

    def weights():
        engine.rfa_weights(part, M, length, alpha, NU, d2, dist1, b1, obj1, flag)

    def torch_path():
        keep['out'] = torch_rfa(W, sel64, x, alpha, T_ITERS, NU)

    one = res
    chain()
    for name, fn in [('fs_aggregate_sel', floor), ('fs_aggregate_rfa', chain), ('fs_rfa_step', one_step),
                     ('fs_rfa_weights', weights), ('torch_path', torch_path), ('fs_aggregate_sel_again', floor)]:
        ms, reps = time_launches(fn)
        one[name] = entry(ms, reps)
        flag.zero_()
    chain()
    one['max_abs_diff_to_torch'] = float((out - keep['out']).abs().max())
    one['objective'] = [float(v) for v in obj.cpu()]
    one['step_over_floor'] = one['fs_rfa_step']['us'] / one['fs_aggregate_sel']['us']
    one['step_tb_per_s'] = 4.0 * M * length / (one['fs_rfa_step']['us'] * 1e-6) / 1e12
    one['step_fraction_of_hbm_peak'] = one['step_tb_per_s'] / PEAK_HBM_TBS
    one['floor_tb_per_s'] = 4.0 * M * length / (one['fs_aggregate_sel']['us'] * 1e-6) / 1e12
    one['weights_over_step'] = one['fs_rfa_weights']['us'] / one['fs_rfa_step']['us']
    one['torch_over_chain'] = one['torch_path']['us'] / one['fs_aggregate_rfa']['us']
    one['floor_session_spread'] = one['fs_aggregate_sel_again']['us'] / one['fs_aggregate_sel']['us']
    one['condition_met'] = bool(one['fs_aggregate_rfa']['us'] <= one['torch_path']['us'] * (1.0 + one['torch_path']['spread']))
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
    for algo in ('fedavg', 'fedrfa', 'fedavg_again', 'fedrfa_again'):
        torch.manual_seed(9)
        rf = algo.startswith('fedrfa')
        kw = dict(rfa=dict(iters=T_ITERS, nu=NU, init='start')) if rf else {}
        fed = tools.Federation('fedrfa' if rf else 'fedavg', Xs, ys, Xt, yt, None, 'classification', C, D, LR, E, B,
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
    res['fedrfa_over_fedavg'] = res['fedrfa']['ms_per_round'] / res['fedavg']['ms_per_round']
    res['fedrfa_over_fedavg_again'] = res['fedrfa_again']['ms_per_round'] / res['fedavg_again']['ms_per_round']
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
            'source_revision': {k: _lib.source_revision(k) for k in ('aggregate_rfa', 'aggregate_nova', 'local_train')}}
    ok = True
    if 'b' in parts:
        line = dict(head, metric='rfa_aggregate', warmup=WARMUP, timed=TIMED, reps=REPS, settle_ms=SETTLE_MS,
                    T=T_ITERS, nu=NU, peak_hbm_tb_per_s=PEAK_HBM_TBS, torch_path_max_abs_diff_to_restatement=
                    check_torch_path(dev), shapes={})
        for s in a.shapes.split(','):
            line['shapes'][s] = bench_fold(FOLD_SHAPES[s], dev)
            torch.cuda.empty_cache()
        line['condition_met'] = all(line['shapes'][s]['condition_met'] for s in line['shapes'])
        ok = line['condition_met']
        write(a.out, line)
    if 'c' in parts:
        line = dict(head, metric='rfa_round', E=E, B=B, T=T_ITERS, rounds_warm=ROUNDS_WARM, rounds_timed=ROUNDS_TIMED,
                    shapes={})
        for s in a.round_shapes.split(','):
            line['shapes']['config%s' % s] = bench_round(ROUND_SHAPES[s], dev)
            torch.cuda.empty_cache()
        write(a.round_out, line)
    if not ok:
        print('FAILED: fs_aggregate_rfa is not at or below the torch path at every shape', file=sys.stderr)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())

#!/usr/bin/env python3
"""Record which p-solver fs_mix_solve launches over a grid into tests/golden/mix_plan_table.npz.

    python tests/golden/make_mix_plan_table.py [--out FILE]        (on the MI355X)
    python tests/golden/make_mix_plan_table.py --compare           (record, compare with the table, write nothing)

It records by LAUNCHING: one p-SGD step (n_val = Bv, epochs = 1) at every grid point, then
fs_mix_solve_last_mode and fs_mix_solve_last_layout.  It uses nothing newer than those two
queries, so it runs on any commit -- the table in the repository was recorded on the commit
before the planner (csrc/mixture_host.cpp) existed, and tests/test_mix_plan_table.py holds
fs_mix_solve_plan to it on the CPU.  Regenerate it only with a change that means to move a
choice, and say so in that change.
Grid: one value on each side of every threshold of the solver table.  Legs: the default tuning,
mix_solver forced to each of the nine solvers, mix_qmc_lane_clients 4 and 8.
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, 'mix_plan_table.npz')
AXES = ('N', 'C', 'Bv')
GRID = dict(N=[1, 4, 10, 16, 17, 64, 65, 100, 128, 129, 256, 257, 300, 520, 1000, 1024, 1025, 2048, 2049, 4096],
            C=[1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 17, 24, 25],
            Bv=[1, 8, 16, 17, 32, 64])
SOLVERS = ('bin', 'wave', 'quad', 'reg2', 'reg', 'qmc', 'mc', 'staged', 'global')
LEGS = [{}] + [dict(mix_solver=s) for s in SOLVERS] + [dict(mix_qmc_lane_clients=4), dict(mix_qmc_lane_clients=8)]


def record(lib, grid, legs):
    """Per leg three arrays [len(N)][len(C)][len(Bv)]: the solver launched, and qmc's workgroups
    and clients per lane (0, 0 after any other solver)."""
    import ctypes

    import torch
    L = lib.lib()
    dev = torch.device('cuda')
    Nm, Cm, Bm = (max(grid[k]) for k in AXES)
    ldn = lambda n: (n + 3) // 4 * 4   # noqa: E731
    Z = (torch.randn(Bm * Cm * ldn(Nm), generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    labels = torch.zeros(Bm, dtype=torch.int32, device=dev)
    perms = torch.arange(Bm, dtype=torch.int32, device=dev)
    p, buf = torch.empty(Nm, device=dev), torch.empty(Nm, device=dev)
    first = torch.ones(1, dtype=torch.int32, device=dev)
    points = list(itertools.product(*(list(map(int, grid[k])) for k in AXES)))
    ws = torch.zeros(max(int(L.fs_mix_solve_ws_bytes(*pt)) for pt in points), dtype=torch.uint8, device=dev)
    k, nk = ctypes.c_int(0), ctypes.c_int(0)
    shape = tuple(len(grid[a]) for a in AXES)
    out = []
    for fields in legs:
        S, K, NK = (np.zeros(len(points), np.int32) for _ in range(3))
        with lib.tuning(**fields):
            for i, (N, C, Bv) in enumerate(points):
                p[:N] = 1.0 / N
                buf.zero_()
                first.fill_(1)
                ws.zero_()
                at = 'fs_mix_solve%r %r' % ((N, C, Bv), fields)
                lib.check(L.fs_mix_solve(lib.ptr(Z), lib.ptr(labels), lib.ptr(perms), N, C, Bv, 1, Bv, 0.1, 0.9,
                                         lib.ptr(p), lib.ptr(buf), lib.ptr(first), lib.ptr(ws),
                                         int(L.fs_mix_solve_ws_bytes(N, C, Bv)), lib.stream_ptr()), at)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(p[:N]).all()), at
                S[i] = L.fs_mix_solve_last_mode()
                lib.check(L.fs_mix_solve_last_layout(ctypes.byref(k), ctypes.byref(nk)), at)
                K[i], NK[i] = k.value, nk.value
        print('leg %r: %s' % (fields, {lib.SOLVER_NAMES[s]: int((S == s).sum()) for s in np.unique(S)}), flush=True)
        out.append(tuple(a.reshape(shape) for a in (S, K, NK)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=TABLE)
    ap.add_argument('--compare', action='store_true', help='record and compare with --out; write nothing')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from fedamw_amd import _lib
    _lib.lib()
    out = dict(tunings=np.array(json.dumps(LEGS)))
    out.update({a: np.array(GRID[a], np.int32) for a in AXES})
    for i, (S, K, NK) in enumerate(record(_lib, GRID, LEGS)):
        out['solver_%d' % i] = S.astype(np.int8)
        out['workgroups_%d' % i] = K.astype(np.int16)
        out['lane_clients_%d' % i] = NK.astype(np.int8)
    if args.compare:
        t = np.load(args.out)
        bad = [k for k in out if not np.array_equal(out[k], t[k])]
        print('differs from %s in: %s' % (args.out, bad) if bad else 'equal to %s' % args.out)
        sys.exit(1 if bad else 0)
    np.savez_compressed(args.out, **out)
    print('%s: %d launches, %d bytes' % (args.out, len(LEGS) * out['solver_0'].size, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()

"""The p-solve launch follows its plan: fs_mix_solve runs the solver and layout fs_mix_solve_plan
names (tests/test_mix_plan_table.py pins the plan itself, on the CPU), at the named shapes and at
three forced solvers that do not cover their shape and fall through.  One step pair each."""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import amd  # noqa: F401 (fixture)
from tests.test_mix_plan_table import BY_NAME

pytestmark = pytest.mark.gpu

CASES = [(shape, {}) for shape in sorted(BY_NAME)] + [
    ((300, 10, 16), dict(mix_solver='quad')),     # quad ends at N = 128
    ((100, 10, 16), dict(mix_solver='qmc')),      # qmc starts past N = 128
    ((10, 4, 16), dict(mix_solver='bin')),        # bin is the two-class solver
]


@pytest.mark.parametrize('shape,fields', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_mix_solve_follows_plan(amd, shape, fields):
    lib, L = amd.lib, amd.lib.lib()
    N, C, Bv = shape
    nv, ldN = 2 * Bv, (N + 3) // 4 * 4
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(N + C + Bv)
    Z = (torch.randn(nv, C * ldN, generator=g) * 0.1).to(dev)
    y = torch.randint(0, C, (nv,), generator=g).to(dtype=torch.int32, device=dev)
    perms = torch.randperm(nv, generator=g).to(dtype=torch.int32, device=dev)
    p0 = torch.full((N,), 1.0 / N, device=dev)
    p, buf = p0.clone(), torch.zeros(N, device=dev)
    first = torch.ones(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(int(L.fs_mix_solve_ws_bytes(N, C, Bv)), dtype=torch.uint8, device=dev)
    with lib.tuning(**fields):
        plan = lib.mix_plan(N, C, nv, 1, Bv)
        lib.check(L.fs_mix_solve(lib.ptr(Z), lib.ptr(y), lib.ptr(perms), N, C, nv, 1, Bv, 0.1, 0.9, lib.ptr(p),
                                 lib.ptr(buf), lib.ptr(first), lib.ptr(ws), ws.numel(), lib.stream_ptr()),
                  'fs_mix_solve')
        torch.cuda.synchronize()
    assert L.fs_mix_solve_last_mode() == plan['solver']
    assert lib.last_mix_layout() == (plan['workgroups'], plan['lane_clients'])
    if not fields:
        solver, layout = BY_NAME[shape]
        assert lib.SOLVER_NAMES[plan['solver']] == solver and lib.last_mix_layout() == (layout or (0, 0))
    else:
        assert lib.SOLVER_NAMES[plan['solver']] in ('staged', 'global')
    assert plan['ws_bytes'] <= ws.numel()
    assert int(ws[-lib.ERR_BLOCK:].view(torch.int32)[0]) == 0, 'exchange timeout'
    assert bool(torch.isfinite(p).all()) and not torch.equal(p, p0)
    assert int(first) == 0

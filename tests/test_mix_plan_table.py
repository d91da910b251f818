"""fs_mix_solve_plan pinned over a grid of shapes and tunings (CPU: the planner is host code).

Which p-solver a shape gets is a measured decision.  tests/golden/
mix_plan_table.npz (tests/golden/make_mix_plan_table.py) holds what fs_mix_solve LAUNCHED at
every grid point on the MI355X, recorded on the commit before the planner existed; this test
replays the grid through fs_mix_solve_plan and requires the solver and qmc's layout to be equal
at every point.  The benchmark shapes' solvers are asserted by name besides, so a regenerated
fixture cannot hide a moved choice.  tests/test_gpu_mix_plan.py checks that a launch follows
the plan.
"""
import itertools
import json
import os

import numpy as np
import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mix_plan_table.npz')
AXES = ('N', 'C', 'Bv')
# one value on each side of every threshold of the solver table: the fixture must hold this grid
GRID = dict(N=[1, 4, 10, 16, 17, 64, 65, 100, 128, 129, 256, 257, 300, 520, 1000, 1024, 1025, 2048, 2049, 4096],
            C=[1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 17, 24, 25],
            Bv=[1, 8, 16, 17, 32, 64])
SOLVERS = ('bin', 'wave', 'quad', 'reg2', 'reg', 'qmc', 'mc', 'staged', 'global')
LEGS = [{}] + [dict(mix_solver=s) for s in SOLVERS] + [dict(mix_qmc_lane_clients=4), dict(mix_qmc_lane_clients=8)]
FIELDS = ('solver', 'workgroups', 'lane_clients', 'ws_bytes')

# (N, C, Bv) under the default tuning: solver, and qmc's (K, NK)
BY_NAME = {
    (10, 2, 16): ('bin', None), (16, 4, 16): ('wave', None), (100, 10, 16): ('quad', None),
    (129, 4, 16): ('reg2', None), (129, 10, 16): ('mc', None), (300, 10, 16): ('qmc', (5, 4)),
    (1000, 10, 16): ('qmc', (16, 4)), (2000, 10, 16): ('qmc', (16, 8)), (2000, 16, 16): ('mc', None),
    (100, 24, 16): ('global', None),
    # two batches of 32 rows x 10 classes x 100 clients are 256 KB, past staged's 150 KB of LDS: the
    # launch recorded before the planner ran `global` here; (16, 2, 17) is a staged shape
    (100, 10, 32): ('global', None), (16, 2, 17): ('staged', None),
}


@pytest.fixture(scope='module')
def lib():
    from fedamw_amd import _lib
    _lib.lib()
    return _lib


def replay(lib, legs, blocks=1):
    """Per leg a dict of arrays [len(N)][len(C)][len(Bv)] of fs_mix_solve_plan's FIELDS at
    n_val = Bv, epochs = 1 (as the fixture was recorded)."""
    shape = tuple(len(GRID[a]) for a in AXES)
    points = list(itertools.product(*(GRID[a] for a in AXES)))
    out = []
    for fields in legs:
        with lib.tuning(**fields):
            plans = [lib.mix_plan(N, C, Bv, 1, Bv, blocks) for N, C, Bv in points]
        out.append({f: np.array([p[f] for p in plans], np.int64).reshape(shape) for f in FIELDS})
    return out


@pytest.fixture(scope='module')
def plans(lib):
    return replay(lib, LEGS)


def _first(bad, fields):
    b = tuple(bad[0])
    return dict(zip(AXES, (GRID[a][j] for a, j in zip(AXES, b))), **fields), b


def test_mix_plan_table(lib, plans):
    """Every recorded launch against the plan: same solver, same qmc workgroups and lane width."""
    t = np.load(TABLE)
    assert json.loads(str(t['tunings'])) == LEGS and all(t[a].tolist() == GRID[a] for a in AXES), \
        'the fixture must hold the whole grid and every leg'
    for i, (fields, got) in enumerate(zip(LEGS, plans)):
        for name in ('solver', 'workgroups', 'lane_clients'):
            ref = t['%s_%d' % (name, i)]
            bad = np.argwhere(got[name] != ref)
            if len(bad):
                at, b = _first(bad, fields)
                raise AssertionError('%s differs at %d points, first %r: planned %d, launched %d'
                                     % (name, len(bad), at, got[name][b], ref[b]))


@pytest.mark.parametrize('shape', sorted(BY_NAME))
def test_mix_plan_by_name(lib, shape):
    """The named shapes, from the planner and from the recorded table (2000 is not on the grid)."""
    solver, layout = BY_NAME[shape]
    N, C, Bv = shape
    p = lib.mix_plan(N, C, Bv, 1, Bv)
    assert lib.SOLVER_NAMES[p['solver']] == solver
    assert (p['workgroups'], p['lane_clients']) == (layout or (0, 0))
    if N in GRID['N']:
        t = np.load(TABLE)
        at = tuple(GRID[a].index(v) for a, v in zip(AXES, shape))
        assert lib.SOLVER_NAMES[int(t['solver_0'][at])] == solver
        assert (int(t['workgroups_0'][at]), int(t['lane_clients_0'][at])) == (layout or (0, 0))


def test_mix_plan_workspace_within_ws_bytes(lib, plans):
    """The workspace a plan uses never exceeds fs_mix_solve_ws_bytes, which knows no tuning."""
    L = lib.lib()
    ws = np.array([L.fs_mix_solve_ws_bytes(N, C, Bv) for N, C, Bv in itertools.product(*(GRID[a] for a in AXES))],
                  np.int64).reshape(plans[0]['ws_bytes'].shape)
    for fields, got in zip(LEGS, plans):
        bad = np.argwhere(got['ws_bytes'] > ws)
        assert not len(bad), 'plan.ws_bytes > fs_mix_solve_ws_bytes, first %r' % (_first(bad, fields)[0],)


def test_mix_plan_blocked(lib, plans):
    """fs_mix_solve_blocked_covers is "the plan with blocks > 1 is qmc", and where the blocked entry
    point accepts the shape (N a multiple of 4 * blocks, qmc) the plan is the one of blocks = 1."""
    L = lib.lib()
    qmc = lib.SOLVERS['qmc']
    points = list(itertools.product(*(GRID[a] for a in AXES)))
    for fields, one, two in zip(LEGS, plans, replay(lib, LEGS, blocks=2)):
        with lib.tuning(**fields):
            covers = np.array([L.fs_mix_solve_blocked_covers(N, C, Bv, 1, Bv) for N, C, Bv in points],
                              bool).reshape(one['solver'].shape)
        bad = np.argwhere(covers != (two['solver'] == qmc))
        assert not len(bad), 'fs_mix_solve_blocked_covers != (plan is qmc), first %r' % (_first(bad, fields)[0],)
        accepts = covers & (np.array(GRID['N'])[:, None, None] % 8 == 0)
        assert accepts.any() or fields.get('mix_solver', 'qmc') != 'qmc'
        for f in FIELDS:
            bad = np.argwhere(accepts & (one[f] != two[f]))
            assert not len(bad), '%s differs between blocks = 1 and 2, first %r' % (f, _first(bad, fields)[0])

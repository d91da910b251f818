"""fs_local_train_plan pinned over a grid of shapes, requests and tunings.

Which form and width every shape gets is a measured decision, and the workspace
size follows from it.  tests/golden/lt_plan_table.npz (tests/golden/make_plan_table.py) records
the planner's answer (G_out, ws_bytes) at every point of the grid on a 256-CU MI355X; this test
replays the grid and requires every answer to be equal.  The fixture is this project's own
output: it pins the planner's behaviour, it is no claim that each answer is the best one.  The
five benchmark configs' forms are asserted by name besides, so a regenerated fixture cannot hide
a changed choice.
"""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import amd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lt_plan_table.npz')
AXES = ('N', 'C', 'B', 'ld', 'chained', 'prox')


def replay(lib, axes, legs):
    """The planner's answers over ``axes`` (a dict of value lists, AXES order) for every leg
    ((tuning fields, requests)): per leg two arrays [len(N)]...[len(prox)][len(requests)], G_out
    and ws_bytes."""
    L = lib.lib()
    plan = L.fs_local_train_plan
    g, ws = ctypes.c_int(0), ctypes.c_int64(0)
    pg, pws = ctypes.byref(g), ctypes.byref(ws)
    shape = tuple(len(axes[k]) for k in AXES)
    points = list(itertools.product(*(list(map(int, axes[k])) for k in AXES)))
    out = []
    for fields, requests in legs:
        requests = list(map(int, requests))
        G = np.zeros((len(points), len(requests)), np.int32)
        W = np.zeros((len(points), len(requests)), np.int64)
        with lib.tuning(**fields):
            for i, (N, C, B, ld, chained, prox) in enumerate(points):
                for r, want in enumerate(requests):
                    g.value = want
                    if plan(N, C, B, 2, ld, 2 * 512, chained, prox, pg, pws) != 0:
                        lib.check(-1, 'fs_local_train_plan%r' % ((N, C, B, ld, chained, prox, want),))
                    G[i, r] = g.value
                    W[i, r] = ws.value
        out.append((G.reshape(shape + (len(requests),)), W.reshape(shape + (len(requests),))))
    return out


def _cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def test_plan_table(amd):
    """Every recorded answer, replayed: same device CU count (the groups in flight, and with them
    the pair / pipe choices and the workspace sizes, follow from it), same G_out, same ws_bytes."""
    t = np.load(TABLE)
    assert _cus() == int(t['cus']), 'the table was recorded on %d CUs' % int(t['cus'])
    axes = {k: t[k].tolist() for k in AXES}
    legs = [(fields, t['requests_%d' % i].tolist()) for i, fields in enumerate(json.loads(str(t['tunings'])))]
    for i, ((fields, requests), (G, W)) in enumerate(zip(legs, replay(amd.lib, axes, legs))):
        for name, got, ref in (('G_out', G, t['G_%d' % i]), ('ws_bytes', W, t['ws_%d' % i])):
            bad = np.argwhere(got != ref)
            if len(bad):
                b = tuple(bad[0])
                at = dict(zip(AXES, (axes[k][j] for k, j in zip(AXES, b))), request=requests[b[-1]], **fields)
                raise AssertionError('%s differs at %d points, first %r: %d, recorded %d'
                                     % (name, len(bad), at, got[b], ref[b]))


# the form each benchmark config's shape gets (E = 2, B = 32 throughout)
BENCH_FORMS = {
    'config 1: narrow split G = 8, chained': (dict(N=10, C=2, B=32, ld=2048, chained=1, prox=0), 8),
    'config 2: split G = 2': (dict(N=100, C=10, B=32, ld=2048, chained=0, prox=0), 2),
    'config 3: split G = 4 with prox': (dict(N=1000, C=7, B=32, ld=4096, chained=0, prox=1), 4),
    'config 4: pipe G = 2': (dict(N=1250, C=10, B=32, ld=2048, chained=0, prox=0), 2 | 1024),
    'config 5: split G = 16': (dict(N=1000, C=10, B=32, ld=16384, chained=0, prox=0), 16),
}


@pytest.mark.parametrize('name', sorted(BENCH_FORMS))
def test_plan_bench_configs(amd, name):
    """The benchmark configs by name, from the planner and from the recorded table."""
    shape, want = BENCH_FORMS[name]
    assert amd.lib.G_PIPE == 1024
    (G, W), = replay(amd.lib, {k: [v] for k, v in shape.items()}, [({}, [0])])
    assert int(G.item()) == want
    t = np.load(TABLE)
    assert t['requests_0'][0] == 0 and json.loads(str(t['tunings']))[0] == {}
    at = tuple(t[k].tolist().index(shape[k]) for k in AXES) + (0,)
    assert int(t['G_0'][at]) == want and int(t['ws_0'][at]) == int(W.item())

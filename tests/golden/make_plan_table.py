#!/usr/bin/env python3
"""Record fs_local_train_plan's answers over a grid into tests/golden/lt_plan_table.npz.

    python tests/golden/make_plan_table.py          (on the MI355X: the planner reads the CU count)

The fixture pins the planner's behaviour as it stands (tests/test_gpu_plan_table.py replays it);
regenerate it only with a change that means to move a choice, and say so in that change.
Legs: every request under the default tuning, then the automatic choice (request 0) under each
fs_tuning field the planner reads, and explicit pair / team requests under split_pipe = 1.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from fedamw_amd import _lib  # noqa: E402
from tests.test_gpu_plan_table import AXES, TABLE, _cus, replay  # noqa: E402

GRID = dict(N=[1, 2, 10, 100, 127, 128, 129, 1000, 1250],
            C=[1, 2, 7, 10, 14, 15, 16, 17],
            B=[1, 16, 17, 20, 32, 33],
            ld=[64, 128, 256, 512, 1024, 1088, 2048, 4096, 8192, 16384],
            chained=[0, 1], prox=[0, 1])
WIDTHS = [2, 4, 8, 16]
FORMS = [_lib.G_PAIR, _lib.G_TEAMS, _lib.G_PIPE]
LEGS = [({}, [0, 1, 2, 3, 4, 8, 16] + [g | f for f in FORMS for g in WIDTHS]),
        (dict(train_form=1), [0]), (dict(train_form=2), [0]),
        (dict(split_pipe=1), [0]), (dict(split_pipe=-1), [0]),
        (dict(split_teams=1), [0]),
        (dict(split_pipe=1), [g | f for f in (_lib.G_PAIR, _lib.G_TEAMS) for g in WIDTHS])]


def main():
    _lib.lib()
    out = dict(cus=np.int32(_cus()), tunings=np.array(json.dumps([f for f, _ in LEGS])))
    out.update({k: np.array(GRID[k], np.int64) for k in AXES})
    for i, ((_, requests), (G, W)) in enumerate(zip(LEGS, replay(_lib, GRID, LEGS))):
        out['requests_%d' % i] = np.array(requests, np.int32)
        out['G_%d' % i] = G.astype(np.int16)
        out['ws_%d' % i] = W
    np.savez_compressed(TABLE, **out)
    print('%s: %d CUs, %d answers, %d bytes' % (TABLE, out['cus'], sum(out['G_%d' % i].size for i in range(len(LEGS))),
                                                os.path.getsize(TABLE)))


if __name__ == '__main__':
    main()

"""The compiled schedule of config 2's split instance (csrc/local_train_split.hip, SP_BWD_FENCE).

hipcc used to sink the last four in-backward row loads of local_train_split_kernel<2,2,false,4,1,8,2,0>
behind the tile's last MFMAs (issued after backward MFMA 61-63 instead of 36-48) and to put the
rows on the dead gradient accumulators.  scripts/lt_issue_points.py reads the issue points out of
the built library; here every in-backward row load must issue within one backward iteration
(4 MFMAs) of the point the source gives it, and the instance must hold no VGPR spill.
Needs no GPU; skips without llvm-objdump or a built library.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import lt_issue_points as tool  # noqa: E402

SRC = os.path.join(tool.PKG, 'csrc', 'local_train_split.hip')
LIB = os.path.join(tool.PKG, 'libfedsim.so')


def _default(name):
    """the shipped value of a build macro of local_train_split.hip (#ifndef NAME / #define NAME v)"""
    m = re.search(r'#ifndef %s\s*\n#define %s (\d+)' % (name, name), open(SRC).read())
    assert m, name
    return int(m.group(1))


@pytest.fixture(scope='module')
def listing():
    if not tool.tool('llvm-objdump') or not tool.tool('llvm-readelf'):
        pytest.skip('llvm-objdump / llvm-readelf not found')
    if not os.path.exists(LIB):
        pytest.skip('libfedsim.so is not built')
    inst = '2, 2, false, %d, 1, 8, 2, 0' % _default('SP_EG2')
    rate = '%d/%d' % (_default('SP_BWD_NUM'), _default('SP_BWD_DEN'))
    tail = '%d/%d' % (_default('SP_BWD_TAIL'), _default('SP_BWD_TAILPER'))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'lt_issue_points.py'), inst,
                          '--lib', LIB, '--rate', rate, '--tail', tail], check=True, capture_output=True, text=True).stdout
    print(out)
    return out


def test_config2_row_loads_issue_at_their_source_points(listing):
    loads = re.findall(r'^load +\d+ +issued after backward MFMA +(\d+), source after +(\d+)', listing, re.M)
    nld = 16 - _default('SP_EG2')                  # 16 row loads per wave and step, the early ones ahead of S3
    assert len(loads) == nld, listing
    for k, (at, src) in enumerate(loads):
        assert abs(int(at) - int(src)) <= 4, (k, at, src)
    assert int(loads[-1][0]) <= 64, loads            # all of them inside the backward's 64 MFMAs


def test_config2_instance_has_no_vgpr_spill(listing):
    m = re.search(r'^spill +VGPR spill count (\d+)', listing, re.M)
    assert m, listing
    assert int(m.group(1)) == 0

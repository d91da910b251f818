"""The compiled hand-off chain of config 2's split instance (csrc/local_train_split.hip, round 12).

A step of local_train_split_kernel<2,2,false,4,1,8,2,0> is serial -- forward, S1, publish, poll, S2,
softmax, S3, backward -- and everything from the publish to S3 runs with the MFMA pipe idle, so an
instruction cut from that chain is a cycle cut from the step.  Round 12 removed the work there that
the result never needed; scripts/split_chain_isa.py counts what the built library holds, and the
counts must stay below the parent's (a3928a8: 498 instructions from S1 to S3, 56 of them
v_readlane_b32 restores of spilled SGPRs; 2 integer divisions per step; 2 IEEE divisions in the
softmax; 2 publish stores and 4 sc1 loads per poll; 77 spilled SGPRs, 32 bytes of scratch per lane).
Needs no GPU; skips without llvm-objdump or a built library.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import lt_issue_points as tool  # noqa: E402
import split_chain_isa as isa  # noqa: E402

LIB = os.path.join(tool.PKG, 'libfedsim.so')
INSTANCE = '2, 2, false, 4, 1, 8, 2, 0'
PARENT = dict(s1_s3=498, s1_s3_readlane=56, sgpr_spill=77, scratch=32)


@pytest.fixture(scope='module')
def counts():
    if not tool.tool('llvm-objdump') or not tool.tool('llvm-readelf'):
        pytest.skip('llvm-objdump / llvm-readelf not found')
    if not os.path.exists(LIB):
        pytest.skip('libfedsim.so is not built')
    sym = tool.mangled(tool.parse_args_str(INSTANCE))
    listing, meta = tool.disassemble(LIB, sym)
    c = isa.counts(listing, meta, sym)
    print(c)
    return c


def test_no_integer_division_in_the_step_loop(counts):
    """(epoch, batch) are carried as counters: no v_rcp_iflag_f32 sequence per step (the parent: 2)"""
    assert counts['loop_rcp_iflag'] == 0


def test_no_ieee_division_in_the_softmax(counts):
    """1 / batch rows is taken at the client's start: no v_div_scale_f32 between S2 and S3 (the parent: 2)"""
    assert counts['s2_s3_div_scale'] == 0


def test_one_exchange_slot(counts):
    """C <= 15: one sc1 publish store, and G = 2 sc1 loads per poll (the first poll and the re-poll
    of the spin loop); the parent compiled 2 and 4"""
    assert counts['publish_stores'] == 1
    assert counts['poll_loads'] == [2, 2]


def test_chain_is_shorter_than_the_parents(counts):
    assert counts['s1_s3'] < PARENT['s1_s3']
    assert counts['s1_s3_readlane'] < PARENT['s1_s3_readlane']


def test_no_more_spills_than_the_parent(counts):
    assert counts['vgpr_spill'] == 0
    assert counts['scratch'] <= PARENT['scratch']
    assert counts['sgpr_spill'] <= PARENT['sgpr_spill']

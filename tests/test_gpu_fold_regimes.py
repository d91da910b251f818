"""Every weighted aggregate, in every regime, bit for bit against tests/fold_restatement.py: the
sub-ranges of the one-launch form, the chunks of the two-stage form and its stage-2 tree restated in
numpy float32 with each rule's term and finish.  (The per-rule tests pin the left-fold regime bitwise
and hold the other regimes to a summation bound; this one pins the order of every regime.)

Rules: fs_aggregate / fs_aggregate_sel, fs_aggregate_nova modes 1 and 2, fs_aggregate_opt through its
AVGM probe (m' = delta) and with ADAM's step, fs_aggregate_scaffold's W_g and c.

Shapes: tests/test_gpu_aggregate_nova.py's, and at len in {4, 192}
  M = 17            two unequal sub-ranges, 9 + 8
  M = 100           16 sub-ranges of 7, the last holding 4 rows
  M = 200 (len 4)   32 sub-ranges of 7, 29..31 empty: the in-order fold stops at s * per < M
  M = 30, 12 chunks 10 chunks of 3: more partials than the tree has threads per position, its strided half
each on rows 0..M-1 and gathered from a 2M-row buffer whose other rows hold NaN."""
import numpy as np
import pytest
import torch

from tests import fedopt_restatement as FO
from tests import fold_restatement as FD
from tests.test_gpu_aggregate_nova import S0, SHAPES as NOVA_SHAPES, TE, case, plain
from tests.test_gpu_aggregate_nova import run as run_nova
from tests.test_gpu_aggregate_opt import PROBE, SC, run_opt
from tests.test_gpu_aggregate_scaffold import CS, coef
from tests.test_gpu_aggregate_scaffold import run as run_scaffold

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = NOVA_SHAPES + [(M, L, 0) for M in (17, 100) for L in (4, 192)] + [(200, 4, 0)] + [(30, L, 12) for L in (4, 192)]


@pytest.fixture(scope='module')
def amd():
    import fedamw_amd  # noqa: F401
    from fedamw_amd import _lib, engine
    _lib.lib()
    return type('amd', (), dict(lib=_lib, engine=engine, dev=torch.device('cuda')))


def ws_partials(M, sets=1):
    """Partials engine.Aggregator's workspace holds at M clients, for a rule keeping ``sets`` per chunk."""
    return max(1, min(64, M)) // sets


def same(got, ref, what):
    bad = np.flatnonzero(got != ref)
    assert np.isfinite(ref).all() and got.tobytes() == ref.tobytes(), (what, len(bad), got[bad[:4]], ref[bad[:4]])


def test_the_shapes_reach_every_regime_and_no_workspace_clamps():
    for M, L, chunks in SHAPES:
        if not FD.one_launch(M, chunks):
            want = FD.aggregate_chunks(M, chunks, M)
            assert FD.aggregate_chunks(M, chunks, ws_partials(M)) == want
            assert FD.aggregate_chunks(M, chunks, ws_partials(M, 2)) == want
    subs = {FD.one_launch_sub(M) for M, L, chunks in SHAPES if FD.one_launch(M, chunks)}
    assert subs == {1, 2, 8, 16, 32}
    assert -(-17 // 2) == 9 and -(-100 // 16) == 7 and 15 * 7 > 100 > 14 * 7 and 29 * 7 >= 200 > 28 * 7
    assert FD.aggregate_chunks(30, 12, ws_partials(30, 2)) == (10, 3) and 10 > FD.FP_SUB
    assert FD.aggregate_chunks(513, 0, ws_partials(513, 2)) == (8, 65)
    assert FD.aggregate_chunks(20, 3, ws_partials(20, 2)) == (3, 7)


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_plain_and_sel(amd, M, L, chunks):
    for gathered in (False, True):
        cs = case(M, L, gathered)
        rows, q = cs['rows'], cs['q']
        ref = FD.fold(M, chunks, ws_partials(M), lambda k, first: q[k] * rows[k])
        same(plain(amd, cs, chunks), ref, gathered)


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_nova(amd, M, L, chunks):
    te, s0 = F32(TE), F32(S0)
    for gathered in (False, True):
        cs = case(M, L, gathered)
        rows, q, b, base = cs['rows'], cs['q'], cs['b'], cs['base']
        ref1 = FD.fold(M, chunks, ws_partials(M),
                       lambda k, first: rows[k] * s0 if first else ((q[k] * rows[k]) * te) / b[k])
        same(run_nova(amd, cs, chunks, 1), ref1, (gathered, 1))
        ref2 = FD.fold(M, chunks, ws_partials(M), lambda k, first: q[k] * (rows[k] - base), lambda t: base + t)
        same(run_nova(amd, cs, chunks, 2), ref2, (gathered, 2))
        same(run_nova(amd, cs, chunks, 2, in_place=True), ref2, (gathered, 'in place'))


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_opt(amd, M, L, chunks):
    for gathered in (False, True):
        cs = case(M, L, gathered)
        rows, q, x = cs['rows'], cs['q'], cs['base']
        rs = np.random.RandomState(M + L)
        m = (0.1 * rs.normal(size=L)).astype(F32)
        v = rs.uniform(0.5, 2.0, size=L).astype(F32)
        for rule, sc, m0, v0 in (('avgm', PROBE, np.full(L, 3.0, F32), None), ('adam', SC, m, v)):
            ref = FD.fold(M, chunks, ws_partials(M), lambda k, first: q[k] * (rows[k] - x),
                          lambda d: FO.finish(rule, d, x, m0, v0, sc))
            got = run_opt(amd, cs, chunks, rule, sc, x, m0, v0)
            same(got[0], ref[0], (gathered, rule, 'x'))
            same(got[1], ref[1], (gathered, rule, 'm'))
            if v0 is not None:
                same(got[2], ref[2], (gathered, rule, 'v'))


@pytest.mark.parametrize('M,L,chunks', SHAPES)
def test_scaffold(amd, M, L, chunks):
    cs_ = F32(CS)
    for gathered in (False, True):
        cs = case(M, L, gathered)
        rows, q, x = cs['rows'], cs['q'], cs['base']
        r, c0 = coef(cs)
        ref = FD.fold(M, chunks, ws_partials(M, 2),
                      lambda k, first: np.stack([q[k] * (rows[k] - x), r[k] * (x - rows[k])]),
                      lambda t: (x + t[0], cs_ * c0 + t[1]))
        Wg, c = run_scaffold(amd, cs, chunks, r, c0)
        same(Wg, ref[0], (gathered, 'W_g'))
        same(c, ref[1], (gathered, 'c'))

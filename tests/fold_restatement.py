"""CPU restatement of the regimes of the weighted aggregates (csrc/aggregate_fold.h, aggregate_geom.h):
which ranges of k = 0..M-1 are folded on their own and in which order their partial sums are added,
in numpy float32, so that a kernel's output can be held to it bit for bit in every regime.

  one-launch form (chunks <= 0 and M <= ONE_MAX_N): SUB = one_launch_sub(M) consecutive sub-ranges of
      per = ceil(M / SUB) terms; the partials of the non-empty ones (s * per < M) added in order.
  two-stage form: aggregate_chunks(M, chunks, workspace) consecutive chunks; one chunk is the result,
      else the fixed tree -- thread s < FP_SUB adds the partials s, s + FP_SUB, ... in order, then
      those sums are added in order.

Everywhere the first term of a range is the term itself (not 0 + term), and every sum is rounded to
float32.  The rule is a ``term(k, first_of_fold)`` function (first_of_fold: k == 0, which FedNova's
reference form scales on its own) returning a float32 array -- two stacked rows for a rule with two
accumulators -- and a ``finish`` applied once to the folded total.
"""
import numpy as np

F32 = np.float32
ONE_MAX_N = 512     # AG_ONE_MAX_N
FP_SUB = 8          # AG_FP_SUB


def one_launch_sub(N):
    """Sub-ranges per position of the one-launch form: 1 below 16 terms, else the largest power of
    two <= min(32, N // 6)."""
    if N < 16:
        return 1
    s = 1
    while s * 2 <= 32 and s * 2 <= N // 6:
        s *= 2
    return s


def aggregate_chunks(N, chunks, ws_partials):
    """(chunks, per) of the two-stage form.  ``ws_partials``: how many partials the workspace holds
    (floats // len; for a rule with two partial sets, of half the floats), None without a workspace."""
    if chunks <= 0:
        chunks = max(1, min(8, N // 8))
    chunks = min(chunks, N)
    if chunks > 1:
        chunks = 1 if ws_partials is None else min(chunks, ws_partials)
    chunks = max(chunks, 1)
    per = -(-N // chunks)
    return -(-N // per), per


def one_launch(M, chunks):
    return chunks <= 0 and M <= ONE_MAX_N


def left(vals):
    """The in-order float32 sum whose first term is the term itself."""
    acc = None
    for v in vals:
        v = np.asarray(v, F32)
        acc = v if acc is None else (acc + v).astype(F32)
    return acc


def fold(M, chunks, ws_partials, term, finish=lambda t: t):
    """finish(the sum of term(k, k == 0), k = 0..M-1) as the kernels of every regime order it."""
    def part(k0, k1):
        return left(term(k, k == 0) for k in range(k0, k1))
    if one_launch(M, chunks):
        per = -(-M // one_launch_sub(M))
        return finish(left(part(k0, min(M, k0 + per)) for k0 in range(0, M, per)))
    K, per = aggregate_chunks(M, chunks, ws_partials)
    parts = [part(c * per, min(M, c * per + per)) for c in range(K)]
    if K == 1:
        return finish(parts[0])
    return finish(left(left(parts[s::FP_SUB]) for s in range(min(FP_SUB, K))))

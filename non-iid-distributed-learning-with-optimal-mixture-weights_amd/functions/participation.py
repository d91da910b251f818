"""Partial client participation: which clients train in which round (host only, no GPU).

``make_schedule(N, R, participation, sample_seed)`` returns R sorted int64 arrays of client ids:

* a float ``participation`` in (0, 1] samples ``M = max(1, floor(participation * N + 0.5))``
  clients per round (McMahan's C), an int in [1, N] is M itself.  The sampler is a private
  ``torch.Generator`` seeded with ``sample_seed``; round t takes
  ``sorted(torch.randperm(N, generator=g)[:M])``, one ``randperm`` per round in round order.  It
  never touches torch's global generator, which the shuffles of the run consume.
* a sequence of R id arrays is an explicit schedule (M may differ per round); ids must be
  distinct, in [0, N) and every round non-empty, else ``ValueError``.
"""
import math
import numbers

import numpy as np
import torch

__all__ = ['make_schedule', 'sample_size']


def sample_size(N, participation):
    """M of a float fraction in (0, 1] or an int count in [1, N]."""
    N = int(N)
    if isinstance(participation, bool):
        raise ValueError('participation must be a fraction in (0, 1], a count in [1, N] or a schedule')
    if isinstance(participation, numbers.Integral):
        M = int(participation)
        if not 1 <= M <= N:
            raise ValueError('participation=%d clients per round must be in [1, %d]' % (M, N))
        return M
    f = float(participation)
    if not (0.0 < f <= 1.0):
        raise ValueError('participation=%r must be a fraction in (0, 1]' % (participation,))
    return min(N, max(1, int(math.floor(f * N + 0.5))))


def _explicit(N, R, rounds):
    rounds = list(rounds)
    if len(rounds) != R:
        raise ValueError('an explicit participation schedule needs one id array per round (%d), got %d'
                         % (R, len(rounds)))
    out = []
    for t, ids in enumerate(rounds):
        a = np.asarray(ids)
        if a.ndim != 1 or a.size == 0:
            raise ValueError('round %d of the participation schedule must be a non-empty 1-D array of client ids' % t)
        if a.dtype.kind not in 'iu':
            raise ValueError('round %d of the participation schedule: client ids must be integers' % t)
        a = np.sort(a.astype(np.int64))
        if a[0] < 0 or a[-1] >= N:
            raise ValueError('round %d of the participation schedule: client ids must lie in [0, %d)' % (t, N))
        if a.size > 1 and bool(np.any(a[1:] == a[:-1])):
            raise ValueError('round %d of the participation schedule names a client twice' % t)
        out.append(a)
    return out


def make_schedule(N, R, participation, sample_seed=0):
    """The sampled clients of each of R rounds over N clients: a list of R sorted int64 arrays."""
    N, R = int(N), int(R)
    if N < 1 or R < 0:
        raise ValueError('make_schedule needs N >= 1 and R >= 0')
    if participation is None:
        raise ValueError('participation is None (every client trains): there is no schedule to make')
    if not isinstance(participation, (numbers.Real, str)) and hasattr(participation, '__len__'):
        return _explicit(N, R, participation)
    M = sample_size(N, participation)
    g = torch.Generator()
    g.manual_seed(int(sample_seed))
    return [np.sort(torch.randperm(N, generator=g)[:M].numpy().astype(np.int64)) for _ in range(R)]

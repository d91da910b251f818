"""The exact-arithmetic and mixed-row cases of the wide form of fs_local_train (batch sizes above
64; tests/test_gpu_bigbatch.py), built from tests/softmax_reference.py's ``train_problem``, and
shared with the CPU tests that prove them (tests/test_bigbatch_oracle.py): a saturated case is
admitted only while every row keeps a lead of GAP_EXACT over all steps, a mixed case only where
the fp32 oracle stays within a quarter of the bound the GPU test asserts."""
import numpy as np

from tests import softmax_reference as R

# (D, C, B): clients of exactly one batch (two and four 64-row blocks), class tiles of 16 and 32,
# weights in LDS and (D = 4000) in global memory
SAT_CASES = [(64, 2, 128), (200, 10, 128), (200, 10, 256), (130, 17, 256), (64, 26, 128), (4000, 10, 128)]
# (D, C, B, lr, prox and ridge on): batches of two 64-row blocks, tails of 1, 7 and B - 3 rows.
# (200, 10, 128) at lr = 2^-6 has the fp32 oracle at 0.44 of the bound on chained clients (the
# offset column trains at the edge of stability, as softmax_reference.MIXED_TRAIN_LR notes): 2^-7
MIXED_CASES = [(200, 10, 128, 2.0 ** -7, False), (130, 17, 128, 2.0 ** -6, True)]
ALL_WON_CLIENT = R.ALL_WON_CLIENT


def _seed(D, C, B, kind):
    return R.train_case_seed('wide', 1, D, C, B, kind)


def saturated_inputs(D, C, B):
    """(Xs, ys, W0): four clients of exactly one batch each, the third one 'all_won'."""
    rs = np.random.RandomState(_seed(D, C, B, 'saturated'))
    Xs, ys, W0 = R.train_problem(rs, [B] * 4, D, C, 'saturated')
    Xa, ya, _ = R.train_problem(rs, [B], D, C, 'all_won')
    Xs[ALL_WON_CLIENT], ys[ALL_WON_CLIENT] = Xa[0], ya[0]
    return Xs, ys, W0


def saturated_args(B):
    return (R.LR_SAT, 2, B, False, 0.0, False, 0.0)


def mixed_sizes(B):
    return [B + 1, B + 7, 2 * B - 3, B - 3]


def mixed_inputs(D, C, B):
    rs = np.random.RandomState(_seed(D, C, B, 'mixed'))
    return R.train_problem(rs, mixed_sizes(B), D, C, 'mixed')


def mixed_args(B, lr, on):
    return (lr, 2, B, on, R.MU, on, R.LAM)

"""A plain float64 reference of the test evaluation (fs_eval, the fused evaluation blocks) and
inputs on which the kernel's logits carry no rounding error at all.

``ce_acc_ref``     per-row cross-entropy, mean loss and correct count in float64.
``exact_problem``  features and weights that are small integers times a power of two: every
                   product and every partial sum of a logit is a small integer times one fixed
                   power of two, far below 2^24 of them, so fp32 gives the same logits in ANY
                   summation order (MFMA tiles, wave split, LDS partial sums).  What is left of
                   the kernel's error is its softmax arithmetic alone (``loss_bound``), and its
                   arg-max has no excuse: accuracy is compared exactly, ties included.
``SWEEP_*``        the structural sweep of tests/test_gpu_eval.py, shared with the CPU tests
                   that check the sweep itself (tests/test_eval_reference.py).
"""
import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff (half an ulp, relative)

# the boundaries of eval_group16's tile loop at 8 waves (T0 = w, T1 = T0 + 8, stride 16): one
# tile; one per wave; the second tile for wave 0 only; all second tiles; a second trip
SWEEP_TILES = (1, 2, 8, 9, 16, 17, 24, 25, 33)
SWEEP_ROWS = (1, 15, 16, 17, 33)                 # 16 rows per workgroup: ragged / full last group
SWEEP_CLASSES = (1, 2, 15, 16, 17, 31, 32)       # eval_kernel<1> up to 16 classes, <2> above
BIG_N, BIG_LD, BIG_C = 4113, 64, (10, 17)        # 258 workgroups: the finaliser's second stride


def sweep_cases(tiles):
    """The (n, D, ld, C) of one tile count: every row count with every class count, D = ld on
    one half and ld - 37 (a ragged last tile, zero padding read) on the other, so that each row
    count and each class count meets both."""
    ld = 64 * tiles
    return [(n, ld if (i + j) % 2 == 0 else ld - 37, ld, C)
            for i, n in enumerate(SWEEP_ROWS) for j, C in enumerate(SWEEP_CLASSES)]


def case_seed(n, D, ld, C):
    return (n * 1000003 + D * 1009 + C) % (2 ** 31 - 1)


def ce_acc_ref(X, y, W):
    """float64 reference of one evaluation: (ce per row, mean loss, correct count).  Logits
    X W^T in float64, cross-entropy as log-sum-exp with the maximum subtracted, arg-max by
    np.argmax (the first maximum: ties go to the lowest class index)."""
    z = np.asarray(X, np.float64) @ np.asarray(W, np.float64).T
    y = np.asarray(y).astype(np.int64)
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    ce = lse - z[np.arange(len(y)), y]
    correct = int((np.argmax(z, axis=1) == y).sum())
    return ce, float(ce.mean()), correct


def tied_rows(z, y):
    """Rows of the logits z whose maximum is attained more than once: (count, of those the rows
    labelled with the lowest tied class, of those the rows labelled with the highest)."""
    m = z.max(axis=1, keepdims=True)
    hit = z == m
    tied = hit.sum(axis=1) > 1
    lo = np.argmax(hit, axis=1)
    hi = z.shape[1] - 1 - np.argmax(hit[:, ::-1], axis=1)
    y = np.asarray(y)
    return int(tied.sum()), int((tied & (y == lo)).sum()), int((tied & (y == hi)).sum())


def exact_problem(rs, n, D, C, spread=20.0):
    """(X [n, D], y [n], W [C, D], info): fp32 inputs whose logits are exact in fp32 in any
    summation order.  Entries are integers in [-3, 3] times a power of two (X about unit row
    norm, W taking the rest of the scale), the scale such that the logits' standard deviation
    4 sqrt(D) quanta is about spread / 3.  Every partial sum of a logit is at most 9 D + 1300
    quanta (D <= 4160 here): far below 2^24.

    Every fourth row (1, 5, 9, ..., never the last) is then given an exact tie of its two largest
    logits (of its largest and one of the next three), by moving one feature where the other's
    weight is one off the leader's, such that no third class passes the pair: the labels of these rows go lower, higher, lower of the tied
    pair in turn -- never as many on the higher as on the lower, so a kernel that takes the last
    maximum gets another correct COUNT, the one figure fs_eval reports.
    Labels include 0 (row 0) and C - 1 (the last row) whenever n >= 2.

    info: 'tied' rows with a tied maximum, 'tied_low' / 'tied_high' those labelled with the
    lowest / highest tied class, 'quantum' the logits' unit."""
    Xi = rs.randint(-3, 4, size=(n, D)).astype(np.int64)
    Wi = rs.randint(-3, 4, size=(C, D)).astype(np.int64)
    y = rs.randint(0, C, size=n).astype(np.int64)
    y[0] = 0
    if n >= 2:
        y[-1] = C - 1
    flip = 0
    for i in range(1, n - 1, 4):
        if C < 2:
            break
        z = Wi @ Xi[i]
        order = np.argsort(-z, kind='stable')
        a = int(order[0])
        # a feature where a runner-up's weight is one above (below) the leader's, moved up (down)
        # by their gap, closes it; kept if no third class passes the pair
        moves = ((int(b), d) for b in order[1:4] if z[a] - z[b] <= 400
                 for d in np.nonzero(np.abs(Wi[b] - Wi[a]) == 1)[0])
        for b, d in moves:
            x = Xi[i].copy()
            x[d] += int(z[a] - z[b]) * (Wi[b, d] - Wi[a, d])
            z2 = Wi @ x
            if z2[a] == z2[b] == z2.max():
                Xi[i] = x
                y[i] = max(a, b) if flip % 3 == 1 else min(a, b)
                flip += 1
                break
    k = int(np.round(np.log2(4.0 * np.sqrt(D) / (spread / 3.0))))
    kx = int(np.round(np.log2(2.0 * np.sqrt(D))))
    X = (Xi * 2.0 ** -kx).astype(np.float32)
    W = (Wi * 2.0 ** -(k - kx)).astype(np.float32)
    zi = Xi @ Wi.T
    assert np.abs(zi).max() < 2 ** 20
    t, tl, th = tied_rows(zi, y)
    return X, y, W, dict(tied=t, tied_low=tl, tied_high=th, quantum=2.0 ** -k)


def kernel_formula_f32(z, y):
    """eval_rows.h's per-row arithmetic in numpy float32 on given fp32 logits:
    -(z_y - m - log(sum_c exp(z_c - m))), the sum over the classes in order."""
    z = np.asarray(z, np.float32)
    m = z.max(axis=1)
    se = np.zeros(len(z), np.float32)
    for c in range(z.shape[1]):
        se = (se + np.exp(z[:, c] - m)).astype(np.float32)
    zy = z[np.arange(len(z)), np.asarray(y)]
    return (-((zy - m).astype(np.float32) - np.log(se))).astype(np.float32).astype(np.float64)


def loss_bound(C, ce_rows):
    """|kernel loss - float64 loss| on exact logits: the mean over the rows of
    2^-23 (C + 8) max(1, ce_row).

    Derivation (u = 2^-24; expf and logf accurate to k ulp, i.e. 2 k u relative).  The logits are
    exact, so the maximum m and the differences z_c - m are exact.  Each exp(z_c - m) carries
    2 k u relative; the C positive terms are summed in order, C - 1 roundings, so the sum s is
    off by at most (2 k + C - 1) u relative, and so is log s in absolute terms.  logf adds
    2 k u |log s|, and 0 <= log s <= ce (ce = log s - (z_y - m) with z_y <= m).  z_y - m is
    exact; the last subtraction rounds once, u ce.  Together
        (2 k + C - 1) u + 2 k u ce + u ce  <=  (C + 4 k) u max(1, ce).
    The fp64 sum of the rows and the division add parts in 2^-53.  2^-23 (C + 8) = (2 C + 16) u
    is that bound for every k <= 4: the device's expf / logf are documented at 1 ulp, numpy's
    float32 loops (which the CPU test of this bound runs) at under 4, so one constant serves
    both and it is the one the derivation gives at k = 4."""
    ce_rows = np.asarray(ce_rows, np.float64)
    return float(np.mean(2.0 ** -23 * (C + 8) * np.maximum(1.0, ce_rows)))


def dot_bound_rows(X, W):
    """Per row, 2 (D + 7) u max_c sum_d |x_d w_cd|: twice the worst error of an fp32 dot product
    of D terms in any summation order (D - 1 additions, the products' roundings, the partial
    sums of 8 waves), which is both what a row's cross-entropy can move by (log-sum-exp and z_y
    each follow the logits 1 : 1) and the gap below which two logits can change order."""
    A = np.abs(np.asarray(X, np.float64)) @ np.abs(np.asarray(W, np.float64)).T
    return 2.0 * (X.shape[1] + 7) * U * A.max(axis=1)

"""fs_aggregate_robust restated in numpy: the rule of include/fedsim.h -- the total order on the bits,
the kept ranks b+1 .. M-b, and the kernel's order of the float64 summation -- so that the GPU result
can be compared bit for bit (NaN as NaN: a NaN's payload is not part of the rule).

The selection itself is a sort here; which algorithm finds the two thresholds cannot matter, since
the kept multiset is fixed by the order.  What has to be reproduced is the sum: T = 256 / width(M)
slices, slice s holding 0.0 plus the values strictly between the thresholds at k = s, s + T, ... in
ascending k, the slices joined by the pairwise tree, then the two tie terms count * value."""
import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32

MAX_M32, MAX_M16, MAX_M = 1261, 2523, 5047   # the last M of each stripe width; fs_aggregate_robust_max_m()


def width(M):
    """Columns of a workgroup's stripe at M rows."""
    return 32 if M <= MAX_M32 else 16 if M <= MAX_M16 else 8


def keys(W):
    """The monotone 32-bit key of every float's bits."""
    bits = np.ascontiguousarray(W, dtype=F32).view(U32)
    return np.where(bits >> 31, ~bits, bits | U32(0x80000000)).astype(U32)


def values(K):
    """The floats of keys."""
    K = np.asarray(K, dtype=U32)
    return np.where(K >> 31, K & U32(0x7FFFFFFF), ~K).astype(U32).view(F32)


def thresholds(W, b):
    """Per column: the keys at ranks b+1 and M-b, and the kept copies of each (clo, chi)."""
    K = keys(W)
    M = K.shape[0]
    Ks = np.sort(K, axis=0)
    klo, khi = Ks[b], Ks[M - b - 1]
    n = M - 2 * b
    below_lo, eq_lo, below_hi = (K < klo).sum(0), (K == klo).sum(0), (K < khi).sum(0)
    same = klo == khi
    clo = np.where(same, n, below_lo + eq_lo - b)
    chi = np.where(same, 0, (M - b) - below_hi)
    return K, klo, khi, clo, chi


def robust(W, b):
    """fs_aggregate_robust on the rows W [M, len] float32 with trim count b: float32 [len]."""
    W = np.ascontiguousarray(W, dtype=F32)
    M = W.shape[0]
    assert M >= 1 and 0 <= 2 * b < M and M <= MAX_M
    n = M - 2 * b
    T = 256 // width(M)
    K, klo, khi, clo, chi = thresholds(W, b)
    lo, hi = values(klo).astype(F64), values(khi).astype(F64)
    with np.errstate(all='ignore'):
        tlo = clo.astype(F64) * lo
        if n > 2:
            inside = (K > klo) & (K < khi)
            V = W.astype(F64)
            p = np.zeros((T, W.shape[1]), F64)
            for k0 in range(0, M, T):                       # slice s takes k = s, s + T, ...: ascending k
                r = min(T, M - k0)
                p[:r] = np.where(inside[k0:k0 + r], p[:r] + V[k0:k0 + r], p[:r])
            h = 1
            while h < T:                                    # p[j] += p[j + h] for j = 0, 2h, 4h, ...
                p[0::2 * h] = p[0::2 * h] + p[h::2 * h]
                h *= 2
            S = p[0] + tlo
        else:
            S = tlo
        S = np.where(chi > 0, S + chi.astype(F64) * hi, S)
        return (S / F64(n)).astype(F32)


def reference(W, b):
    """The sorted float64 mean of the kept values (finite inputs)."""
    M = W.shape[0]
    return np.sort(np.asarray(W, F32).astype(F64), 0)[b:M - b].mean(0)


def bound(W, b):
    """|out - ref| <= 2^-24 |ref| + n 2^-52 mean|kept| + 2^-149: one float rounding, the first-order error
    of any ordering of n double additions, a subnormal slack."""
    M = W.shape[0]
    n = M - 2 * b
    kept = np.sort(np.asarray(W, F32).astype(F64), 0)[b:M - b]
    return 2.0 ** -24 * np.abs(kept.mean(0)) + n * 2.0 ** -52 * np.abs(kept).mean(0) + 2.0 ** -149


def same_bits(got, ref):
    """Bitwise equal, a NaN equal to any NaN."""
    got, ref = np.asarray(got, F32).reshape(-1), np.asarray(ref, F32).reshape(-1)
    gn, rn = np.isnan(got), np.isnan(ref)
    return got.shape == ref.shape and bool((gn == rn).all()) and got[~gn].tobytes() == ref[~rn].tobytes()


def trim_count(rule, trim, M):
    """b of a round of M clients (tools.robust_trim_count, fs_plan_set_robust)."""
    if rule == 'median':
        return (M - 1) // 2
    if rule == 'mean':
        return 0
    return min(int(np.floor(float(trim) * float(M))), (M - 1) // 2)


# ---- inputs shared by the CPU and the GPU tests ----

def inputs(kind, M, L, seed=0):
    """[M, L] float32 rows of one input family."""
    rs = np.random.RandomState(1000 * seed + 7 * M + L)
    if kind == 'normal':
        return rs.normal(size=(M, L)).astype(F32)
    if kind == 'quantised':                                  # at most 3 distinct values per column
        lv = rs.normal(size=(3, L)).astype(F32)
        return np.take_along_axis(lv, rs.randint(0, 3, size=(M, L)), 0)
    if kind == 'equal':
        return np.repeat(rs.normal(size=(1, L)).astype(F32), M, 0)
    if kind == 'zeros':                                      # +0 and -0 only
        return np.where(rs.randint(0, 2, size=(M, L)) == 1, F32(-0.0), F32(0.0)).astype(F32)
    if kind == 'wide':                                       # mixed signs, magnitudes 1e-30 .. 1e30
        mag = 10.0 ** rs.uniform(-30, 30, size=(M, L))
        return (mag * rs.choice([-1.0, 1.0], size=(M, L))).astype(F32)
    if kind == 'near_one':                                   # sign-mixed near +-1: heavy cancellation
        return (rs.choice([-1.0, 1.0], size=(M, L)) * (1.0 + 1e-3 * rs.normal(size=(M, L)))).astype(F32)
    if kind == 'digits':                                     # column j: keys that differ in the 4-bit digit j % 8 only
        base = rs.normal(size=L).astype(F32).view(U32)
        d = rs.randint(0, 16, size=(M, L)).astype(U32)
        sh = (4 * (np.arange(L) % 8)).astype(U32)
        # (digit 7 holds sign and exponent top: keep it to the sign bit, so that no Inf / NaN appears)
        d = np.where(sh == 28, (d & 1) << 3, d).astype(U32)
        bits = (base & ~(U32(15) << sh)) ^ (d << sh)
        return bits.astype(U32).view(F32)
    raise ValueError(kind)


KINDS = ('normal', 'quantised', 'equal', 'zeros', 'wide', 'near_one', 'digits')


# ---- the drop-in cases (tests/test_gpu_robust.py): N = 12 unequal clients, C = 3 (regression: 1), D = 32 ----
SIZES = [21, 8, 37, 5, 16, 12, 9, 30, 14, 7, 25, 11]
D, C, R, E, B, LR, LAM, MU = 32, 3, 2, 2, 8, 0.5, 0.001, 0.1
TORCH_SEED, SAMPLE_SEED, DATA_SEED, PARTICIPATION = 100, 0, 78, 0.5


def case_data(regression=False):
    """The inputs of every drop-in case: random-feature rows with a label skew across the clients;
    regression: a noisy linear target of the same rows."""
    rs = np.random.RandomState(DATA_SEED)
    n, nt = sum(SIZES), 40
    raw = rs.normal(size=(n + nt, 10)).astype(F32)
    phi = (np.cos(raw @ rs.normal(0, 0.7, size=(10, D)).astype(F32) + rs.uniform(0, 2 * np.pi, size=(1, D)).astype(F32))
           / np.sqrt(D)).astype(F32)
    lab = np.argmax(phi @ rs.normal(size=(D, C)).astype(F32) + 0.1 * rs.normal(size=(n + nt, C)), axis=1).astype(np.int64)
    order = np.argsort(lab[:n] + 1.5 * rs.normal(size=n), kind='stable')     # non-IID: clients sorted along the label
    y = lab
    if regression:
        y = (phi @ rs.normal(size=D).astype(F32) + 0.05 * rs.normal(size=n + nt)).astype(F32)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    Xs = [phi[order][off[i]:off[i + 1]] for i in range(len(SIZES))]
    ys = [y[:n][order][off[i]:off[i + 1]] for i in range(len(SIZES))]
    return Xs, ys, phi[n:], y[n:]

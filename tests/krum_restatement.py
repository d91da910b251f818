"""fs_aggregate_krum restated in numpy, in two parts that never meet in one comparison:

(i)  the squared distances in float64 from the float32 differences ``fl(W_k - x)`` -- the value that
     fs_krum_distances approximates within the a-priori bound of include/fedsim.h (``dist_bound``);
(ii) from a GIVEN float32 matrix D: every row's score, the pick and the weights of the final fold,
     in exactly the header's order -- fs_krum_select equals it bit for bit.

The selection is a sort here: which algorithm finds the n-th smallest value cannot matter, since values
that tie at the threshold are equal floats.  What has to be reproduced is the sum: 256 slices, slice s
holding 0.0 plus the values strictly below the threshold at b = s, s + 256, ... in ascending b (b != a),
the slices joined by the pairwise tree, then count * threshold."""
import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32

MAX_M = 5120            # fs_aggregate_krum_max_m()
NT = 256                # slices of a row's sum
TILE, BK, MIN_STEPS, TARGET_WG = 128, 32, 8, 512


def ldd(M):
    """The row pitch of D."""
    return (int(M) + 3) & ~3


def split(M, length):
    """(S, kc) of fs_krum_split: slices of the len axis and K-steps of 32 per slice."""
    T = (M + TILE - 1) // TILE
    P = T * (T + 1) // 2
    nk = (length + BK - 1) // BK
    smax = max(1, TARGET_WG // P)
    kc = max(MIN_STEPS, (nk + smax - 1) // smax)
    return (nk + kc - 1) // kc, kc


def chain(M, length):
    """The longest chain of additions a product passes through on its way into D_ab."""
    S, kc = split(M, length)
    return min(length, BK * kc) + S + 1


# ---- (i) ----

def centred(W, x):
    """fl(W_k - x) in float32."""
    return (np.ascontiguousarray(W, dtype=F32) - np.asarray(x, dtype=F32)[None, :]).astype(F32)


def distances64(W, x, gram=None):
    """float64 [M, M]: ||U_a - U_b||^2 of the float32 differences (finite inputs), and ||U_a||^2.
    Small inputs: from the differences themselves.  ``gram`` (default: above 2e7 multiply-adds): from the
    float64 Gram matrix, max(0, n2_a + n2_b - 2 G_ab) -- its own error, about len 2^-52 (n2_a + n2_b), is
    2^-28 of dist_bound's first term."""
    U = centred(W, x).astype(F64)
    M = U.shape[0]
    n2 = (U * U).sum(1)
    if gram is None:
        gram = M * M * U.shape[1] > 2e7
    if gram:
        D = np.maximum(n2[:, None] + n2[None, :] - 2.0 * (U @ U.T), 0.0)
    else:
        D = np.zeros((M, M), F64)
        for a in range(M):
            d = U - U[a][None, :]
            D[a] = (d * d).sum(1)
    D[np.arange(M), np.arange(M)] = 0.0
    return D, n2


def dist_bound(D64, n2, M, length):
    """|D^ - D| <= 2 g (||U_a||^2 + ||U_b||^2) + 2^-24 D, g = n 2^-24 / (1 - n 2^-24), n = chain(M, len)."""
    n = chain(M, length)
    assert n <= length + 2
    u = n * 2.0 ** -24
    g = u / (1.0 - u)
    return 2.0 * g * (n2[:, None] + n2[None, :]) + 2.0 ** -24 * D64


# ---- (ii) ----

def scores(D, f):
    """float64 [M] from float32 D [M, M] (>= 0 or +Inf); all rows at once."""
    D = np.ascontiguousarray(D, dtype=F32)
    M = D.shape[0]
    n = M - f - 2
    assert M >= 3 and f >= 0 and n >= 1 and D.shape == (M, M)
    K = D.view(U32)
    off = ~np.eye(M, dtype=bool)
    Kx = np.where(off, K, U32(0xFFFFFFFF))                   # a itself: out of the n smallest, by index
    thr = np.partition(Kx, n - 1, axis=1)[:, n - 1]
    below = off & (K < thr[:, None])
    c = n - below.sum(1)
    assert (c >= 1).all()
    p = np.zeros((M, NT), F64)
    with np.errstate(all='ignore'):
        for b0 in range(0, M, NT):                           # slice s takes b = s, s + 256, ...: ascending b
            r = min(NT, M - b0)
            # (p + 0.0 is p: the sums are >= 0, so a term left out and a term of 0.0 give the same bits)
            p[:, :r] = p[:, :r] + np.where(below[:, b0:b0 + r], D[:, b0:b0 + r].astype(F64), 0.0)
        h = 1
        while h < NT:                                        # p[j] += p[j + h] for j = 0, 2h, 4h, ...
            p[:, 0::2 * h] = p[:, 0::2 * h] + p[:, h::2 * h]
            h *= 2
        return p[:, 0] + c.astype(F64) * thr.view(F32).astype(F64)


def pick(score, m, sel=None):
    """The row ids of the m smallest (score, position), in ascending position; int32 [m]."""
    score = np.asarray(score, F64)
    M = len(score)
    order = np.lexsort((np.arange(M), score.view(np.uint64)))     # bits: scores are >= 0, NaN above +Inf
    pos = np.sort(order[:m])
    ids = pos if sel is None else np.asarray(sel)[pos]
    return ids.astype(np.int32)


def select(D, f, m, sel=None):
    """fs_krum_select: (score [M] float64, pick [m] int32, q [m] float32 == f32(1 / m))."""
    s = scores(D, f)
    return s, pick(s, m, sel), np.full(m, F32(1.0 / m), F32)


def sorted_score(D, f):
    """The sorted float64 sum of the n smallest off-diagonal values of every row."""
    D = np.asarray(D, F32).astype(F64)
    M = D.shape[0]
    n = M - f - 2
    out = np.zeros(M, F64)
    with np.errstate(all='ignore'):
        for a in range(M):
            out[a] = np.sort(np.delete(D[a], a))[:n].sum()
    return out


def same_bits(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    return got.shape == ref.shape and got.dtype == ref.dtype and got.tobytes() == ref.tobytes()


def counts(f, m, M):
    """(f, m) of a round of M clients as tools.krum_counts: f a count or a fraction, m None: M - f."""
    fc = int(f) if isinstance(f, (int, np.integer)) else int(np.floor(float(f) * float(M)))
    return fc, (M - fc if m is None else int(m))


# ---- inputs shared by the CPU and the GPU tests ----

def sym(A):
    """A symmetric float32 matrix with a zero diagonal from the upper triangle of A."""
    A = np.triu(np.asarray(A, F32), 1)
    return (A + A.T).astype(F32)


def hand_made():
    """Named (D, f, m) cases: ties at the threshold, duplicate rows, +Inf rows, f = 0, n = 1, m = 1 and
    m = M - f, equal scores resolved by id."""
    inf = np.inf
    out = {}
    # ties at the threshold: row 0's off-diagonal values 1 1 1 1 2, n = 3 -- three of four equal copies kept
    A = sym([[0, 1, 1, 1, 1, 2], [0, 0, 3, 4, 5, 6], [0, 0, 0, 7, 8, 9], [0, 0, 0, 0, 2, 3], [0, 0, 0, 0, 0, 1],
             [0, 0, 0, 0, 0, 0]])
    out['ties_at_threshold'] = (A, 1, 1)
    out['ties_multi'] = (A, 1, 5)
    # duplicate rows: D_01 = 0 with 0 != 1, and both rows otherwise equal -- equal scores, id decides
    B = sym([[0, 0, 2, 3, 4], [0, 0, 2, 3, 4], [0, 0, 0, 1, 5], [0, 0, 0, 0, 6], [0, 0, 0, 0, 0]])
    out['duplicate_rows_krum'] = (B, 1, 1)
    out['duplicate_rows_multi'] = (B, 1, 4)
    # all rows at equal distances: every score equal, the ids 0..m-1 win
    E = sym(np.ones((7, 7)))
    out['equal_scores_by_id'] = (E, 2, 3)
    out['equal_scores_f0'] = (E, 0, 7)
    # +Inf rows: rows 2 and 5 are at +Inf from everyone
    G = sym(np.arange(64, dtype=np.float32).reshape(8, 8) + 1)
    G[[2, 5], :] = inf
    G[:, [2, 5]] = inf
    G[np.arange(8), np.arange(8)] = 0
    out['inf_rows_krum'] = (G, 2, 1)
    out['inf_rows_multi'] = (G, 2, 6)
    out['inf_rows_too_many'] = (G, 1, 7)       # (f = 1 < 2 bad rows, m = 7: one +Inf score is picked, last by score)
    # f = 0 and n = 1 at the smallest M
    H = sym([[0, 3, 1], [0, 0, 2], [0, 0, 0]])
    out['M3_f0_n1_krum'] = (H, 0, 1)
    out['M3_f0_n1_all'] = (H, 0, 3)
    out['n1_M5'] = (sym(np.arange(25).reshape(5, 5) % 7 + 1), 2, 3)
    return out


def random_D(M, seed=0, quantised=False, n_inf=0):
    """A symmetric float32 distance matrix with a zero diagonal; quantised: few distinct values (ties);
    n_inf rows (and columns) at +Inf."""
    rs = np.random.RandomState(1000 * seed + M)
    A = rs.randint(1, 4, size=(M, M)).astype(F32) if quantised else rs.gamma(2.0, 1.0, size=(M, M)).astype(F32)
    D = sym(A)
    if n_inf:
        bad = rs.permutation(M)[:n_inf]
        D[bad, :] = np.inf
        D[:, bad] = np.inf
        D[np.arange(M), np.arange(M)] = 0
    return D


def fm_cases(M):
    """Several (f, m) per M: f = 0, 1, a tenth, the largest with M >= 2f + 3 and the largest at all
    (n = 1); m = 1, M - f and one in between."""
    fs = sorted({f for f in (0, 1, M // 10, (M - 3) // 2, M - 3) if f >= 0 and M - f - 2 >= 1})
    out = []
    for f in fs:
        for m in sorted({1, (M - f + 1) // 2, M - f}):
            out.append((f, m))
    return out


def rows(kind, M, L, seed=0):
    """(W [M, L], x [L]) float32 of one input family of the distance stage."""
    rs = np.random.RandomState(1000 * seed + 7 * M + L)
    x = rs.normal(size=L).astype(F32)
    W = (x[None, :].astype(F64) + 1e-3 * rs.normal(size=(M, L))).astype(F32)     # |x| ~ 1, updates ~ 1e-3
    if kind == 'gaussian':
        return W, x
    if kind == 'duplicate':
        W[M - 1] = W[0]
        return W, x
    if kind == 'bad':                                        # one NaN row, one Inf row, one 1e30 row where M allows
        W[0, L // 2] = np.nan
        if M > 3:
            W[M // 2, 0] = np.inf
        if M > 4:
            W[M - 1, :] = 1e30
        return W, x
    raise ValueError(kind)


def bad_rows(M):
    return sorted({0} | ({M // 2} if M > 3 else set()) | ({M - 1} if M > 4 else set()))


# ---- the drop-in cases (tests/test_gpu_krum.py): N = 14 unequal clients, C = 3 (regression: 1), D = 32 ----
SIZES = [21, 8, 37, 5, 16, 12, 9, 30, 14, 7, 25, 11, 19, 13]
D, C, R, E, B, LR, LAM, MU = 32, 3, 2, 2, 8, 0.5, 0.001, 0.1
TORCH_SEED, SAMPLE_SEED, DATA_SEED, PARTICIPATION = 100, 0, 78, 0.6


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

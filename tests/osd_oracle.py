"""The numpy statement of ordered-statistics post-processing (include/ldpc_hip.h ldpc_osd_*), one frame at a time.
test_osd_cpu.py checks it against the code books of the toy codes; test_gpu_osd.py holds the device to it bit for bit."""
import numpy as np


def hard(llr):
    """h_v = (llr_v < 0): NaN and +-0 give 0."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(llr) < 0).astype(np.uint8)


def sort_order(post):
    """pi: the variables in ascending order of the key (bits of fp32 |post_v| << 32) | v, NaN counted as 0."""
    post = np.asarray(post)
    with np.errstate(over="ignore", invalid="ignore"):
        rho = np.abs(np.where(np.isnan(post), 0, post)).astype(np.float32)  # nearest-even; beyond fp32: inf
    keys = (rho.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(post), dtype=np.uint64)
    return np.argsort(keys, kind="stable").astype(np.int64)


def rref(A):
    """Reduced row echelon form over GF(2) of A [m, n] in {0,1}, columns left to right, pivot = the first unused row with a 1 (the
    reduced form does not depend on that choice).  -> (R [m, n] uint8, rowof [n]: pivot row of each column, -1 = free).  Rows are
    packed into bytes so that a row operation is one XOR of n / 8 bytes per row."""
    m, n = A.shape
    P = np.packbits(np.asarray(A, dtype=np.uint8), axis=1)
    used = np.zeros(m, dtype=bool)
    rowof = np.full(n, -1, dtype=np.int64)
    for j in range(n):
        col = (P[:, j >> 3] >> (7 - (j & 7))) & 1
        cand = np.flatnonzero((col == 1) & ~used)
        if len(cand) == 0:
            continue
        r = cand[0]
        used[r] = True
        rowof[j] = r
        others = np.flatnonzero(col)
        others = others[others != r]
        P[others] ^= P[r]
    return np.unpackbits(P, axis=1)[:, :n], rowof


def eliminate(H, post):
    """Steps 2 and 3 for one frame -> (pi, reduced form of H[:, pi], rowof)."""
    pi = sort_order(post)
    R, rowof = rref(np.asarray(H, dtype=np.uint8)[:, pi])
    return pi, R, rowof


def osd_frame(H, post, prior, order, depth, elim=None):
    """One frame.  H [m, n] in {0,1}; post, prior [n] of one dtype (float32 / float64); order in {0, 1}; depth >= 0.
    -> (word uint8 [n], pick, cost).  pick = -1, cost = -1.0: the hard decisions of post are a codeword and are returned untouched.
    ``elim``: ``eliminate(H, post)`` computed earlier (the same frame under several (order, depth))."""
    H = np.asarray(H, dtype=np.uint8)
    post, prior = np.asarray(post), np.asarray(prior)
    assert post.dtype == prior.dtype and post.dtype in (np.float32, np.float64) and order in (0, 1) and depth >= 0
    m, n = H.shape
    h = hard(post)
    if not ((H.astype(np.int64) @ h.astype(np.int64)) % 2).any():
        return h, -1, -1.0
    pi, R, rowof = eliminate(H, post) if elim is None else elim
    free = np.flatnonzero(rowof < 0)
    piv = np.flatnonzero(rowof >= 0)
    hp = h[pi]
    T = min(int(depth), len(free)) if order == 1 else 0
    # candidates in POSITION order: row t of X
    X = np.zeros((T + 1, n), dtype=np.uint8)
    X[:, free] = hp[free]
    for t in range(1, T + 1):
        X[t, free[t - 1]] ^= 1
    Rf = R[np.ix_(rowof[piv], free)].astype(np.float64)  # [pivots, free]: the free bits each pivot row sums (counts < 2^53: exact)
    X[:, piv] = ((X[:, free].astype(np.float64) @ Rf.T) % 2).astype(np.uint8)
    # score: fp64, from +0.0, positions in order, plain adds
    g = hard(prior)[pi]
    w = np.abs(np.where(np.isnan(prior), 0, prior)).astype(np.float64)[pi]
    cost = np.zeros(T + 1, dtype=np.float64)
    for p in range(n):
        d = X[:, p] != g[p]
        cost[d] = cost[d] + w[p]
    t = int(np.argmin(cost))  # the first minimum: the smallest t on equal cost
    word = np.zeros(n, dtype=np.uint8)
    word[pi] = X[t]
    return word, t, float(cost[t])

"""The numpy statement of bit-sliced Gallager-B (include/ldpc_hip.h ldpc_hard_*).

TEST INFRASTRUCTURE ONLY, written from the contract, not from the kernels.  ``galb_decode`` handles a batch at once: the messages of
all frames are rows of one uint8 array in H's row-major edge order, the check rule is ``np.bitwise_xor.reduceat`` over the CSR order, the
vote count ``np.add.reduceat`` over the CSC order; frames that have left are dropped from the arrays.  ``galb_decode_plain`` is the
same contract one frame and one edge at a time, for cross-checking the vectorised form on small cases.
"""
import numpy as np

NO_EARLY_EXIT = 1


def flip_threshold(d, t):
    """b_d: floor((d - 1) / 2) + 1 for t = 0, min(t, max(d - 1, 1)) for t >= 1."""
    d = np.asarray(d, dtype=np.int64)
    if t == 0:
        return np.where(d > 0, (d - 1) // 2, 0) + 1
    return np.minimum(t, np.maximum(d - 1, 1))


class Graph:
    def __init__(self, m, n, edge_chk, edge_var):
        self.m, self.n = int(m), int(n)
        chk, var = np.asarray(edge_chk, dtype=np.int64), np.asarray(edge_var, dtype=np.int64)
        order = np.lexsort((var, chk))  # row-major: by check, then variable
        self.chk, self.var = chk[order], var[order]
        self.E = len(self.chk)
        self.dc = np.bincount(self.chk, minlength=self.m)
        self.dv = np.bincount(self.var, minlength=self.n)
        self.rows = np.flatnonzero(self.dc)  # checks with an edge (reduceat has no empty segments)
        self.row_start = (np.cumsum(self.dc) - self.dc)[self.rows]
        self.csc = np.lexsort((self.chk, self.var))  # edges in variable-major order
        self.cols = np.flatnonzero(self.dv)
        self.col_start = (np.cumsum(self.dv) - self.dv)[self.cols]

    @classmethod
    def of(cls, code):
        return code if isinstance(code, cls) else cls(code.m, code.n, code.edge_chk, code.edge_var)

    def syndrome_any(self, x):
        """x [n, F] uint8 -> [F] bool: some check is unsatisfied"""
        if not len(self.rows):
            return np.zeros(x.shape[1], dtype=bool)
        return np.bitwise_xor.reduceat(x[self.var], self.row_start, axis=0).any(axis=0)


def galb_decode(code, y, t=0, max_iter=20, flags=0):
    """y [B, n] in {0, 1} -> (xhat uint8 [B, n], iters int32 [B])"""
    g = Graph.of(code)
    if max_iter <= 0 or not 0 <= t <= 255:
        raise ValueError("max_iter >= 1 and 0 <= t <= 255")
    y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.uint8)
    B = y.shape[0]
    no_early = bool(flags & NO_EARLY_EXIT)
    xhat, iters = y.copy(), np.zeros(B, dtype=np.int32)
    yT = np.ascontiguousarray(y.T)  # [n, B]
    live = np.arange(B)
    if not no_early:
        live = live[g.syndrome_any(yT)]
    yl = yT[:, live]
    v2c = yl[g.var]  # [E, F]
    dv = g.dv[:, None]
    b = flip_threshold(g.dv, t)[g.var][:, None]
    for sweep in range(1, max_iter + 1):
        if not len(live):
            break
        par = np.zeros((g.m, len(live)), dtype=np.uint8)
        if len(g.rows):
            par[g.rows] = np.bitwise_xor.reduceat(v2c, g.row_start, axis=0)
        delta = par[g.chk] ^ v2c ^ yl[g.var]
        T = np.zeros((g.n, len(live)), dtype=np.int64)
        if len(g.cols):
            T[g.cols] = np.add.reduceat(delta[g.csc].astype(np.int64), g.col_start, axis=0)
        x = yl ^ (2 * T > dv + 1).astype(np.uint8)
        v2c = yl[g.var] ^ ((T[g.var] - delta) >= b).astype(np.uint8)
        xhat[live] = x.T
        iters[live] = sweep
        if no_early or sweep == max_iter:
            continue
        keep = g.syndrome_any(x)
        live, yl, v2c = live[keep], yl[:, keep], v2c[:, keep]
    if no_early:
        iters[:] = max_iter
    return xhat, iters


def galb_decode_plain(code, y, t=0, max_iter=20, flags=0):
    """One frame, one edge at a time: y [n] -> (xhat [n], iters)"""
    g = Graph.of(code)
    y = [int(v) for v in y]
    edges = list(zip(g.chk.tolist(), g.var.tolist()))
    no_early = bool(flags & NO_EARLY_EXIT)

    def codeword(x):
        s = [0] * g.m
        for c, v in edges:
            s[c] ^= x[v]
        return not any(s)

    if not no_early and codeword(y):
        return np.array(y, dtype=np.uint8), 0
    v2c = {(c, v): y[v] for c, v in edges}
    x = list(y)
    for sweep in range(1, max_iter + 1):
        par = [0] * g.m
        for c, v in edges:
            par[c] ^= v2c[(c, v)]
        delta = {(c, v): par[c] ^ v2c[(c, v)] ^ y[v] for c, v in edges}
        T = [0] * g.n
        for (c, v), dl in delta.items():
            T[v] += dl
        x = [y[v] ^ int(2 * T[v] > int(g.dv[v]) + 1) for v in range(g.n)]
        v2c = {(c, v): y[v] ^ int(T[v] - delta[(c, v)] >= int(flip_threshold(g.dv[v], t))) for c, v in edges}
        if not no_early and codeword(x):
            return np.array(x, dtype=np.uint8), sweep
    return np.array(x, dtype=np.uint8), max_iter

"""CPU restatement of layered (serial-C) corrected min-sum -- what the LDPC_ALG_LMSA kernels must reproduce bit for bit.

TEST INFRASTRUCTURE ONLY, written from the contract in include/ldpc_hip.h (LDPC_ALG_LMSA), not from the kernels; of
``oracle/bp_oracle.py`` it uses ``Edges`` and ``syndrome_ok``.  Per frame, in the arithmetic T (np.float64 or np.float32):

  layers   two checks of one layer share no variable; greedy default: check c takes the smallest layer none of whose earlier checks
           shares a variable with it; processing order ascending (layer, check index)
  init     marg = prior, every c2v = +0; x_hat = y0 if given
  exits    before each sweep: sweeps >= max_iter (<= 0: unbounded), or H x_hat = 0 (from sweep 1 on; at sweep 0 only with y0)
  sweep    for every check in processing order, edges in row-major order:
               v_j = marg[var_j] - c2v_j ;  s_j = product of the signs of the other v_i (sgn(x) = -1 iff x < 0) ;  m_j = min_{i != j} |v_i|
               c2v_j = s_j * max(fl(fl(scale * m_j) - offset), 0) ;  marg[var_j] = v_j + c2v_j
           then x_hat = (marg < 0)
numpy never fuses the multiply and the subtraction, so the two roundings are the contract's.
"""
import numpy as np

import bp_oracle as O


def _rows(g):
    """edges of every check, row-major: list of index arrays into the edge list"""
    chk = np.asarray(g.chk)
    assert (np.diff(chk) >= 0).all()
    ptr = np.searchsorted(chk, np.arange(g.m + 1))
    return [np.arange(ptr[c], ptr[c + 1]) for c in range(g.m)]


def greedy_layers(g):
    """layer(c) = the smallest l >= 0 such that no check c' < c with layer(c') = l shares a variable with c"""
    var = np.asarray(g.var)
    used = [set() for _ in range(g.n)]
    lay = np.zeros(g.m, dtype=np.int64)
    for c, k in enumerate(_rows(g)):
        taken = set().union(*(used[v] for v in var[k])) if k.size else set()
        l = 0
        while l in taken:
            l += 1
        lay[c] = l
        for v in var[k]:
            used[v].add(l)
    return lay


def check_layers(g, layers):
    """ValueError unless ``layers`` is one non-negative int per check and no two checks of a layer share a variable"""
    lay = np.asarray(layers)
    if lay.ndim != 1 or lay.size != g.m or lay.dtype.kind not in "iu" or (lay < 0).any():
        raise ValueError("a layering is one non-negative integer per check")
    pairs = set()
    for l, v in zip(lay[np.asarray(g.chk)].tolist(), np.asarray(g.var).tolist()):
        if (l, v) in pairs:
            raise ValueError("two checks of layer %d share variable %d" % (l, v))
        pairs.add((l, v))
    return lay.astype(np.int64)


def processing_order(layers):
    return np.argsort(np.asarray(layers), kind="stable")  # ascending (layer, check index)


def lmsa_decode(g, y0, priors, max_iter, scale, offset, layers=None, dtype=np.float64, early_exit=True, one_by_one=False):
    """Batched layered min-sum.  y0: [B, n] received words for the iteration-0 check or None, priors [B, n].  -> (xhat uint8 [B, n],
    iters int32 [B], soft [B, n] of ``dtype``: the marginals of each frame's last executed sweep, 0 where it executed none).
    ``early_exit`` False: no syndrome exits (LDPC_FLAG_NO_EARLY_EXIT), every frame runs max_iter sweeps."""
    dt = np.dtype(dtype).type
    priors = np.atleast_2d(np.asarray(priors)).astype(dt)
    B = priors.shape[0]
    lay = greedy_layers(g) if layers is None else check_layers(g, layers)
    rows, var = _rows(g), np.asarray(g.var)
    if min(r.size for r in rows) < 2:
        raise ValueError("a check of degree < 2")
    a, b, zero = dt(scale), dt(offset), dt(0)
    marg = priors.copy()
    c2v = np.zeros((B, len(var)), dtype=dt)
    x_hat = np.zeros((B, g.n), dtype=np.uint8) if y0 is None else np.atleast_2d(np.asarray(y0)).astype(np.uint8).copy()
    soft = np.zeros((B, g.n), dtype=dt)
    iters = np.zeros(B, dtype=np.int32)
    live = np.ones(B, dtype=bool)
    # The checks of a layer touch disjoint variables (check_layers), so processing them together equals processing them one by one in
    # ascending (layer, index) order; ``one_by_one`` does exactly that, for the test that says so.
    if one_by_one:
        groups = [rows[c][None, :] for c in processing_order(lay)]
    else:
        groups = []
        deg = np.array([r.size for r in rows])
        for l in np.unique(lay):
            for d in np.unique(deg[lay == l]):
                groups.append(np.stack([rows[c] for c in np.flatnonzero((lay == l) & (deg == d))]))
    sweeps = 0
    cap = max_iter if max_iter > 0 else 100000
    while sweeps < cap:
        if early_exit and (sweeps > 0 or y0 is not None):
            live &= ~O.syndrome_ok(g, x_hat.astype(np.int64))
        if not live.any():
            break
        L = np.flatnonzero(live)
        for K in groups:  # [checks, dc] edge indices: checks of one layer and one degree, independent of each other
            vs = var[K]
            rows_of = L[:, None, None]
            v = marg[rows_of, vs] - c2v[rows_of, K]  # [frames, checks, dc], one subtraction
            neg = v < zero
            mag = np.abs(v)
            d = K.shape[1]
            new = np.empty_like(v)
            for j in range(d):
                others = [i for i in range(d) if i != j]
                m = mag[:, :, others].min(axis=2)
                s_neg = (neg[:, :, others].sum(axis=2) & 1).astype(bool)
                t = m * a
                t = t - b
                t = np.maximum(t, zero)
                new[:, :, j] = np.where(s_neg, -t, t)
            assert new.dtype == dt
            c2v[rows_of, K] = new
            marg[rows_of, vs] = v + new  # one addition
        x_hat[L] = (marg[L] < zero).astype(np.uint8)
        soft[L] = marg[L]
        iters[L] += 1
        sweeps += 1
    return x_hat, iters, soft

"""CPU restatement of layered fixed-point min-sum -- what the ``ldpc_lqmsa_*`` kernel must reproduce exactly.

TEST INFRASTRUCTURE ONLY, written from the contract in include/ldpc_hip.h (the LQMSA block), not from the kernel.  The quantiser is
``qmsa_oracle.quantise``; the layering (greedy default, validity, processing order) is ``lmsa_oracle``'s; ``bp_oracle`` gives ``Edges`` and
``syndrome_ok``.  After the quantiser every value is a numpy int64 and every operation an integer one.  With V = 2^(bits-1) - 1 and
scale64 = 64 * scale:

  init     marg = level, every c2v = 0; x_hat = y0 if given
  exits    before each sweep: sweeps >= max_iter (<= 0: unbounded, capped at 100000), or H x_hat = 0 (from sweep 1 on; at sweep 0 only with y0)
  sweep    for every check in processing order, edges in row-major order:
               v_j = marg[var_j] - c2v_j ;  a_j = min(|v_j|, V) ;  neg_j = (v_j < 0)
               m_j = min_{i != j} a_i ;  s_j = XOR_{i != j} neg_i
               c2v_j = (s_j ? -1 : +1) * max(((scale64 * m_j) >> 6) - offset, 0) ;  marg[var_j] = v_j + c2v_j      (v_j is not clipped)
           then x_hat = (marg < 0)
"""
import numpy as np

import bp_oracle as O
import lmsa_oracle as L
import qmsa_oracle as Q


def scale64_of(scale):
    s = 64.0 * float(scale)
    if not (0.0 < float(scale) <= 1.0) or s != int(s):
        raise ValueError("scale is a multiple of 1/64 with 0 < scale <= 1")
    return int(s)


def check_params(bits, frac_bits, scale, offset):
    if int(bits) != bits or not 2 <= bits <= 8 or int(frac_bits) != frac_bits or not -8 <= frac_bits <= 8 or int(offset) != offset or offset < 0:
        raise ValueError("2 <= bits <= 8, -8 <= frac_bits <= 8, an integer offset >= 0")
    return scale64_of(scale)


def lqmsa_decode(g, y0, priors, max_iter, bits=6, frac_bits=2, scale=0.8125, offset=0, layers=None, early_exit=True, one_by_one=False):
    """Batched layered fixed-point min-sum.  y0: [B, n] received words for the iteration-0 check or None; priors [B, n] float32 or float64
    (quantised in their own type).  -> (xhat uint8 [B, n], iters int32 [B], soft int16 [B, n]: the marginals in levels of each frame's last
    executed sweep, 0 where it executed none, the largest |v_j| seen).  ``early_exit`` False: LDPC_FLAG_NO_EARLY_EXIT."""
    s64 = check_params(bits, frac_bits, scale, offset)
    V = Q.vmax_of(bits)
    priors = np.atleast_2d(np.asarray(priors))
    assert priors.dtype in (np.float32, np.float64)
    level = Q.quantise(priors, bits, frac_bits)
    marg = level.astype(np.int64)
    assert (marg == level).all() and (np.abs(marg) <= V).all()
    B = marg.shape[0]
    lay = L.greedy_layers(g) if layers is None else L.check_layers(g, layers)
    rows, var = L._rows(g), np.asarray(g.var)
    if min(r.size for r in rows) < 2:
        raise ValueError("a check of degree < 2")
    c2v = np.zeros((B, len(var)), dtype=np.int64)
    x_hat = np.zeros((B, g.n), dtype=np.uint8) if y0 is None else np.atleast_2d(np.asarray(y0)).astype(np.uint8).copy()
    soft = np.zeros((B, g.n), dtype=np.int16)
    iters = np.zeros(B, dtype=np.int32)
    live = np.ones(B, dtype=bool)
    # the checks of a layer touch disjoint variables, so processing them together equals processing them one by one in ascending
    # (layer, index) order; ``one_by_one`` does exactly that
    if one_by_one:
        groups = [rows[c][None, :] for c in L.processing_order(lay)]
    else:
        groups = []
        deg = np.array([r.size for r in rows])
        for l in np.unique(lay):
            for d in np.unique(deg[lay == l]):
                groups.append(np.stack([rows[c] for c in np.flatnonzero((lay == l) & (deg == d))]))
    peak = 0
    sweeps = 0
    cap = max_iter if max_iter > 0 else 100000
    while sweeps < cap:
        if early_exit and (sweeps > 0 or y0 is not None):
            live &= ~O.syndrome_ok(g, x_hat.astype(np.int64))
        if not live.any():
            break
        F = np.flatnonzero(live)
        for K in groups:  # [checks, dc] edge indices: checks of one layer and one degree
            vs = var[K]
            fr = F[:, None, None]
            v = marg[fr, vs] - c2v[fr, K]  # [frames, checks, dc]
            peak = max(peak, int(np.abs(v).max()))
            a = np.minimum(np.abs(v), V)
            neg = (v < 0).astype(np.int64)
            d = K.shape[1]
            new = np.empty_like(v)
            for j in range(d):
                others = [i for i in range(d) if i != j]
                m = a[:, :, others].min(axis=2)
                s = neg[:, :, others].sum(axis=2) & 1
                mag = np.maximum(((s64 * m) >> 6) - int(offset), 0)
                new[:, :, j] = np.where(s == 1, -mag, mag)
            assert new.dtype == np.int64
            c2v[fr, K] = new
            marg[fr, vs] = v + new
        assert np.abs(marg[F]).max() < 2 ** 15
        x_hat[F] = (marg[F] < 0).astype(np.uint8)
        soft[F] = marg[F].astype(np.int16)
        iters[F] += 1
        sweeps += 1
    return x_hat, iters, soft, peak


def pack_words(xhat):
    """Decisions as packed words in the layout of ldpc_decode_bits: bit (v & 31) of word (v >> 5), padding bits 0 -> uint32 [B, ceil(n/32)]"""
    B, n = xhat.shape
    W = (n + 31) // 32
    padded = np.zeros((B, W * 32), dtype=np.uint8)
    padded[:, :n] = xhat & 1
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(B, W)

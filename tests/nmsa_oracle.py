"""CPU restatement of corrected (normalised / offset) min-sum -- what the LDPC_ALG_NMSA kernels must reproduce bit for bit.

TEST INFRASTRUCTURE ONLY, built from the pieces of ``oracle/bp_oracle.py`` (``Edges``, ``msa_check_update``, ``syndrome_ok``,
``sum_cols``), which it does not edit.  The rule (include/ldpc_hip.h, LDPC_ALG_NMSA): with m_j the plain min-sum magnitude on edge j
and s_j its sign (src/bpa.py:86-102),

    c2v_j = s_j * max( fl( fl(scale * m_j) - offset ), 0 )

in the decoder's arithmetic T (np.float64 or np.float32), scale and offset cast to T ONCE, two roundings (numpy never fuses a multiply
and a subtraction).  Everything else is ``BPA.decode`` (src/bpa.py:17-63): ordered column sums from +0.0, prior last, v2c = marginal -
c2v, syndrome exit on the previous decisions, iteration-0 check of the received word, marginal < 0 <=> bit 1.
"""
import numpy as np

import bp_oracle as O


def correct(mag, scale, offset):
    """x -> max(fl(fl(scale * x) - offset), 0) in the dtype of ``mag`` (scale / offset: scalars of that dtype)."""
    dt = mag.dtype.type
    t = mag * dt(scale)
    t = t - dt(offset)
    return np.maximum(t, dt(0))


def nmsa_check_update(g, v2c, scale, offset):
    """Corrected min-sum check rule in the dtype of ``v2c``.  ``msa_check_update`` only compares and negates, so its (float64) result
    holds the plain rule's values of any narrower dtype exactly; sign and magnitude are taken apart, the magnitude corrected in T."""
    dt = v2c.dtype.type
    plain = O.msa_check_update(g, v2c)
    mag = correct(np.abs(plain).astype(dt), dt(scale), dt(offset))
    return np.where(np.signbit(plain), -mag, mag)


def nmsa_decode(g, y, priors, max_iter, scale, offset, dtype=np.float64):
    """Batched corrected min-sum.  y: [B, n] received words for the iteration-0 check (None: no such check -- a real-valued BI-AWGN
    observation never passes it), priors [B, n].  -> (xhat uint8 [B, n], iters int32 [B], soft [B, n] of ``dtype``: the marginals of each
    frame's last executed sweep, 0 where it executed none)."""
    dt = np.dtype(dtype).type
    priors = np.atleast_2d(np.asarray(priors)).astype(dt)
    B = priors.shape[0]
    a, b = dt(scale), dt(offset)
    x_hat = np.zeros((B, g.n), dtype=np.uint8)
    soft = np.zeros((B, g.n), dtype=dt)
    iters = np.zeros(B, dtype=np.int32)
    live = np.ones(B, dtype=bool)
    if y is not None:
        x_hat = np.atleast_2d(np.asarray(y)).astype(np.uint8)
    v2c = priors[:, g.var].copy()
    it = 0
    while live.any():
        if 0 < max_iter <= it:
            break
        if it > 0 or y is not None:
            live &= ~O.syndrome_ok(g, x_hat.astype(np.int64))
        if not live.any():
            break
        L = np.flatnonzero(live)
        c2v = nmsa_check_update(g, v2c[L], a, b)
        assert c2v.dtype == dt
        marginal = priors[L] + g.sum_cols(c2v)
        v2c[L] = marginal[:, g.var] - c2v
        assert marginal.dtype == dt and not np.isnan(marginal).any()
        x_hat[L] = (marginal < 0).astype(np.uint8)
        soft[L] = marginal
        iters[L] += 1
        it += 1
    return x_hat, iters, soft

"""CPU restatement of fixed-point min-sum -- what the LDPC_ALG_QMSA kernels must reproduce bit for bit, in every precision.

TEST INFRASTRUCTURE ONLY, built from the pieces of ``oracle/bp_oracle.py`` (``Edges``, ``msa_check_update``, ``syndrome_ok``,
``sum_cols``), which it does not edit.  The rule (include/ldpc_hip.h, LDPC_ALG_QMSA), with V = 2^(bits-1) - 1:

    level_v = clamp( rint(prior_v * 2^frac_bits), -V, +V )                      the quantiser, in the type the priors arrive in
    c2v_j   = s_j * max( floor(scale * min(m_j, V)) - offset, 0 )               m_j, s_j: the plain min-sum magnitude and sign

``qmsa_decode`` states it in a floating type T (np.float64 or np.float32) the way the kernels compute it: the variable -> check messages
clipped to +-V, the plain rule of ``bp_oracle``, then ``min(mag, V)``, ``floor(mag * scale) - offset`` and ``max(., 0)`` in T, the sign kept.
Everything else is ``BPA.decode`` (src/bpa.py:17-63).  ``qmsa_decode_int`` states the same rule for ONE frame with Python / numpy integers
and ``//`` only -- no floating-point operation after the quantiser -- and is what the float statements are held to.
"""
import numpy as np

import bp_oracle as O


def vmax_of(bits):
    return (1 << (int(bits) - 1)) - 1


def quantise(priors, bits, frac_bits):
    """clamp(rint(prior * 2^k), -V, V) in the dtype of ``priors`` (np.rint rounds half to even; +-inf -> +-V); -0 is returned as +0."""
    dt = priors.dtype.type
    V = dt(vmax_of(bits))
    q = np.rint(priors * dt(2.0 ** frac_bits))
    return np.clip(q, -V, V) + dt(0)


def fix(mag, scale, offset, V):
    """x -> max(floor(scale * min(x, V)) - offset, 0) in the dtype of ``mag``."""
    dt = mag.dtype.type
    t = np.minimum(mag, dt(V))
    t = np.floor(t * dt(scale)) - dt(offset)
    return np.maximum(t, dt(0))


def qmsa_check_update(g, v2c, scale, offset, V):
    """Fixed-point check rule in the dtype of ``v2c`` (integer levels held in floats)."""
    dt = v2c.dtype.type
    plain = O.msa_check_update(g, np.clip(v2c, -dt(V), dt(V)))  # compares and negations only: exact in float64 for any narrower dtype
    mag = fix(np.abs(plain).astype(dt), scale, offset, V)        # (a check of degree 1: |plain| = +inf -> V)
    return np.where(np.signbit(plain), -mag, mag)


def qmsa_decode(g, y, priors, max_iter, bits=6, frac_bits=2, scale=0.8125, offset=0, dtype=np.float64, early=True):
    """Batched fixed-point min-sum.  y: [B, n] received words for the iteration-0 check (None: none), priors [B, n] (quantised here, in
    ``dtype``).  -> (xhat uint8 [B, n], iters int32 [B], soft [B, n] of ``dtype``: the marginals, in levels, of each frame's last executed
    sweep, 0 where it executed none, peak |marginal| seen).  early=False: no syndrome exit (LDPC_FLAG_NO_EARLY_EXIT)."""
    dt = np.dtype(dtype).type
    V = vmax_of(bits)
    level = quantise(np.atleast_2d(np.asarray(priors)).astype(dt), bits, frac_bits)
    B = level.shape[0]
    x_hat = np.zeros((B, g.n), dtype=np.uint8)
    soft = np.zeros((B, g.n), dtype=dt)
    iters = np.zeros(B, dtype=np.int32)
    live = np.ones(B, dtype=bool)
    peak = 0.0
    if y is not None:
        x_hat = np.atleast_2d(np.asarray(y)).astype(np.uint8)
    v2c = level[:, g.var].copy()
    it = 0
    while live.any():
        if 0 < max_iter <= it:
            break
        if early and (it > 0 or y is not None):
            live &= ~O.syndrome_ok(g, x_hat.astype(np.int64))
        if not live.any():
            break
        L = np.flatnonzero(live)
        c2v = qmsa_check_update(g, v2c[L], scale, offset, V)
        assert c2v.dtype == dt
        marginal = level[L] + g.sum_cols(c2v)
        v2c[L] = marginal[:, g.var] - c2v
        assert marginal.dtype == dt and (marginal == np.rint(marginal)).all()
        peak = max(peak, float(np.abs(marginal).max()))
        x_hat[L] = (marginal < 0).astype(np.uint8)
        soft[L] = marginal
        iters[L] += 1
        it += 1
    return x_hat, iters, soft, peak


def qmsa_decode_int(g, y, levels, max_iter, bits=6, scale64=52, offset=0, early=True):
    """ONE frame, integers only: ``levels`` are the quantised priors (int64 [n]), ``scale64`` = 64 * scale.  floor(scale * m) is
    ``(scale64 * m) // 64``.  -> (xhat uint8 [n], iterations, marginals int64 [n] of the last executed sweep, 0 if none)."""
    V = vmax_of(bits)
    levels = np.asarray(levels, dtype=np.int64)
    assert levels.ndim == 1 and (np.abs(levels) <= V).all()
    rows = [np.flatnonzero(g.chk == c) for c in range(g.m)]  # edges of each check, ascending edge (= variable) order
    x_hat = np.zeros(g.n, dtype=np.uint8) if y is None else np.asarray(y).astype(np.uint8).copy()
    soft = np.zeros(g.n, dtype=np.int64)
    v2c = levels[g.var].copy()
    it = 0
    while not (0 < max_iter <= it):
        if early and (it > 0 or y is not None):
            synd = np.zeros(g.m, dtype=np.int64)
            np.add.at(synd, g.chk, x_hat[g.var].astype(np.int64))
            if not (synd % 2).any():
                break
        c2v = np.zeros(g.E, dtype=np.int64)
        for e in rows:
            v = v2c[e]
            parity = int((v < 0).sum()) & 1
            mags = np.minimum(np.abs(v), V)
            for j in range(len(e)):
                others = np.delete(mags, j)
                m = int(others.min()) if len(others) else V      # an empty minimum saturates
                mag = max((scale64 * m) // 64 - offset, 0)
                neg = parity ^ int(v[j] < 0)                     # row parity / own sign, sgn(0) = +1
                c2v[e[j]] = -mag if neg else mag
        marginal = levels.copy()
        np.add.at(marginal, g.var, c2v)
        v2c = marginal[g.var] - c2v
        x_hat = (marginal < 0).astype(np.uint8)
        soft = marginal
        it += 1
    return x_hat, it, soft

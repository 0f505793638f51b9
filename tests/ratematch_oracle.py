"""CPU restatement of a transmission pattern -- what ``ratematch.Pattern``, ``ldpc_channel_pattern`` over the BSC and
``ldpc_count_errors_pattern`` must reproduce exactly.

TEST INFRASTRUCTURE ONLY, written from the contract in include/ldpc_hip.h (the punctured / shortened block), not from the kernels.
Everything here is integers (the BSC's one float, its LLR, is computed as the library computes it and compared with ``==``).
"""
import math

import numpy as np

import bp_oracle as O

SENT, PUNCTURED, SHORTENED = 0, 1, 2


def kind_of(n, punctured=(), shortened=()):
    """The pattern rules: one byte per variable; both sets inside 0 .. n - 1 and disjoint, else ValueError."""
    p, s = sorted(set(int(v) for v in punctured)), sorted(set(int(v) for v in shortened))
    for v in p + s:
        if not 0 <= v < n:
            raise ValueError("variable %d outside 0 .. %d" % (v, n - 1))
    if set(p) & set(s):
        raise ValueError("a variable is both punctured and shortened")
    kind = np.zeros(n, dtype=np.uint8)
    kind[p] = PUNCTURED
    kind[s] = SHORTENED
    return kind


def parse(spec, n):
    """Comma-separated indices and half-open ranges a:b -> sorted list of indices."""
    out = set()
    for part in spec.split(","):
        if ":" in part:
            a, b = part.split(":")
            a, b = int(a), int(b)
            if not 0 <= a < b <= n:
                raise ValueError(part)
            out.update(range(a, b))
        else:
            if not 0 <= int(part) < n:
                raise ValueError(part)
            out.add(int(part))
    return sorted(out)


def peel(g, kind):
    """Variables left erased when exactly the punctured ones start erased and a check with one erased variable resolves it."""
    erased = set(int(v) for v in np.flatnonzero(np.asarray(kind) == PUNCTURED))
    rows = [[] for _ in range(g.m)]
    for c, v in zip(np.asarray(g.chk), np.asarray(g.var)):
        rows[int(c)].append(int(v))
    moved = True
    while moved and erased:
        moved = False
        for r in rows:
            e = [v for v in r if v in erased]
            if len(e) == 1:
                erased.discard(e[0])
                moved = True
    return sorted(erased)


def bsc_threshold(p):
    """flip <=> (w + 0.5) * 2^-32 < p <=> w < ceil(p * 2^32 - 0.5)"""
    return max(int(np.ceil(p * 4294967296.0 - 0.5)), 0)


def philox_words(seed, stream, frame0, B, n):
    """uint64 [B, n]: word v of frame frame0 + f is word v & 3 of Philox block v >> 2 of that frame (``bp_oracle.philox_frame_words``)."""
    return np.stack([O.philox_frame_words(seed, stream, frame0 + f, n).astype(np.uint64) for f in range(B)])


def bsc_pattern(p, sent, codeword, kind, short_llr, seed, stream, frame0, B, dtype, words=None):
    """-> (priors [B, n] in ``dtype``, y uint8 [B, n]).  Word q of Philox block j of a frame belongs to variable 4 j + q of the MOTHER code.
    ``words``: ``philox_words(seed, stream, frame0, B, n)`` where a caller has them already."""
    kind = np.asarray(kind)
    n = kind.size
    thr = bsc_threshold(p)
    llr = dtype(math.log(1.0 - p) - math.log(p))  # libm's log, as the library's host code
    y = np.zeros((B, n), dtype=np.uint8)
    pri = np.zeros((B, n), dtype=dtype)
    words = philox_words(seed, stream, frame0, B, n) if words is None else words
    for f in range(B):
        w = words[f]
        bit = np.full(n, codeword, dtype=np.uint8) if sent is None else np.asarray(sent[f], dtype=np.uint8)
        s = bit ^ (w < np.uint64(thr)).astype(np.uint8)
        y[f] = np.where(kind == SENT, s, 0)
        pri[f] = np.where(kind == SENT, llr * (1 - 2 * s.astype(np.int64)).astype(dtype), np.where(kind == PUNCTURED, dtype(0), dtype(short_llr)))
    return pri, y


def tally(xhat, sent, codeword, kind, iters, hist_bins):
    """The masked counters int64 [4 + hist_bins]: tot, wec, bec, iter_sum, hist[min(iters, bins - 1)]; errors over kind != 2."""
    xhat = np.asarray(xhat)
    want = np.full_like(xhat, codeword) if sent is None else np.asarray(sent)
    err = ((xhat != want) & (np.asarray(kind) != SHORTENED)[None, :]).sum(axis=1)
    out = np.zeros(4 + hist_bins, dtype=np.int64)
    out[0], out[1], out[2] = xhat.shape[0], (err > 0).sum(), err.sum()
    if iters is not None:
        out[3] = np.asarray(iters, dtype=np.int64).sum()
        if hist_bins:
            out[4:] = np.bincount(np.minimum(np.asarray(iters), hist_bins - 1), minlength=hist_bins)
    return out

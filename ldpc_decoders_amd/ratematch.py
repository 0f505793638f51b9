"""Transmission patterns: which bits of the mother code's codeword are sent (no upstream counterpart: the reference sends every bit).

A deployed system punctures bits -- codeword bits that are not transmitted; the decoder starts them from a prior of 0 -- and shortens
bits -- filler bits known to be 0 that are not transmitted either; the decoder starts them from a large positive prior.  ``Pattern`` holds
one byte per variable, ``kind[n]``: 0 sent, 1 punctured, 2 shortened.  Host only (numpy); the device side is ``ldpc_channel_pattern`` /
``ldpc_count_errors_pattern`` (csrc/ldpc_ratematch.hip) and ``_device.PatternHandle``, which composes them with any LLR decoder's handle.

SNR convention: the channel parameter means what it means without a pattern, PER TRANSMITTED SYMBOL (``sigma^2 = 10^(-snr/10)``,
src/biawgn.py:10).  No rate correction is applied: a curve of a punctured code is drawn over the same Es/N0 axis as its mother code's.

Counting: a punctured bit is a codeword bit and its errors count; a shortened bit is known and is left out, so the bit error rate of a
pattern is ``bec / (tot * n_counted)`` with ``n_counted = n - #shortened``.
"""
import numpy as np

from .codes import Code

SENT, PUNCTURED, SHORTENED = 0, 1, 2
SHORT_LLR = 32.0  # a power of two (exact on every prior grid and under the quantisers), below the |v| ~ 38.2 from where fp64 tanh(v / 2) is 1.0


def _indices(what, idx, n):
    a = np.asarray(list(idx) if not isinstance(idx, np.ndarray) else idx)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("%s: a list of variable indices" % what)
    a = np.unique(a.astype(np.int64))
    if a[0] < 0 or a[-1] >= n:
        raise ValueError("%s: variable %d is outside 0 .. %d" % (what, a[0] if a[0] < 0 else a[-1], n - 1))
    return a


def parse(spec, n):
    """The command-line form -> sorted int64 indices: comma-separated indices and half-open ranges ``a:b``, e.g. ``0:54,600,1100:1200``.
    ValueError for anything else, an empty or reversed range, or an index outside 0 .. n - 1."""
    out = []
    for part in str(spec).split(","):
        part = part.strip()
        try:
            if ":" in part:
                a, b = (int(t) for t in part.split(":"))
                if not 0 <= a < b <= n:
                    raise ValueError
                out.append(np.arange(a, b, dtype=np.int64))
            else:
                v = int(part)
                if not 0 <= v < n:
                    raise ValueError
                out.append(np.array([v], dtype=np.int64))
        except ValueError:
            raise ValueError("pattern spec %r: %r is neither an index nor a half-open range a:b inside 0 .. %d" % (spec, part, n))
    return np.unique(np.concatenate(out))


def spec_of(indices):
    """The canonical spec string of a set of indices (``parse`` gives them back): maximal runs as ``a:b``, single indices as ``a``."""
    a = np.unique(np.asarray(indices, dtype=np.int64))
    if a.size == 0:
        return ""
    cuts = np.flatnonzero(np.diff(a) != 1) + 1
    runs = np.split(a, cuts)
    return ",".join(str(r[0]) if r.size == 1 else "%d:%d" % (r[0], r[-1] + 1) for r in runs)


def block_columns(cols, Z):
    """The variables of whole block columns of a quasi-cyclic code of lifting size Z: column j is j Z .. (j + 1) Z - 1."""
    c = np.unique(np.asarray(list(cols), dtype=np.int64))
    if int(Z) != Z or Z < 1 or (c.size and c[0] < 0):
        raise ValueError("block columns are non-negative integers and Z >= 1")
    return (c[:, None] * int(Z) + np.arange(int(Z), dtype=np.int64)[None, :]).ravel()


class Pattern:
    """``Pattern(n, punctured=(), shortened=())``: ``kind`` uint8 [n] with 0 sent, 1 punctured, 2 shortened.  The two sets must be disjoint
    and inside 0 .. n - 1 (ValueError)."""

    def __init__(self, n, punctured=(), shortened=()):
        self.n = int(n)
        if self.n < 1:
            raise ValueError("a pattern needs n >= 1 variables")
        self.punctured = _indices("punctured", punctured, self.n)
        self.shortened = _indices("shortened", shortened, self.n)
        both = np.intersect1d(self.punctured, self.shortened)
        if both.size:
            raise ValueError("variable %d is both punctured and shortened" % both[0])
        self.kind = np.zeros(self.n, dtype=np.uint8)
        self.kind[self.punctured] = PUNCTURED
        self.kind[self.shortened] = SHORTENED
        self._short = None   # (code, its shortened code, index map) of the last shortened_code call

    @property
    def n_tx(self):
        return self.n - self.punctured.size - self.shortened.size

    @property
    def n_counted(self):
        return self.n - self.shortened.size

    @property
    def empty(self):
        return self.n_tx == self.n

    @property
    def puncture_spec(self):
        return spec_of(self.punctured)

    @property
    def shorten_spec(self):
        return spec_of(self.shortened)

    def unrecoverable(self, code):
        """Peel with exactly the punctured variables erased (a check with one erased variable resolves it) -> the sorted int64 residual.
        Not empty: the punctured set contains a stopping set, and no BP decoder can ever move those bits off a prior of 0."""
        self._check(code)
        erased = self.kind == PUNCTURED
        chk, var = np.asarray(code.edge_chk, dtype=np.int64), np.asarray(code.edge_var, dtype=np.int64)
        while erased.any():
            on = erased[var]
            cnt = np.bincount(chk[on], minlength=code.m)
            solved = var[on & (cnt[chk] == 1)]
            if solved.size == 0:
                break
            erased[solved] = False
        return np.flatnonzero(erased).astype(np.int64)

    def shortened_code(self, code):
        """-> (the ``Code`` with the shortened columns deleted, n' = n - #shortened; int64 [n'] index map from its columns to those of
        ``code``).  Checks left with degree 0 or 1 are allowed: only the encoder sees this code.  Kept on the pattern."""
        self._check(code)
        if self._short is None or self._short[0] is not code:
            keep = np.flatnonzero(self.kind != SHORTENED).astype(np.int64)
            new = np.full(self.n, -1, dtype=np.int64)
            new[keep] = np.arange(keep.size)
            var = np.asarray(code.edge_var, dtype=np.int64)
            on = new[var] >= 0
            short = Code.from_edges(code.m, keep.size, np.asarray(code.edge_chk)[on], new[var[on]])
            self._short = (code, short, keep)
        return self._short[1], self._short[2]

    def _check(self, code):
        if code.n != self.n:
            raise ValueError("a pattern of %d variables on a code of %d" % (self.n, code.n))


def from_args(args, code):
    """The pattern of a command line (``--puncture --shorten --puncture-cols --shorten-cols``), or None when none of them is given.
    The block-column flags take Z from ``--qc-lift`` / ``qc.resolve``."""
    specs = [getattr(args, k, None) for k in ("puncture", "shorten", "puncture_cols", "shorten_cols")]
    if all(s is None for s in specs):
        return None
    n = code.n
    sets = [parse(s, n) if s is not None else np.zeros(0, dtype=np.int64) for s in specs[:2]]
    if specs[2] is not None or specs[3] is not None:
        from . import qc

        Z = qc.resolve(code, getattr(args, "qc_lift", 0) or 0)[1]
        for i, s in enumerate(specs[2:]):
            if s is not None:
                sets[i] = np.union1d(sets[i], _indices("block columns", block_columns(parse(s, n // Z), Z), n))
    return Pattern(n, sets[0], sets[1])

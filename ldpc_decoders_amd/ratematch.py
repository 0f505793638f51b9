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


HARQ_MAX_TX = 16    # transmissions of one schedule (csrc/ldpc_harq.hpp)
HARQ_MAX_COPIES = 255  # of one variable over a whole schedule: the tables are bytes


def rv_starts(Ncb, T, Z=1):
    """Starts that step through the buffer in the order 0, 2, 3, 1 quarters: ``floor((0, 2, 3, 1)[t mod 4] * Ncb / 4)`` rounded down to a
    multiple of ``Z``.  A rule, not a standard's table."""
    Ncb, T, Z = int(Ncb), int(T), int(Z)
    if Ncb < 1 or T < 1 or Z < 1:
        raise ValueError("rv_starts needs Ncb >= 1, T >= 1 and Z >= 1")
    return tuple(((0, 2, 3, 1)[t % 4] * Ncb // 4) // Z * Z for t in range(T))


def _int_list(what, values):
    try:
        out = tuple(int(v) for v in values)
        if any(float(v) != int(v) for v in values):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("%s: a list of integers" % what)
    return out


def parse_ints(what, spec):
    """The command-line form of ``--harq-bits`` / ``--harq-starts``: comma-separated non-negative integers, e.g. ``800,800,400``."""
    parts = [p.strip() for p in str(spec).split(",")]
    if not parts or any(not p.isdigit() for p in parts):
        raise ValueError("%s %r: comma-separated non-negative integers" % (what, spec))
    return tuple(int(p) for p in parts)


class Harq:
    """``Harq(pattern, tx_bits, starts=None)``: an incremental-redundancy schedule over the circular buffer of ``pattern``.

    The buffer is the variables of kind 0 in ascending index, ``Ncb = pattern.n_tx`` of them (kind 1, punctured, now reads "never in the
    buffer"; kind 2, shortened, is as before).  Transmission ``t`` of ``T = len(tx_bits)`` (1 .. 16) sends the buffer positions
    ``(starts[t] + i) mod Ncb`` for ``i = 0 .. tx_bits[t] - 1``; ``tx_bits[t] > Ncb`` repeats bits.  ``starts`` defaults to all 0: Chase
    combining.  ``cnt`` and ``first``, uint8 [T, n], are what the device reads: the copies of every variable in transmission ``t`` and in
    all transmissions before it (0 outside the buffer).  ValueError for a variable with more than 255 copies over the schedule."""

    def __init__(self, pattern, tx_bits, starts=None):
        self.pattern, self.n, self.Ncb = pattern, pattern.n, int(pattern.n_tx)
        if self.Ncb < 1:
            raise ValueError("the circular buffer is empty: every variable is punctured or shortened")
        self.tx_bits = _int_list("tx_bits", tx_bits)
        self.T = len(self.tx_bits)
        if not 1 <= self.T <= HARQ_MAX_TX or min(self.tx_bits) < 1:
            raise ValueError("a schedule has 1 .. %d transmissions of at least one bit each" % HARQ_MAX_TX)
        self.starts = (0,) * self.T if starts is None else _int_list("starts", starts)
        if len(self.starts) != self.T or min(self.starts) < 0 or max(self.starts) >= self.Ncb:
            raise ValueError("one start per transmission, each inside the buffer 0 .. %d" % (self.Ncb - 1))
        self.buffer = np.flatnonzero(pattern.kind == SENT).astype(np.int64)
        pos = np.arange(self.Ncb, dtype=np.int64)
        total = np.zeros(self.Ncb, dtype=np.int64)
        cnt = np.zeros((self.T, self.n), dtype=np.int64)
        first = np.zeros((self.T, self.n), dtype=np.int64)
        for t, (E, k) in enumerate(zip(self.tx_bits, self.starts)):
            d = (pos - k) % self.Ncb
            c = np.where(d >= E, 0, 1 + (E - 1 - d) // self.Ncb)
            cnt[t, self.buffer], first[t, self.buffer] = c, total
            total += c
        if total.max() > HARQ_MAX_COPIES:
            raise ValueError("variable %d is sent %d times over the schedule; the tables hold at most %d copies"
                             % (self.buffer[int(total.argmax())], total.max(), HARQ_MAX_COPIES))
        self.cnt, self.first = cnt.astype(np.uint8), first.astype(np.uint8)

    def copies(self, t, p):
        """Copies of buffer position ``p`` in transmission ``t``."""
        d = (int(p) - self.starts[t]) % self.Ncb
        return 0 if d >= self.tx_bits[t] else 1 + (self.tx_bits[t] - 1 - d) // self.Ncb

    def first_copy(self, t, p):
        """Copies of buffer position ``p`` in the transmissions before ``t``: the ordinal of the first copy of transmission ``t``."""
        return sum(self.copies(u, p) for u in range(t))

    @property
    def bits_spec(self):
        return ",".join(str(E) for E in self.tx_bits)

    @property
    def starts_spec(self):
        return ",".join(str(k) for k in self.starts)


def harq_from_args(args, pattern):
    """The schedule of a command line (``--harq-bits E0,E1,..`` with ``--harq-starts k0,k1,..`` or ``rv``) over ``pattern``, or None without
    ``--harq-bits``.  ``rv`` takes Z from ``--qc-lift`` (1 when that is 0)."""
    bits, starts = getattr(args, "harq_bits", None), getattr(args, "harq_starts", None)
    if bits is None:
        if starts is not None:
            raise ValueError("--harq-starts needs --harq-bits")
        return None
    bits = parse_ints("--harq-bits", bits)
    if starts is not None:
        starts = rv_starts(pattern.n_tx, len(bits), getattr(args, "qc_lift", 0) or 1) if starts == "rv" else parse_ints("--harq-starts", starts)
    return Harq(pattern, bits, starts)


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

"""Deterministic codes and LLR batches at the check degrees, variable degrees and sizes where the ADMM decoder (csrc/ldpc_admm.hip) changes
kernel, and the tests' own statement of which kernel a code must reach.

TEST INFRASTRUCTURE ONLY (no tests in here).  numpy ``RandomState`` seeds throughout, so that test_admm_codes_cpu.py can hold the builders,
the expected dispatch and the exercise conditions on the CPU before test_gpu_admm_degrees.py compares the device with the C oracle.
"""
import numpy as np

from ldpc_decoders_amd import codes
from ldpc_decoders_amd.codes import Code

SEED = 4100
MU, EPS, MAX_ITER, B = 3.0, 1e-5, 100, 130  # the defaults of every case: two full tiles of 64 frames and a ragged third


class Graph:
    """What oracle/admm_oracle.py reads of a code."""

    def __init__(self, code):
        self.m, self.n, self.chk, self.var = code.m, code.n, code.edge_chk, code.edge_var


def check_degrees(code):
    return np.bincount(code.edge_chk, minlength=code.m)


def var_degrees(code):
    return np.bincount(code.edge_var, minlength=code.n)


# ---- builders -------------------------------------------------------------------------------------------------------------------------

def rows_code(degrees, n, seed):
    """Check i has ``degrees[i]`` distinct variables drawn uniformly among the n (0: an empty row)."""
    rng = np.random.RandomState(seed)
    rows = [np.sort(rng.choice(n, int(d), replace=False)) for d in degrees]
    chk = np.repeat(np.arange(len(rows)), [len(r) for r in rows])
    return Code.from_edges(len(rows), n, chk.astype(np.int32), np.concatenate(rows).astype(np.int32))


def regular_code(n, l, r, seed):
    """(l, r)-regular: every variable in l checks, every check of r variables (r divides n)."""
    assert n % r == 0
    return codes.rand_reg_ldpc(n, l, r, np.random.RandomState(seed))


def dc6_code(m, n, seed):
    """Every check has six distinct variables, every variable one, two or three checks (all three when n = 2 m); 2 m <= n <= 6 m.
    The 6 m sockets of the variables are shuffled and dealt six to a check; a check that holds a variable twice then trades one of the two
    sockets with a socket of another check, drawn until neither check repeats a variable."""
    assert 2 * m <= n <= 6 * m
    rng = np.random.RandomState(seed)
    extra = 6 * m - n                      # edges beyond one per variable: three-fold variables take two of them, two-fold ones one
    three = max(extra - n, extra // 3)
    two = extra - 2 * three
    deg = np.ones(n, dtype=np.int64)
    deg[:three] = 3
    deg[three:three + two] = 2
    deg = deg[rng.permutation(n)]
    sock = np.repeat(np.arange(n), deg)[rng.permutation(6 * m)].reshape(m, 6)
    while True:
        bad = [c for c in range(m) if len(set(sock[c])) < 6]
        if not bad:
            break
        for c in bad:
            row = list(sock[c])
            for j in range(6):
                if row[j] not in row[:j]:
                    continue
                while True:  # a partner socket such that both rows end up without a repeat
                    c2, j2 = int(rng.randint(m)), int(rng.randint(6))
                    if c2 == c or sock[c2, j2] in row:
                        continue
                    if row[j] in np.delete(sock[c2], j2):
                        continue
                    sock[c, j], sock[c2, j2] = sock[c2, j2], sock[c, j]
                    row = list(sock[c])
                    break
    return Code.from_edges(m, n, np.repeat(np.arange(m), 6).astype(np.int32), sock.ravel().astype(np.int32))


# ---- the expected dispatch ----------------------------------------------------------------------------------------------------------------

def _split(E):
    """Blocks of numpy's pairwise sum of E elements, left to right, as (length, depth below the root): a piece of more than 128 elements is
    cut in two, the left part half of it rounded down to a multiple of 8."""
    todo, out = [(int(E), 0)], []
    while todo:
        n, depth = todo.pop()
        if n <= 128:
            out.append((n, depth))
        else:
            left = (n // 2) // 8 * 8
            todo.append((n - left, depth + 1))  # popped second: blocks come out left to right
            todo.append((left, depth + 1))
    return out


def blocks_of(E):
    return [n for n, _ in _split(E)]


def leaves_of(E):
    return len(_split(E))


LDS_BYTES = 160 * 1024


def lds_plan(code):
    """None where a decode must run on the streaming kernels, else (waves per frame, checks per lane) of the LDS-resident kernel: codes
    whose checks all have six edges and whose variables have one to three; at least 128 checks (a frame must fill a workgroup); four waves up
    to 256 checks, eight up to 512, eight in two passes up to 1024; two variables per lane (three in the two-pass form); one lane per
    accumulator chain of the stopping sums, eight chains per block and two sums; the frame's state within 160 KiB of LDS."""
    dc, dv = check_degrees(code), var_degrees(code)
    if dc.min() != 6 or dc.max() != 6 or dv.min() < 1 or dv.max() > 3 or code.m < 128 or code.m > 1024:
        return None
    nw = 4 if code.m <= 256 else 8
    cpl = 1 if code.m <= 512 else 2
    lanes = 64 * nw
    if code.n > lanes * (2 if cpl == 1 else 3):
        return None
    blocks = _split(code.E)
    leaves, levels = len(blocks), max(d for _, d in blocks)
    if 2 * 8 * leaves > lanes:
        return None
    nodes = 2 * leaves - 1
    doubles = 5 * code.E + code.n + 2 * 8 * leaves + max(2 * nodes, 64)  # z, lambda, lambda / mu, two distance vectors; x; chains; the tree
    ints = 2 * nodes + levels + 1 + 2 * leaves                           # the schedule of the tree and the blocks
    if 8 * doubles + 64 + 4 * ints + 16 > LDS_BYTES:
        return None
    return nw, cpl


def z_kernel_of(code):
    """The z-update kernel of the streaming path: register-only for one check degree in 2..8, work arrays in the LDS for unequal degrees up
    to 8 (and a uniform degree below 2), private work arrays for degrees 9..16."""
    dc = check_degrees(code)
    lo, hi = int(dc.min()), int(dc.max())
    if hi > 16:
        raise ValueError("check degree %d above 16" % hi)
    if lo == hi and 2 <= hi <= 8:
        return "fixed<%d>" % hi
    return "lds_arrays<8>" if hi <= 8 else "private<16>"


# ---- LLR batches --------------------------------------------------------------------------------------------------------------------------

PLANTED = {"zero": 1, "plus": 2, "minus": 3, "alternating": 4, "grid": 5, "inf": 6}  # row of each (frame 0 stays a noise frame)


def planted_gamma(code, rng, B, snr_db):
    """BI-AWGN LLRs [B, n] of the all-zero word (sent as -1: gamma = -2 y / sigma^2 > 0 without noise), rows PLANTED overwritten as far as B
    reaches: all 0.0 (every projection input a tie at 0.5); all +1e6; all -1e6; +1e6 / -1e6 alternating; the row's own LLRs rounded to
    multiples of 0.75 (many equal values: the stable sort order and the ties of the break-point merge matter); +inf / -inf by the sign of the
    row's own LLRs."""
    var = 10.0 ** (-snr_db / 10.0)
    g = -2.0 * (-1.0 + rng.normal(0.0, np.sqrt(var), (B, code.n))) / var
    alt = np.where(np.arange(code.n) % 2 == 0, 1e6, -1e6)
    rows = {"zero": lambda r: np.zeros(code.n), "plus": lambda r: np.full(code.n, 1e6), "minus": lambda r: np.full(code.n, -1e6),
            "alternating": lambda r: alt, "grid": lambda r: np.round(r / 0.75) * 0.75, "inf": lambda r: np.where(r < 0, -np.inf, np.inf)}
    for name, f in PLANTED.items():
        if f < B:
            g[f] = rows[name](g[f].copy())
    return np.ascontiguousarray(g)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# name -> (builder, snr_db); every GPU case and every CPU exercise condition goes through case_code / case_gamma, so both see the same bits

UNIFORM = {2: (96, 1, 2), 3: (96, 2, 3), 4: (96, 2, 4), 5: (100, 3, 5), 6: (96, 3, 6), 7: (98, 3, 7), 8: (96, 3, 8)}  # L -> (n, l, r)
CYCLE_0_8 = [(i + 1) % 9 for i in range(45)]                 # 1..8, 0, 1..8, 0, ...: empty rows inside and as the last row
CYCLE_1_16 = [1 + i % 16 for i in range(64)]
E_EDGES = [1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 257, 263]
LDS_SHAPES = [(127, 300), (128, 256), (128, 512), (129, 400), (256, 512), (128, 513), (257, 514), (257, 1024), (512, 1024), (257, 1025),
              (513, 1026), (513, 1536), (513, 1537)]
LDS_ALL_DV3 = [(128, 256), (256, 512), (257, 514), (512, 1024), (513, 1026)]


def edge_degrees(E):
    """Check degrees <= 4 adding up to E: 4, 3, 2, 1 in turn, the last check takes what is left."""
    out = []
    while sum(out) < E:
        out.append(min((4, 3, 2, 1)[len(out) % 4], E - sum(out)))
    return out


def edge_tail(E):
    """How many of the last edges of an E-edge code are single-edge checks on variables of their own: the elements that the last block of the
    stopping sums adds one by one behind its eight accumulators (all of a block below eight), as far as four edges are left for the rest."""
    t = blocks_of(E)[-1] % 8
    return t if E == 1 else min(t, max(E - 4, 0))


def edge_code(E, seed):
    """E edges in checks of degree <= 4 on at most 90 variables.  The last edge_tail(E) edges are ISOLATED: a check of one variable that is in no
    other check.  Such an edge is a scalar recursion of its own (z = 0, x <- clip(-lambda / mu - gamma / mu)): with gamma = -mu (k + 1/2) on
    its variable and +1e6 on all others it keeps (x - z)^2 >= 1/4 for k + 1 iterations while every other edge is exactly 0 from the second
    iteration on -- the frame ends when THAT element of the sum says so (tail_rows).  -> Code with .tail_vars"""
    t = edge_tail(E)
    body = edge_degrees(E - t)
    n_body = int(min(83, max(6, E // 3 + 5))) if body else 5
    rng = np.random.RandomState(seed)
    rows = [np.sort(rng.choice(n_body, d, replace=False)) for d in body] + [np.array([n_body + j]) for j in range(t)]
    chk = np.repeat(np.arange(len(rows)), [len(r) for r in rows])
    code = Code.from_edges(len(rows), n_body + t, chk.astype(np.int32), np.concatenate(rows).astype(np.int32))
    code.tail_vars = np.arange(n_body, n_body + t)
    return code


TAIL_ROW0 = 7  # the first row behind PLANTED


def tail_rows(code):
    """One LLR row per isolated edge j: +1e6 everywhere, -mu (10.5 + j) on its variable -- the frame leaves at iteration 12 + j by that
    edge alone."""
    g = np.full((len(code.tail_vars), code.n), 1e6)
    g[np.arange(len(code.tail_vars)), code.tail_vars] = -MU * (10.5 + np.arange(len(code.tail_vars)))
    return g


def lds_mstar():
    """The largest m whose (m, 1536) code of six-edge checks still has one lane per accumulator chain in eight waves: at most 32 blocks."""
    return max(m for m in range(513, 1025) if leaves_of(6 * m) <= 32)


def _build(name):
    kind, _, arg = name.partition(":")
    seed = SEED + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    if kind == "uniform":
        n, l, r = UNIFORM[int(arg)]
        return regular_code(n, l, r, seed)
    if kind == "regular":
        n, l, r = (int(t) for t in arg.split(","))
        return regular_code(n, l, r, seed)
    if kind == "rows":
        table = {"cycle0_8": (CYCLE_0_8, 60), "all1": ([1] * 5, 8), "one_edge": ([1], 3), "7_8": ([7, 8] * 12, 70),
                 "cycle1_16": (CYCLE_1_16, 120), "9_16": ([9, 16] * 10, 110), "deg17": ([17, 3, 3], 40), "deg16": ([16, 3, 3], 40)}
        return rows_code(table[arg][0], table[arg][1], seed)
    if kind == "E":
        return edge_code(int(arg), seed)
    if kind == "dc6":
        m, n = (int(t) for t in arg.split(","))
        return dc6_code(m, n, seed)
    raise KeyError(name)


_CODES = {}


def case_code(name):
    if name not in _CODES:
        _CODES[name] = _build(name)
    return _CODES[name]


def case_snr(name):
    """3 dB; the six-edge codes 2.6 dB where every variable has three checks and 4 dB where n > 2 m (variables of one and two checks)."""
    if name.startswith("dc6:"):
        m, n = (int(t) for t in name[4:].split(","))
        return 2.6 if n == 2 * m else 4.0
    return 3.0


def case_gamma(name, B=B):
    """planted_gamma of the case; the E-edge codes also hold tail_rows from row TAIL_ROW0 on."""
    seed = SEED + 7 + sum(ord(ch) * (i + 3) for i, ch in enumerate(name))
    code = case_code(name)
    g = planted_gamma(code, np.random.RandomState(seed), B, case_snr(name))
    if name.startswith("E:"):
        t = tail_rows(code)
        assert TAIL_ROW0 + len(t) <= B
        g[TAIL_ROW0:TAIL_ROW0 + len(t)] = t
    return g


def lds_names():
    """The shapes of the LDS-resident kernel: LDS_SHAPES, the last pair of n = 1536 codes on each side of the 160 KiB rule (LDS_LAST_M) and
    the pair at lds_mstar(), which that rule has already sent to the streaming kernels."""
    ms = lds_mstar()
    return ["dc6:%d,%d" % s for s in LDS_SHAPES + [(LDS_LAST_M, 1536), (LDS_LAST_M + 1, 1536), (ms, 1536), (ms + 1, 1536)]]


LDS_LAST_M = 606  # 240 m + 18256 bytes at n = 1536 and 32 blocks: 606 is the last m within 160 KiB (test_admm_codes_cpu.py holds this)
REPACK_B = 64 * 6 + 5
DEGENERATE = ("rows:all1", "rows:one_edge", "E:1")  # no check above degree 1: every projection is 0, a frame is n scalar recursions


def decode_cases():
    """(name, B, max_iter) of every case that test_gpu_admm_degrees.py decodes with a cap of at least 60 iterations."""
    out = [("uniform:%d" % L, B, MAX_ITER) for L in sorted(UNIFORM)]
    out += [(nm, B, MAX_ITER) for nm in ("rows:cycle0_8", "rows:all1", "rows:one_edge", "rows:7_8", "regular:99,3,9", "regular:96,4,16",
                                         "rows:cycle1_16", "rows:9_16", "rows:deg16")]
    out += [("E:%d" % e, 70, 60) for e in E_EDGES]
    out += [(nm, B, MAX_ITER) for nm in lds_names()]
    out += [("rows:cycle1_16", REPACK_B, MAX_ITER)]
    return out


_ORACLE = {}


def oracle_of(name, B=B, max_iter=MAX_ITER):
    """(x, iters, converged) of the C oracle on case_gamma(name, B): computed once, shared by the tests, never written to."""
    import admm_oracle as A

    key = (name, B, max_iter)
    if key not in _ORACLE:
        out = A.admm_decode(Graph(case_code(name)), case_gamma(name, B), MU, EPS, max_iter)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def edge_cases():
    """The cases captured from the reference's ADMM class on GOLDEN_CODES (oracle/make_goldens_admm.py --edge)."""
    import json
    import os

    from helpers import GOLDEN

    with open(os.path.join(GOLDEN, "admm_edge_cases.json")) as fp:
        return json.load(fp)


def edge_arrays(case):
    import os

    from helpers import GOLDEN

    z = np.load(os.path.join(GOLDEN, "admm_edge_vectors.npz"))
    return {k[len(case["tag"]) + 1:]: z[k] for k in z.files if k.startswith(case["tag"] + "_")}


GOLDEN_CODES = ["uniform:3", "uniform:7", "rows:cycle0_8", "rows:cycle1_16", "dc6:128,512"]  # captured from the reference's ADMM class

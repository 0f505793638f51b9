"""A deterministic family of small codes at the word, lane and row-block edges of the GF(2) elimination kernels (csrc/ldpc_bec_ml.hip,
csrc/ldpc_osd.hip), and the input batches the device tests run on them.

TEST INFRASTRUCTURE ONLY (no tests in here).  Everything is drawn from numpy ``RandomState`` seeds, never from device noise, so that
test_edge_codes_cpu.py can assert what a batch holds (planted rows, frames the solver lists and frames it passes through, both sides of
the 32 KiB rule) before test_gpu_elimination_edges.py / test_gpu_chunk_crossing.py compare the device with the statements on it.
"""
import numpy as np

import osd_oracle as OSD
from ldpc_decoders_amd.codes import Code

# (m, n, redundant): n and |R| at 31 / 32 / 33, 63 / 64 / 65, 127 / 128 / 129; m at 63 / 64 / 65 (KC 1 -> 2), 128 / 129; n a power of two
# (no padding keys in the sort of k_osd_solve); more rows than columns
SHAPES = [(9, 31, 3), (16, 32, 3), (17, 33, 3), (31, 63, 3), (32, 64, 3), (33, 65, 3), (63, 96, 3), (64, 127, 3), (65, 128, 3), (66, 129, 3),
          (129, 200, 3), (128, 256, 3), (70, 40, 40)]
LIMIT_BEC = (2048, 576, 577)  # n, accepted m, refused m of ldpc_bec_ml_create
LIMIT_OSD = (1536, 576, 577)  # the same of ldpc_osd_create
OVERFLOW = (256, 896, 897, 192)  # n, m whose all-erased frame fits 32 KiB, m whose all-erased frame does not, rows that are not redundant
SMALL_SLAB = 32 * 1024  # the first pass of k_bec_ml_solve
SEED = 20260


def _support_xor(rows):
    out = set()
    for r in rows:
        out ^= r
    return out


def edge_code(m, n, seed, redundant, isolated=1, degree_one=2):
    """m x n code: every variable has three distinct checks among the first m - redundant rows, except ``isolated`` variables (none) and
    ``degree_one`` variables (one); each of those rows has degree >= 2 (an edge of a regular variable is moved from a row that can spare it
    to a row that is short); the last ``redundant`` rows are GF(2) sums of two or three of the first rows, the first of them a copy of row
    0.  -> Code with ``.isolated`` / ``.degree_one`` (variable indices) and ``.base_rows`` = m - redundant."""
    rng = np.random.RandomState(seed)
    m0 = m - redundant
    assert m0 >= 3 and redundant >= 1 and n > isolated + degree_one
    special = rng.choice(n, isolated + degree_one, replace=False)
    iso, one = np.sort(special[:isolated]), np.sort(special[isolated:])
    checks = {}
    for v in range(n):
        if v in iso:
            checks[v] = set()
        else:
            checks[v] = set(int(c) for c in rng.choice(m0, 1 if v in one else 3, replace=False))
    rows = [set(v for v in range(n) if c in checks[v]) for c in range(m0)]
    for r in range(m0):  # repair: deterministic, ascending
        while len(rows[r]) < 2:
            moved = False
            for v in range(n):
                if len(checks[v]) != 3 or r in checks[v]:
                    continue
                donors = [c for c in sorted(checks[v]) if len(rows[c]) > 2]
                if donors:
                    c = donors[0]
                    checks[v].remove(c)
                    rows[c].remove(v)
                    checks[v].add(r)
                    rows[r].add(v)
                    moved = True
                    break
            assert moved, "no row can spare an edge"
    combos = [(0,)]
    while len(combos) < redundant:
        pick = tuple(int(c) for c in rng.choice(m0, 2 + int(rng.randint(2)), replace=False))
        if _support_xor([rows[c] for c in pick]):  # a sum that cancels to nothing is drawn again
            combos.append(pick)
    rows += [_support_xor([rows[c] for c in pick]) for pick in combos]
    chk = [c for c, r in enumerate(rows) for _ in r]
    var = [v for r in rows for v in sorted(r)]
    code = Code.from_edges(m, n, np.asarray(chk, dtype=np.int32), np.asarray(var, dtype=np.int32))
    code.isolated, code.degree_one, code.base_rows, code.combos = iso, one, m0, combos
    return code


def shape_code(m, n, redundant):
    return edge_code(m, n, SEED + 1000 * m + n, redundant)


def limit_code(m, n, seed=SEED):
    """Sparse random rows of weight 6: the pairs on each side of the create rules."""
    rng = np.random.RandomState(seed)
    var = np.concatenate([np.sort(rng.choice(n, 6, replace=False)) for _ in range(m)])
    return Code.from_edges(m, n, np.repeat(np.arange(m), 6).astype(np.int32), var.astype(np.int32))


def overflow_code(m):
    n, _, _, m0 = OVERFLOW
    return edge_code(m, n, SEED + m, m - m0)


# ---- ML over the BEC ----------------------------------------------------------------------------------------------------------------

def peel_batch(code, Y):
    """test_bec_ml_cpu.peel for a batch: Y [B, n] in {0, 1, 2} -> peeled words (2 on the residual set).  All frames at once, check by check;
    on codewords the result does not depend on the schedule."""
    X = np.array(Y, dtype=np.int64)
    H = code.parity_mtx.astype(np.int64)
    while True:
        er = (X == 2).astype(np.int64)
        cnt = er @ H.T
        if not (cnt == 1).any():
            return X
        for c in np.flatnonzero((cnt == 1).any(axis=0)):
            f = np.flatnonzero(((X == 2).astype(np.int64) @ H[c]) == 1)
            if not len(f):
                continue
            sub = X[f]
            e = np.argmax((sub == 2) & (H[c][None, :] == 1), axis=1)
            val = (np.where(sub == 2, 0, sub) @ H[c]) % 2
            X[f, e] = val


def lds_bytes_of(code, x):
    """bec_ml_lds_words * 4 of one peeled frame (csrc/ldpc_bec_ml.hpp): nc = |R|, rows = the checks that touch R."""
    R = x == 2
    nc, rows = int(R.sum()), int((code.parity_mtx[:, R].sum(axis=1) > 0).sum())
    W, S, RP = (code.n + 31) // 32, (nc + 32) // 32, -(-rows // 64) * 64
    return 4 * (3 * W + 3 * S + S * RP)


def _words(code, rng, B):
    return code.encoder().encode(rng.randint(0, 2, size=(B, code.encoder().k)))


def _erase(sent, rng, eps):
    return np.where(rng.random_sample(sent.shape) < eps, 2, sent).astype(np.uint8)


BEC_PLANTED = {"all": 0, "none": 1, "isolated": 2, "degree_one": 3}


def bec_batch(code, seed, B=192):
    """-> (sent [B, n], y [B, n] in {0, 1, 2}).  Rows 0-3: BEC_PLANTED; the rest in three equal parts at erasure rates around where peeling
    stops finishing (0.55, 0.8 and 1.05 of rank / n, the rate at which ML itself gives up)."""
    rng = np.random.RandomState(seed)
    sent = _words(code, rng, B)
    cap = code.encoder().rank / code.n
    eps = np.repeat([0.55 * cap, 0.8 * cap, min(1.05 * cap, 0.97)], -(-B // 3))[:B]
    y = _erase(sent, rng, eps[:, None])
    y[0] = 2
    y[1] = sent[1]
    y[2] = sent[2]
    y[2, code.isolated[0]] = 2
    y[3] = sent[3]
    y[3, code.degree_one[0]] = 2
    return sent, y


def inconsistent_batch(code, y, peeled, count=16):
    """``count`` listed frames of y with one unerased bit next to the residual set flipped so that the residual system has no solution.
    The bit is taken (ascending) among those whose every check either touches R or has no erasure at all, so no peeling step reads it
    and the peeled word is the old one with that bit flipped, whatever the schedule.  -> (y_bad, peeled_bad, frames flipped)"""
    from test_bec_ml_cpu import ml_statement

    H = code.parity_mtx.astype(np.int64)
    y_bad, p_bad, done = y.copy(), peeled.copy(), []
    for f in np.flatnonzero((peeled == 2).any(axis=1)):
        if len(done) == count:
            break
        R, era = (peeled[f] == 2).astype(np.int64), (y[f] == 2).astype(np.int64)
        touch, clean = (H @ R) > 0, (H @ era) == 0
        for v in np.flatnonzero(y[f] != 2):
            mine = H[:, v] == 1
            if not (touch & mine).any() or not (touch | clean)[mine].all():
                continue
            x = peeled[f].copy()
            x[v] ^= 1
            if ml_statement(code, x, np.zeros(code.n, dtype=np.int64))[1] == -1:
                y_bad[f, v] ^= 1
                p_bad[f] = x
                done.append(int(f))
                break
    return y_bad, p_bad, np.asarray(done, dtype=np.int64)


def overflow_batch(code, seed, B=64):
    """64 frames for the m = 897 code of the overflow pair: 12 all-erased frames (the only pattern whose system is above 32 KiB: they
    differ in their free bits), one erasure short of that, and the levels of bec_batch."""
    sent, y = bec_batch(code, seed, B)
    y[4:16] = 2
    for f in range(16, 24):
        y[f] = 2
        y[f, (f * 37) % code.n] = sent[f, (f * 37) % code.n]
    return sent, y


def limit_bec_batch(code, seed, B=8):
    rng = np.random.RandomState(seed)
    sent = _words(code, rng, B)
    y = _erase(sent, rng, np.linspace(0.2, 0.9, B)[:, None])
    y[0] = 2
    return sent, y


# ---- ordered-statistics post-processing -----------------------------------------------------------------------------------------------

def _awgn_llr(sent, rng, snr_db):
    sigma2 = 10.0 ** (-snr_db / 10.0)
    return 2.0 * ((1.0 - 2.0 * sent) + np.sqrt(sigma2) * rng.standard_normal(sent.shape)) / sigma2


def _snr_half(code, sent, seed):
    """The first SNR on a 0.5 dB grid at which at least 40 % of the hard decisions are codewords (same noise draws at every SNR)."""
    for snr in np.arange(-4.0, 20.5, 0.5):
        llr = _awgn_llr(sent, np.random.RandomState(seed), snr)
        if (code.syndrome((llr < 0).astype(np.int64)).sum(axis=1) == 0).mean() >= 0.4:
            return float(snr)
    raise AssertionError("no SNR on the grid")


OSD_PLANTED = {"zero": 0, "tie_a": 1, "tie_b": 2, "odd": 3}
OSD_FIRST_NOISE_ROW = 12


def osd_winners(code):
    """(row, t) of the frames of osd_batch whose cheapest candidate is number t by construction: t at the lane and round edges of the
    scoring loop of k_osd_solve (lane t & 63 of round t >> 6) and at |F|, as far as the code has free positions."""
    nf = code.n - code.encoder().rank
    ts = sorted(set(t for t in (2, 63, 64, 65, 127, 128, nf) if 2 <= t <= nf))
    return [(4 + i, t) for i, t in enumerate(ts)]


def osd_batch(code, seed, dtype, B=192):
    """-> (post [B, n], prior [B, n]) of ``dtype``.  prior: BI-AWGN LLRs on encoder words; post: the same scaled per variable by a factor in
    [0.5, 2].  Rows 0-3: OSD_PLANTED -- all post = 0 with one negative entry; two BSC-style rows where every |post| and |prior| is one
    value (in tie_b post and prior differ in sign at three places); a listed frame with +inf and NaN in post and in prior.  Rows 4 ...:
    osd_winners -- prior is a noiseless word with distinct magnitudes, post the same scaled with the isolated variable made the least
    reliable (free position 0) and the sign of free position t - 1 flipped: candidate t is the sent word at cost 0, every other costs more."""
    rng = np.random.RandomState(seed)
    n = code.n
    sent = _words(code, rng, B)
    snr = _snr_half(code, sent, seed + 1)
    prior = _awgn_llr(sent, np.random.RandomState(seed + 1), snr).astype(dtype)
    post = (prior * rng.uniform(0.5, 2.0, size=n).astype(dtype)[None, :]).astype(dtype)
    z = OSD_PLANTED["zero"]
    post[z] = 0
    post[z, n // 3] = -1.0
    for name, flips, extra in (("tie_a", 2, 0), ("tie_b", 3, 3)):
        f = OSD_PLANTED[name]
        bits = sent[f].copy()
        bits[rng.choice(n, flips, replace=False)] ^= 1
        prior[f] = (1.0 - 2.0 * bits) * 2.75
        pb = bits.copy()
        pb[rng.choice(n, extra, replace=False)] ^= 1
        post[f] = (1.0 - 2.0 * pb) * 2.75
    failed = np.flatnonzero(code.syndrome((post < 0).astype(np.int64)).sum(axis=1) != 0)
    src, o = failed[failed >= 4][0], OSD_PLANTED["odd"]
    post[o], prior[o] = post[src], prior[src]
    post[o, 1], post[o, n - 1], post[o, n // 4] = np.inf, np.inf, np.nan
    prior[o, 0], prior[o, n - 2], prior[o, n // 5] = np.inf, -np.inf, np.nan
    H = code.parity_mtx.astype(np.uint8)
    for f, t in osd_winners(code):
        prior[f] = ((1.0 - 2.0 * sent[f]) * rng.uniform(1.0, 3.0, size=n)).astype(dtype)
        post[f] = (prior[f] * rng.uniform(0.5, 2.0, size=n).astype(dtype)).astype(dtype)
        post[f, code.isolated[0]] = np.copysign(0.125, post[f, code.isolated[0]])
        pi, _, rowof = OSD.eliminate(H, post[f])
        post[f, pi[np.flatnonzero(rowof < 0)[t - 1]]] *= -1
    return np.ascontiguousarray(post), np.ascontiguousarray(prior)


def osd_listed(code, post):
    """Frames whose hard decisions (post < 0; NaN and 0 give 0) are no codeword: the ones the solver lists."""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(code.syndrome((post < 0).astype(np.int64)).sum(axis=1) != 0)


def limit_osd_batch(code, seed, dtype, B=8):
    """8 listed frames for the accepted code of the OSD limit pair."""
    rng = np.random.RandomState(seed)
    sent = _words(code, rng, 4 * B)
    prior = _awgn_llr(sent, rng, 3.0).astype(dtype)
    post = (prior * rng.uniform(0.5, 2.0, size=code.n).astype(dtype)[None, :]).astype(dtype)
    keep = osd_listed(code, post)[:B]
    return np.ascontiguousarray(post[keep]), np.ascontiguousarray(prior[keep])


# ---- batches across the 2^17-frame chunk (12_3_4_ldpc) --------------------------------------------------------------------------------

CHUNK = 1 << 17
CROSS_B = CHUNK + 37
CROSS_SPLIT = 70000
CROSS_WINDOW = slice(CHUNK - 8, CHUNK + 37)  # the frames held to the statement: the end of the first chunk and the whole second


def cross_words(code, seed, B=CROSS_B):
    cb = code.cb.astype(np.uint8)
    return cb[np.random.RandomState(seed).randint(len(cb), size=B)]


def cross_bec(code, seed, B=CROSS_B):
    """-> (sent, y) at erasure rate 0.5"""
    sent = cross_words(code, seed, B)
    return sent, _erase(sent, np.random.RandomState(seed + 1), 0.5)


def cross_llr(code, seed, dtype, snr_db=4.0, B=CROSS_B):
    """-> (post, prior): BI-AWGN LLRs at ``snr_db`` and the same scaled per variable"""
    sent = cross_words(code, seed, B)
    rng = np.random.RandomState(seed + 2)
    prior = _awgn_llr(sent, rng, snr_db).astype(dtype)
    post = (prior * rng.uniform(0.5, 2.0, size=code.n).astype(dtype)[None, :]).astype(dtype)
    return np.ascontiguousarray(post), np.ascontiguousarray(prior)


def cross_bsc(code, seed, dtype, p=0.15, B=CROSS_B):
    """-> (y0 [B, n] in {0, 1}, priors = (1 - 2 y0) log((1 - p) / p))"""
    sent = cross_words(code, seed, B)
    y0 = (sent ^ (np.random.RandomState(seed + 3).random_sample(sent.shape) < p)).astype(np.uint8)
    return np.ascontiguousarray(y0), np.ascontiguousarray(((1.0 - 2.0 * y0) * np.log((1 - p) / p)).astype(dtype))

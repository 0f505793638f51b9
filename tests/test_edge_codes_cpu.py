"""The synthetic edge codes of edge_codes.py: the builder's promises, the create rules on each side of their limits, the numpy statements
(test_bec_ml_cpu.ml_statement, osd_oracle.osd_frame) against brute force on them, and what every batch of the device tests holds.  No
GPU needed; test_gpu_elimination_edges.py and test_gpu_chunk_crossing.py hold the device to the statements on exactly these batches."""
import itertools

import numpy as np
import pytest

import edge_codes as EC
import osd_oracle as OSD
from test_bec_ml_cpu import ml_statement, peel

MAX_DEGREE = 64  # what the streaming decoders take (a BecMlHandle peels with one)
IDS = ["%dx%d" % s[:2] for s in EC.SHAPES]


def _dense(code):
    return code.parity_mtx.astype(np.int64)


def _gf2_rank(A):
    """Plain row reduction of a dense 0/1 matrix, one row at a time."""
    A = [int("".join(str(b) for b in row), 2) for row in np.asarray(A).tolist()]
    rank = 0
    while A:
        p = A.pop()
        if p:
            rank += 1
            low = p & -p
            A = [a ^ p if a & low else a for a in A]
    return rank


@pytest.mark.parametrize("m,n,redundant", EC.SHAPES, ids=IDS)
def test_builder_keeps_its_promises(m, n, redundant):
    from ldpc_decoders_amd.encoder import gf2_systematic

    code = EC.shape_code(m, n, redundant)
    H, m0 = _dense(code), m - redundant
    assert (code.m, code.n, code.base_rows) == (m, n, m0)
    want = np.full(n, 3)
    want[code.isolated], want[code.degree_one] = 0, 1
    assert len(code.isolated) == 1 and len(code.degree_one) == 2
    assert (H[:m0].sum(axis=0) == want).all()
    assert (H[:m0].sum(axis=1) >= 2).all() and (H.sum(axis=1) >= 1).all()
    assert (H[:, code.isolated] == 0).all()  # a sum of rows keeps a zero column zero
    assert (H[m0] == H[0]).all() and code.combos[0] == (0,) and len(code.combos) == redundant
    for i, pick in enumerate(code.combos):
        assert 1 <= len(pick) <= 3 and len(set(pick)) == len(pick) and max(pick) < m0
        assert (H[m0 + i] == H[list(pick)].sum(axis=0) % 2).all()
    rank = gf2_systematic(code)[0]
    assert rank == code.encoder().rank == _gf2_rank(H) == _gf2_rank(H[:m0]) <= m0  # the redundant rows add nothing
    assert H.sum(axis=0).max() <= MAX_DEGREE and H.sum(axis=1).max() <= MAX_DEGREE
    again = EC.shape_code(m, n, redundant)
    assert (again.edge_chk == code.edge_chk).all() and (again.edge_var == code.edge_var).all()


def test_create_rules_on_each_side_of_their_limits():
    from ldpc_decoders_amd import bec_ml, bpa

    n, ok, bad = EC.LIMIT_BEC
    assert bec_ml.lds_bytes(ok, n) == 151308 <= bec_ml.LDS_BYTES < bec_ml.lds_bytes(bad, n) == 167948
    bec_ml.check_size(EC.limit_code(ok, n))
    with pytest.raises(ValueError, match="160 KiB"):
        bec_ml.check_size(EC.limit_code(bad, n))
    n, ok, bad = EC.LIMIT_OSD
    assert bpa.osd_lds_bytes(ok, n) == 152512 <= bpa.OSD_LDS_BYTES < bpa.osd_lds_bytes(bad, n) == 164800
    bpa.check_osd_size(EC.limit_code(ok, n))
    with pytest.raises(ValueError, match="160 KiB"):
        bpa.check_osd_size(EC.limit_code(bad, n))
    for m, n, _ in EC.SHAPES:
        assert bec_ml.lds_bytes(m, n) <= bec_ml.LDS_BYTES and bpa.osd_lds_bytes(m, n) <= bpa.OSD_LDS_BYTES
    n, fits, over, _ = EC.OVERFLOW
    assert bec_ml.lds_bytes(fits, n) == 4 * (24 + 27 + 9 * 896) == 32460 <= EC.SMALL_SLAB < bec_ml.lds_bytes(over, n) == 34764
    for m in (fits, over):
        code = EC.overflow_code(m)
        assert code.row_degrees().min() >= 1  # every check touches the all-erased frame: rows = m
        assert max(code.col_degrees().max(), code.row_degrees().max()) <= MAX_DEGREE
        assert EC.lds_bytes_of(code, np.full(n, 2)) == bec_ml.lds_bytes(m, n)


def test_refused_codes_raise_value_error_without_loading_the_library(monkeypatch):
    from ldpc_decoders_amd import _lib, bec_ml, bpa

    def boom():
        raise AssertionError("the library must not be loaded for a code above the limit")

    monkeypatch.setattr(_lib, "load", boom)
    with pytest.raises(ValueError, match="167948"):
        bec_ml.BecEliminationML(0.4, EC.limit_code(EC.LIMIT_BEC[2], EC.LIMIT_BEC[0]))
    with pytest.raises(ValueError, match="164800"):
        bpa.OSD(EC.limit_code(EC.LIMIT_OSD[2], EC.LIMIT_OSD[0]), max_iter=5)


# ---- the statements against brute force ----------------------------------------------------------------------------------------------

def _fillings(code, x):
    """Every filling of the residual set R of a peeled word x that satisfies the checks that touch R (the residual system, by trying all
    2^|R| fillings: no elimination)."""
    H = _dense(code)
    R = np.flatnonzero(x == 2)
    rows = np.flatnonzero(H[:, R].any(axis=1))
    fill = np.array(list(itertools.product((0, 1), repeat=len(R))), dtype=np.int64).reshape(-1, len(R))
    words = np.repeat(np.where(x == 2, 0, x)[None, :], len(fill), axis=0)
    words[:, R] = fill
    return words[((words @ H[rows].T) % 2 == 0).all(axis=1)]


@pytest.mark.parametrize("m,n,redundant", EC.SHAPES, ids=IDS)
def test_ml_statement_against_every_filling_of_the_residual_set(m, n, redundant):
    """On the frames of the device batch whose residual set has at most 12 bits: the statement returns one of the fillings that satisfy the
    residual system, 2^nullity is their number, and it returns -1 exactly when there is none (one known bit next to R flipped; some flips
    leave a solvable system, those count too).  From n = 96 on the stopping sets of these codes are larger than 12 bits and only the frame
    with the isolated variable qualifies, so the -1 side is required of the shapes below that."""
    code = EC.shape_code(m, n, redundant)
    sent, y = EC.bec_batch(code, EC.SEED + 1)
    P = EC.peel_batch(code, y)
    _, P_bad, flipped = EC.inconsistent_batch(code, y, P)
    H = _dense(code)
    small = [f for f in range(len(y)) if 0 < (P[f] == 2).sum() <= 12]
    assert len(small) >= 8
    rng = np.random.RandomState(3)
    seen = {True: 0, False: 0}
    for f in small[:40]:
        sols = _fillings(code, P[f])
        w, d = ml_statement(code, P[f], rng.randint(0, 2, size=n))
        assert d >= 0 and 2 ** d == len(sols) and (sols == w[None, :]).all(axis=1).any()
        assert code.syndrome(w).sum() == 0 and ((w == y[f]) | (y[f] == 2)).all()
        cands = [P_bad[f]] if f in flipped else []
        R = P[f] == 2
        for v in np.flatnonzero((P[f] != 2) & (H[H[:, R].any(axis=1)].sum(axis=0) > 0))[:10]:
            x = P[f].copy()
            x[v] ^= 1
            cands.append(x)
        for x in cands:
            sols = _fillings(code, x)
            w, d = ml_statement(code, x, rng.randint(0, 2, size=n))
            assert (d == -1) == (len(sols) == 0) and (d < 0 or 2 ** d == len(sols))
            seen[d == -1] += 1
    print("%d x %d: %d frames by brute force, %d flips without a solution, %d with" % (m, n, len(small[:40]), seen[True], seen[False]))
    assert seen[True] >= 4 or n >= 96


def test_ml_statement_against_the_code_book():
    """The 70 x 40 code (2^10 codewords): the statement returns a codeword that agrees with the unerased symbols, 2^nullity is the number of
    those, and a frame with a corrupted bit has none and gets -1."""
    m, n, redundant = EC.SHAPES[-1]
    code = EC.shape_code(m, n, redundant)
    cb = _code_book(code)
    sent, y = EC.bec_batch(code, EC.SEED + 1)
    P = EC.peel_batch(code, y)
    y_bad, P_bad, flipped = EC.inconsistent_batch(code, y, P)
    rng = np.random.RandomState(4)
    for f in range(len(y)):
        agree = cb[((cb == y[f][None, :]) | (y[f][None, :] == 2)).all(axis=1)]
        w, d = ml_statement(code, P[f], rng.randint(0, 2, size=n))
        assert 2 ** d == len(agree) and (agree == w[None, :]).all(axis=1).any()
    for f in flipped:
        assert not ((cb == y_bad[f][None, :]) | (y_bad[f][None, :] == 2)).all(axis=1).any()
        assert ml_statement(code, P_bad[f], rng.randint(0, 2, size=n)) == (None, -1)


def _code_book(code):
    enc = code.encoder()
    assert enc.k <= 12
    u = np.array(list(itertools.product((0, 1), repeat=enc.k)), dtype=np.int64)
    cb = enc.encode(u).astype(np.int64)
    assert len(np.unique(cb, axis=0)) == 2 ** enc.k and code.syndrome(cb).sum() == 0
    return cb


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_osd_statement_against_the_code_book(dtype):
    """The 70 x 40 code has 2^10 codewords (the only shape of the table with at most 2^12).  Order 0: the one codeword that agrees with h
    on the free positions.  Order 1 with depth >= |F|: the cheapest of the |F| + 1 codewords that agree with h on F or differ from it in
    exactly one free position, the cost summed over the positions in sorted order."""
    m, n, redundant = EC.SHAPES[-1]
    code = EC.shape_code(m, n, redundant)
    cb, H = _code_book(code), _dense(code).astype(np.uint8)
    post, prior = EC.osd_batch(code, EC.SEED + 2, dtype)
    listed = EC.osd_listed(code, post)
    for f in listed[:60]:
        pi, _, rowof = OSD.eliminate(H, post[f])
        F = pi[rowof < 0]  # the free variables, in position order
        assert len(F) == n - code.encoder().rank
        h, g = OSD.hard(post[f]).astype(np.int64), OSD.hard(prior[f]).astype(np.int64)
        wgt = np.abs(np.where(np.isnan(prior[f]), 0, prior[f])).astype(np.float64)

        def cost(x):
            c = 0.0
            for v in pi:
                if x[v] != g[v]:
                    c = c + wgt[v]
            return c

        cands = []
        for t in range(len(F) + 1):
            want = h[F].copy()
            if t:
                want[t - 1] ^= 1
            hit = cb[(cb[:, F] == want[None, :]).all(axis=1)]
            assert len(hit) == 1  # F is an information set
            cands.append(hit[0])
        w0, t0, c0 = OSD.osd_frame(H, post[f], prior[f], 0, 0)
        assert t0 == 0 and (w0 == cands[0]).all() and c0 == cost(cands[0])
        costs = [cost(x) for x in cands]
        best = int(np.argmin(costs))
        for depth in (len(F), len(F) + 1, 10 ** 6):
            w1, t1, c1 = OSD.osd_frame(H, post[f], prior[f], 1, depth)
            assert t1 == best and c1 == costs[best] and (w1 == cands[best]).all()
        w2, t2, c2 = OSD.osd_frame(H, post[f], prior[f], 1, 3)
        assert t2 == int(np.argmin(costs[:4])) and c2 == costs[t2]


# ---- what the device batches hold -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,redundant", EC.SHAPES, ids=IDS)
def test_bec_batches_hold_what_the_device_tests_need(m, n, redundant):
    code = EC.shape_code(m, n, redundant)
    H = _dense(code)
    sent, y = EC.bec_batch(code, EC.SEED + 1)
    assert y.shape == (192, n) and code.syndrome(sent).sum() == 0
    P = EC.peel_batch(code, y)
    for f in range(0, 192, 19):
        assert (peel(code, y[f]) == P[f]).all()
    listed = (P == 2).any(axis=1)
    assert listed.sum() >= 8 and (~listed).sum() >= 8
    a, z, i, o = (EC.BEC_PLANTED[k] for k in ("all", "none", "isolated", "degree_one"))
    assert (y[a] == 2).all() and (P[a] == 2).all()  # nothing to peel from: nc = n, rows = m
    assert (y[z] == sent[z]).all()
    assert (np.flatnonzero(y[i] == 2) == code.isolated).all() and (np.flatnonzero(P[i] == 2) == code.isolated).all()
    assert not H[:, code.isolated].any()  # a listed frame whose system has no row
    assert ml_statement(code, P[i], np.ones(n, dtype=np.int64))[1] == 1
    assert (np.flatnonzero(y[o] == 2) == code.degree_one[:1]).all() and (P[o] == sent[o]).all()
    for part in (slice(4, 64), slice(64, 128), slice(128, 192)):
        assert listed[part].any()
    y_bad, P_bad, flipped = EC.inconsistent_batch(code, y, P)
    assert len(flipped) == 16 and listed[flipped].all()
    same = np.setdiff1d(np.arange(192), flipped)
    assert (y_bad[same] == y[same]).all() and ((y_bad != y).sum(axis=1)[flipped] == 1).all()
    assert (EC.peel_batch(code, y_bad) == P_bad).all()
    for f in flipped:
        assert (peel(code, y_bad[f]) == P_bad[f]).all()
        assert ml_statement(code, P_bad[f], np.zeros(n, dtype=np.int64))[1] == -1
    assert (listed[same] & np.array([ml_statement(code, P[f], np.zeros(n, dtype=np.int64))[1] >= 0 for f in same])).sum() >= 8


def test_overflow_batch_has_frames_on_both_sides_of_the_first_pass():
    n, fits, over, _ = EC.OVERFLOW
    code = EC.overflow_code(over)
    sent, y = EC.overflow_batch(code, EC.SEED + 3)
    assert y.shape == (64, n)
    P = EC.peel_batch(code, y)
    for f in range(0, 64, 7):
        assert (peel(code, y[f]) == P[f]).all()
    listed = (P == 2).any(axis=1)
    need = np.array([EC.lds_bytes_of(code, x) for x in P])
    assert (listed & (need > EC.SMALL_SLAB)).sum() >= 8 and (listed & (need <= EC.SMALL_SLAB)).sum() >= 8 and (~listed).sum() >= 8
    assert need.max() == 34764 and (need <= 160 * 1024).all()
    assert ((P == 2).sum(axis=1) == n - 1).any()  # one erasure short of the all-erased frame: fits


def test_limit_batches():
    n, ok, _ = EC.LIMIT_BEC
    code = EC.limit_code(ok, n)
    sent, y = EC.limit_bec_batch(code, EC.SEED + 4)
    assert y.shape == (8, n) and (y[0] == 2).all() and code.syndrome(sent).sum() == 0
    P = EC.peel_batch(code, y)
    assert (P == 2).any(axis=1).sum() >= 4
    assert EC.lds_bytes_of(code, P[0]) == 151308
    n, ok, _ = EC.LIMIT_OSD
    code = EC.limit_code(ok, n)
    for dtype in (np.float32, np.float64):
        post, prior = EC.limit_osd_batch(code, EC.SEED + 5, dtype)
        assert post.shape == (8, n) and post.dtype == dtype and len(EC.osd_listed(code, post)) == 8


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m,n,redundant", EC.SHAPES, ids=IDS)
def test_osd_batches_hold_what_the_device_tests_need(m, n, redundant, dtype):
    code = EC.shape_code(m, n, redundant)
    post, prior = EC.osd_batch(code, EC.SEED + 2, dtype)
    assert post.shape == prior.shape == (192, n) and post.dtype == prior.dtype == dtype
    listed = EC.osd_listed(code, post)
    assert set(EC.OSD_PLANTED.values()) <= set(listed.tolist())
    real = listed[listed >= EC.OSD_FIRST_NOISE_ROW]
    assert 0.3 * 180 <= len(real) <= 0.7 * 180  # about half the hard decisions are codewords
    z, a, b, o = (EC.OSD_PLANTED[k] for k in ("zero", "tie_a", "tie_b", "odd"))
    assert (post[z] == 0).sum() == n - 1 and (post[z] < 0).sum() == 1
    for f in (a, b):
        assert len(np.unique(np.abs(post[f]))) == 1 and (np.abs(prior[f]) == np.abs(post[f])).all()
    assert ((post[a] < 0) == (prior[a] < 0)).all() and ((post[b] < 0) != (prior[b] < 0)).sum() == 3
    for t in (post, prior):
        assert np.isnan(t[o]).sum() == 1 and np.isposinf(t[o]).sum() >= 1
    H, nf = _dense(code).astype(np.uint8), n - code.encoder().rank
    winners = EC.osd_winners(code)
    assert (4 + len(winners) <= EC.OSD_FIRST_NOISE_ROW and {t for _, t in winners} == {t for t in (2, 63, 64, 65, 127, 128, nf) if 2 <= t <= nf})
    for f, t in winners:
        assert f in listed and OSD.osd_frame(H, post[f], prior[f], 1, t)[1:] == (t, 0.0) and OSD.osd_frame(H, post[f], prior[f], 1, 10 ** 6)[1] == t
        assert OSD.osd_frame(H, post[f], prior[f], 1, t - 1)[2] > 0.0 and OSD.osd_frame(H, post[f], prior[f], 0, 0)[2] > 0.0
    rest = np.arange(EC.OSD_FIRST_NOISE_ROW, 192)
    assert np.isfinite(post[rest]).all() and np.isfinite(prior[rest]).all()
    assert ((post[rest] < 0) == (prior[rest] < 0)).all()
    differ = sum((OSD.sort_order(post[f]) != OSD.sort_order(prior[f])).any() for f in real[:20])
    assert differ >= 10  # post and prior order the variables differently


def test_chunk_crossing_batches():
    from ldpc_decoders_amd import codes

    code = codes.get_code("12_3_4_ldpc")
    assert EC.CROSS_B == (1 << 17) + 37 and 0 < EC.CROSS_SPLIT < 1 << 17 and EC.CROSS_B - EC.CROSS_SPLIT < 1 << 17
    tail = np.arange(EC.CHUNK, EC.CROSS_B)
    sent, y = EC.cross_bec(code, EC.SEED + 6)
    P = EC.peel_batch(code, y)
    listed = (P == 2).any(axis=1)
    assert y.shape == (EC.CROSS_B, 12) and listed[tail].sum() >= 8 and (~listed)[tail].sum() >= 8
    for f in (0, EC.CHUNK - 1, EC.CHUNK, EC.CROSS_B - 1):
        assert (peel(code, y[f]) == P[f]).all()
    for dtype in (np.float32, np.float64):
        post, prior = EC.cross_llr(code, EC.SEED + 7, dtype)
        lst = np.zeros(EC.CROSS_B, dtype=bool)
        lst[EC.osd_listed(code, post)] = True
        assert post.dtype == dtype and lst[tail].sum() >= 8 and (~lst)[tail].sum() >= 8
        y0, pri = EC.cross_bsc(code, EC.SEED + 8, dtype)
        word = code.syndrome(y0.astype(np.int64)).sum(axis=1) == 0
        assert pri.dtype == dtype and ((pri < 0) == (y0 == 1)).all() and word[tail].sum() >= 4 and (~word)[tail].sum() >= 8

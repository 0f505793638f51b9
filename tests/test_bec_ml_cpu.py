"""ML decoding over the BEC by GF(2) elimination (bec_ml.py, csrc/ldpc_bec_ml.hip): the numpy statement of the contract, checked by
brute force against the code books of the toy codes, and the size limit.  No GPU needed; test_gpu_bec_ml.py holds the device to this
statement bit for bit."""
import numpy as np
import pytest

FREE_BLOCK0 = 0xC0000000


def peel(code, y):
    """The erasure decoder's stopping-set exit: a check with one erased neighbour resolves it, until none is left.  y [n] in {0,1,2}
    -> word with 2 on the residual set (the largest stopping set inside the erasure pattern, whatever the schedule)."""
    x = np.array(y, dtype=np.int64)
    H = code.parity_mtx.astype(bool)
    while True:
        er = x == 2
        cnt = (H & er[None, :]).sum(axis=1)
        hit = np.flatnonzero(cnt == 1)
        if len(hit) == 0:
            return x
        for c in hit:
            nb = np.flatnonzero(H[c])
            e = nb[x[nb] == 2]
            if len(e) == 1:
                x[e[0]] = x[nb[x[nb] != 2]].sum() % 2


def free_bits(seed, stream, frame, count):
    """Bits 0 .. count-1 of a frame's tie-break stream: bit t of word w of Philox block 0xC0000000 + j is free bit 128 j + 32 w + t."""
    import bp_oracle as O

    nblk = (count + 127) // 128
    if nblk == 0:
        return np.zeros(0, dtype=np.uint8)
    ctr = np.zeros((nblk, 4), dtype=np.uint32)
    ctr[:, 0] = (FREE_BLOCK0 + np.arange(nblk)).astype(np.uint32)
    ctr[:, 1] = np.uint32(stream & 0xFFFFFFFF)
    ctr[:, 2] = np.uint32(frame & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32((frame >> 32) & 0xFFFFFFFF)
    key = np.zeros((nblk, 2), dtype=np.uint32)
    key[:, 0] = np.uint32(seed & 0xFFFFFFFF)
    key[:, 1] = np.uint32((seed >> 32) & 0xFFFFFFFF)
    words = O.philox4x32(ctr, key).reshape(-1)
    return ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:count].astype(np.uint8)


def residual_system(code, x):
    """Steps 2 of the contract: columns R (ascending), rows = checks touching R (H's order), right-hand side = XOR of the known bits.
    -> (R, [A | s] as a Code of len(rows) x (|R| + 1))."""
    from ldpc_decoders_amd.codes import Code

    H = code.parity_mtx.astype(np.int64)
    R = np.flatnonzero(x == 2)
    rows = np.flatnonzero(H[:, R].any(axis=1))
    known = np.where(x == 2, 0, x)
    aug = np.concatenate([H[np.ix_(rows, R)], ((H[rows] @ known) % 2)[:, None]], axis=1)
    chk, var = np.nonzero(aug)
    return R, Code.from_edges(len(rows), len(R) + 1, chk.astype(np.int32), var.astype(np.int32))


def ml_statement(code, x, free):
    """Steps 2-4 on a peeled word x (2 = residual): reduced row echelon form of [A | s] (encoder.gf2_systematic: columns ascending,
    pivot = first unused row with a 1); the non-pivot columns of R, ascending, take ``free`` (a bit array, or a callable count -> bits);
    the pivot columns follow.  -> (word in {0,1}, nullity d; -1 if inconsistent, the word is then None)."""
    from ldpc_decoders_amd.encoder import gf2_systematic

    x = np.asarray(x, dtype=np.int64)
    if not (x == 2).any():
        return x.astype(np.uint8), 0
    R, sub = residual_system(code, x)
    nc = len(R)
    rank, par, info, P = gf2_systematic(sub)
    if nc in par:
        return None, -1
    assert info[-1] == nc
    d = nc - rank
    u = np.concatenate([np.asarray(free(d) if callable(free) else free[:d], dtype=np.int64), [1]])
    xr = np.zeros(nc, dtype=np.int64)
    xr[info[:-1]] = u[:-1]
    xr[par] = (u @ P.astype(np.int64)) % 2
    out = x.copy()
    out[R] = xr
    return out.astype(np.uint8), d


def ml_keyed(code, x, seed, stream, frame):
    """ml_statement with the free bits of (seed, stream, global frame index)."""
    return ml_statement(code, x, lambda d: free_bits(seed, stream, frame, d))


def test_margulis_raises_value_error_without_loading_the_library(monkeypatch):
    from ldpc_decoders_amd import _lib, bec, codes

    def boom():
        raise AssertionError("the library must not be loaded for a code above the limit")

    monkeypatch.setattr(_lib, "load", boom)
    code = codes.get_code("margulis")
    with pytest.raises(ValueError, match="160 KiB"):
        bec.ML(0.4, code, max_iter=0)


def test_size_rule_covers_the_reference_codes():
    from ldpc_decoders_amd import bec_ml, codes

    for name in codes.get_code_names():
        c = codes.get_code(name)
        fits = bec_ml.lds_bytes(c.m, c.n) <= bec_ml.LDS_BYTES
        assert fits == (name != "margulis"), name
    assert bec_ml.lds_bytes(600, 1200) == 4 * (3 * 38 + 3 * 38 + 38 * 640)


@pytest.mark.parametrize("name", ["7_4_hamming", "12_3_4_ldpc", "6_2_3_ldpc", "4_2_test"])
def test_statement_solution_set_is_the_consistent_code_book(name):
    """Every assignment of the free bits gives a codeword that agrees with the unerased symbols, they are distinct, and together they
    are exactly the code-book words that agree: 2^d == the number of ML ties."""
    from ldpc_decoders_amd import codes

    code = codes.get_code(name)
    cb = code.cb.astype(np.int64)
    rng = np.random.RandomState(5)
    for trial in range(300):
        sent = cb[rng.randint(len(cb))]
        eps = rng.choice([0.2, 0.5, 0.8, 1.0])
        y = np.where(rng.random_sample(code.n) < eps, 2, sent)
        x = peel(code, y)
        agree = cb[((cb == y[None, :]) | (y[None, :] == 2)).all(axis=1)]
        # peeling only resolves bits every consistent codeword shares
        assert ((agree == np.where(x == 2, agree, x)[None, :]) | (x[None, :] == 2)).all()
        d = ml_statement(code, x, np.zeros(64, dtype=np.int64))[1]
        assert d >= 0 and 2 ** d == len(agree), (name, trial)
        words = set()
        for v in range(2 ** d):
            w, dd = ml_statement(code, x, (v >> np.arange(max(d, 1))) & 1)
            assert dd == d and code.syndrome(w).sum() == 0
            assert ((w == y) | (y == 2)).all()
            words.add(w.tobytes())
        assert words == {a.astype(np.uint8).tobytes() for a in agree}


def test_statement_keyed_draws_are_independent_of_the_batch():
    """The free bits depend on (seed, stream, global frame) only, and the keyed statement is reproducible."""
    from ldpc_decoders_amd import codes

    code = codes.get_code("12_3_4_ldpc")
    y = np.full(code.n, 2)
    a, d = ml_keyed(code, peel(code, y), 9, 1, 1000)
    b, _ = ml_keyed(code, peel(code, y), 9, 1, 1000)
    assert (a == b).all() and d == code.encoder().k
    assert (free_bits(9, 1, 1000, 300)[:200] == free_bits(9, 1, 1000, 200)).all()

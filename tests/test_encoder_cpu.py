"""Systematic GF(2) encoder on the host (ldpc_decoders_amd/encoder.py): every code's [I | P] rows are codewords, the rank is that of an
independent elimination, and the toy codes' encoders span exactly their code books.  No GPU."""
import os
import time

import numpy as np
import pytest

from ldpc_decoders_amd import codes
from ldpc_decoders_amd.encoder import Encoder

SHIPPED = sorted(os.path.splitext(f)[0] for f in os.listdir(codes.PACKAGE_CODES_DIR))
BUILTIN = ["4_2_test", "6_2_3_ldpc", "7_4_hamming", "12_3_4_ldpc"]


def _gf2_rank(code):
    """Rank of H over GF(2) by a different method: rows as Python integers, each reduced against pivots keyed by their leading bit."""
    rows = [0] * code.m
    for c, v in zip(code.edge_chk.tolist(), code.edge_var.tolist()):
        rows[c] ^= 1 << v
    piv = {}
    for x in rows:
        while x:
            hb = x.bit_length() - 1
            if hb not in piv:
                piv[hb] = x
                break
            x ^= piv[hb]
    return len(piv)


def _generated():
    rng = np.random.RandomState(2024)
    return {"gen_1200_3_6": codes.rand_reg_ldpc(1200, 3, 6, rng),
            "gen_10000_irregular": codes.rand_irregular_ldpc(10000, codes.LAMBDA_RHO_X5_HALF_RATE, 6, rng)}


_GEN = {}


def _code(name):
    if name.startswith("gen_"):
        if not _GEN:
            _GEN.update(_generated())
        return _GEN[name]
    return codes.get_code(name)


def _check_systematic(code, enc):
    k, r = enc.k, enc.rank
    assert k + r == code.n and len(enc.info_positions) == k and len(enc.parity_positions) == r
    assert sorted(np.r_[enc.info_positions, enc.parity_positions].tolist()) == list(range(code.n))
    assert (np.diff(enc.info_positions) > 0).all() and enc.P.shape == (k, r)
    # every row of [I | P], placed at (info_pos, par_pos), is a codeword: columns of G packed over its k rows, XOR-ed per check
    G = np.zeros((max(k, 1), code.n), dtype=np.uint8)
    G[np.arange(k), enc.info_positions] = 1
    G[:k, enc.parity_positions] = enc.P
    cols = np.packbits(G, axis=0).T  # [n, ceil(k/8)]
    starts = np.r_[0, np.cumsum(code.row_degrees())[:-1]]
    S = np.bitwise_xor.reduceat(cols[code.edge_var], starts, axis=0)
    assert not S.any()
    some = np.random.RandomState(1).randint(0, k, 8) if k else np.zeros(0, dtype=int)
    assert (enc.encode(np.eye(k, dtype=np.uint8)[some]) == G[some]).all()


@pytest.mark.parametrize("name", SHIPPED + BUILTIN + ["gen_1200_3_6", "gen_10000_irregular"])
def test_systematic_form_and_rank(name):
    code = _code(name)
    enc = code.encoder()
    assert code.encoder() is enc  # cached on the Code
    _check_systematic(code, enc)
    assert enc.rank == _gf2_rank(code)
    u = np.random.RandomState(5).randint(0, 2, (16, enc.k))
    assert code.syndrome(enc.encode(u)).sum() == 0


def test_rank_deficient_1200_code():
    code = codes.get_code("1200_3_6_ldpc")
    enc = code.encoder()
    assert code.m == 600 and enc.rank == 598 and enc.k == 602
    assert code.get_k() == 600  # n - m, left as it is


def test_n10000_within_ten_seconds():
    code = codes.rand_irregular_ldpc(10000, codes.LAMBDA_RHO_X5_HALF_RATE, 6, np.random.RandomState(9))
    t = time.time()
    enc = Encoder(code)
    assert time.time() - t <= 10.0
    assert enc.k >= code.n - code.m


def test_deterministic():
    a, b = Encoder(codes.get_code("1200_3_6_ldpc")), Encoder(codes.get_code("1200_3_6_ldpc"))
    assert (a.parity_positions == b.parity_positions).all() and (a.P == b.P).all()


@pytest.mark.parametrize("name,k", [("4_2_test", 2), ("6_2_3_ldpc", 3), ("7_4_hamming", 4), ("12_3_4_ldpc", 5)])
def test_builtin_codes_span_their_code_books(name, k):
    code = codes.get_code(name)
    enc = code.encoder()
    assert enc.k == k == code.gen_mtx.shape[0]
    msgs = np.array([[(i >> b) & 1 for b in range(k)] for i in range(1 << k)], dtype=np.uint8)
    words = {tuple(w) for w in enc.encode(msgs).tolist()}
    assert len(words) == 1 << k
    assert words == {tuple(w) for w in code.cb.astype(np.uint8).tolist()}


def test_size_limit():
    m, n = 1 << 14, (1 << 14) + 1  # m * n just above 2^28; the elimination must refuse before allocating anything dense
    code = codes.Code.from_edges(m, n, np.arange(m), np.arange(m))
    with pytest.raises(ValueError, match="2\\^28"):
        code.encoder()


def test_encode_checks_width():
    enc = codes.get_code("7_4_hamming").encoder()
    with pytest.raises(ValueError):
        enc.encode(np.zeros((2, 5), dtype=np.uint8))

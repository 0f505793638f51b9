"""The (k, r) family of tests/encoder_codes.py keeps its promises, so that test_gpu_encoder_edges.py can rest on them: exact k, r and m,
the rank by a second method, the information positions an information set (which makes "sent[info] == u and H . sent = 0" determine the
word without P), P dense where a dropped k-group must show, and a carry case that crosses 2^32.  No GPU."""
import time

import numpy as np
import pytest

import encoder_codes as EC
from ldpc_decoders_amd.codes import Code
from ldpc_decoders_amd.encoder import Encoder
from test_encoder_cpu import _check_systematic, _gf2_rank

ALL = EC.SHAPES + EC.DEGENERATE


def test_building_every_code_is_quick():
    """All nineteen codes and their systematic forms in less than test_n10000_within_ten_seconds allows for one."""
    EC._CODES.clear()
    t = time.time()
    for k, r in ALL:
        EC.shape_code(k, r).encoder()
    assert time.time() - t <= 10.0


def test_tables_cover_the_shapes():
    assert set(EC.EXPECTED) == set(ALL) and len(set(ALL)) == len(ALL) == 19
    assert [s for s in EC.SHAPES if s[0] >= 8191] == EC.WIDE == [(8191, 40), (8192, 40), (8193, 40), (16385, 8)]
    assert all(s in EC.SHAPES for s in EC.CARRY_SHAPES)
    reached = list(zip(*EC.EXPECTED.values()))
    assert set(reached[0]) == {1, 2, 4, 8} and {1, 3} <= set(reached[1])
    assert set(reached[2]) == {0, 1, 2, 64, 65, 129} and {1, 2, 3} <= set(reached[3])
    # the two columns that are plain ceilings (nt and the column groups are literal: the cost rule is not restated here)
    for (k, r), (nt, cg, kg, ch) in EC.EXPECTED.items():
        assert kg == -(-k // 128) and ch == -(-kg // 64)
        assert nt * cg * 32 >= r and (cg == 0) == (r == 0)


@pytest.mark.parametrize("k,r", ALL)
def test_shape_rank_and_information_set(k, r):
    code = EC.shape_code(k, r)
    enc = code.encoder()
    redundant = 0 if (k, r) in EC.DEGENERATE else EC.REDUNDANT
    assert (code.k, code.r) == (k, r) and code.n == k + r and code.m == max(r, 1) + redundant
    assert (enc.k, enc.rank) == (k, r) and enc.P.shape == (k, r)
    assert _gf2_rank(code) == r
    assert sorted(np.r_[enc.info_positions, enc.parity_positions].tolist()) == list(range(code.n))
    if r and k < EC.WIDE_K:  # every row of [I | P] is a codeword (a dense k x n generator: the narrow codes only; no edges, nothing to hold)
        _check_systematic(code, enc)
    # the parity positions' columns alone have rank r: no two words agree on the information positions
    sub = np.isin(code.edge_var, enc.parity_positions)
    assert _gf2_rank(Code.from_edges(code.m, code.n, code.edge_chk[sub], code.edge_var[sub])) == r
    u = np.concatenate([EC.info_words(k, 5, 1), np.zeros((3, k), dtype=np.uint8)])  # random words and three unit vectors
    if k:
        u[[5, 6, 7], [0, k // 2, k - 1]] = 1
    sent = enc.encode(u)
    assert code.syndrome(sent).sum() == 0 and (sent[:, enc.info_positions] == u).all()
    if r and k:
        assert enc.P.any(axis=0).all()  # every parity bit reads some information bit


def test_rebuilding_gives_the_same_code():
    a, b = EC.kr_code(33, 65, 7, 2), EC.kr_code(33, 65, 7, 2)
    assert (a.edge_chk == b.edge_chk).all() and (a.edge_var == b.edge_var).all()
    c = EC.kr_code(33, 65, 8, 2)
    assert c.E != a.E or (c.edge_var != a.edge_var).any()


@pytest.mark.parametrize("k,r", EC.WIDE)
def test_wide_codes_have_every_k_group_in_every_parity_bit(k, r):
    P = EC.shape_code(k, r).encoder().P
    kg = EC.EXPECTED[(k, r)][2]
    pad = np.zeros((kg * 128, r), dtype=np.uint8)
    pad[:k] = P
    assert pad.reshape(kg, 128, r).any(axis=1).all()
    assert P[-1].all()  # the last information bit (alone in its k-group when k = 128 g + 1) enters every parity bit
    assert 0.4 < P.mean() < 0.6


def test_redundant_rows_do_not_size_anything():
    code = EC.kr_code(17, 33, 3, 5)
    assert code.m == 38 and code.encoder().rank == 33 and code.encoder().k == 17


def test_carry_frames_straddle_two_to_the_32():
    f = EC.carry_frames()
    assert len(f) == EC.CARRY_B == 40 and int(f[0]) == (1 << 32) - 20
    assert int(f[0]) < 1 << 32 <= int(f[-1]) and ((f >> np.uint64(32)) == 0).sum() == 20 and ((f >> np.uint64(32)) == 1).sum() == 20
    # split at 13: the first call stays below the carry, the second crosses it
    assert int(f[EC.CARRY_SPLIT - 1]) < 1 << 32 and int(f[EC.CARRY_SPLIT]) < 1 << 32 <= int(f[-1])
    # the statement itself notices the carry: frame 2^32 is not frame 0
    a = EC.philox_info_bits(5, 1, 1 << 32, 1, 256)
    b = EC.philox_info_bits(5, 1, 0, 1, 256)
    assert (a != b).any()


def test_encoder_info_refuses_a_null_handle():
    import ctypes

    from ldpc_decoders_amd import _lib

    lib = _lib.load()
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert lib.ldpc_encoder_info(None, out) < 0 and b"ldpc_encoder_info" in lib.ldpc_last_error()
    assert list(out) == [7, 7, 7, 7]


def test_philox_info_bits_shapes():
    assert EC.philox_info_bits(1, 2, 3, 4, 0).shape == (4, 0)
    bits = EC.philox_info_bits(1, 2, 3, 4, 129)
    assert bits.shape == (4, 129) and set(np.unique(bits)) == {0, 1}
    assert (EC.philox_info_bits(1, 2, 4, 3, 129) == bits[1:]).all()

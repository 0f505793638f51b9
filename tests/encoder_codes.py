"""A deterministic family of (k, r) codes at the piece, tile, k-group and chunk edges of the GF(2) encoder (csrc/ldpc_encode.hip), the launch
shape each must reach, and the Philox statement of the random information bits.

TEST INFRASTRUCTURE ONLY (no tests in here).  Everything is drawn from numpy ``RandomState`` seeds, so that test_encoder_codes_cpu.py can
hold the builder to its promises (exact k and r, an information set, a dense P) before test_gpu_encoder_edges.py compares the device with
statements that rest on them.
"""
import numpy as np

import bp_oracle as O
from ldpc_decoders_amd.codes import Code

SEED = 61300
INFO_BLOCK0 = 0x80000000  # Philox blocks of the information bits (csrc/ldpc_encode.hip)
REDUNDANT = 2
WIDE_K = 8191  # from here on a row's information support is drawn with probability 1/2

# information bit j = 128 g + 32 q + 16 h + b; parity column = 32 tile + lane:
#   k at 15 / 16 / 17 (h), 31 / 32 / 33 (q), 127 / 128 / 129 (g, kgroups 1 -> 2), 8191 / 8192 / 8193 (chunks of k_info 1 -> 2), 16 385 (3)
#   r at 31 / 32 / 33 (nt 1 -> 2), 63 / 64 / 65 (2 -> 4), 127 / 128 / 129 (4 -> 8), 256 / 257 (8 tiles -> 9: nt 4 in 3 column groups)
SHAPES = [(1, 1),
          (15, 31), (16, 32), (17, 33),
          (31, 63), (32, 64), (33, 65),
          (63, 127), (64, 128), (65, 129),
          (127, 256), (128, 257), (129, 96),
          (8191, 40), (8192, 40), (8193, 40),
          (16385, 8)]
DEGENERATE = [(0, 33), (40, 0)]
WIDE = [s for s in SHAPES if s[0] >= WIDE_K]

# (nt, column groups, kgroups, chunks) of ldpc_encoder_info, worked out by hand.  With tiles = ceil(r / 32), encoder_create takes the nt of
# 8, 4, 2, 1 (in this order, the first of equals) that minimises ceil(tiles / nt) * (nt + 2):
#   tiles 1: 10, 6, 4, 3 -> 1       tiles 2: 10, 6, 4, 6 -> 2        tiles 3: 10, 6, 8, 9 -> 4       tiles 4: 10, 6, 8, 12 -> 4
#   tiles 5: 10, 12, 12, 15 -> 8    tiles 8: 10, 12, 16, 24 -> 8     tiles 9: 20, 18, 20, 27 -> 4 in 3 groups (12 tiles, 3 of them padding)
#   tiles 0: 0, 0, 0, 0 -> 8 in 0 groups (r = 0: k_encode is not launched)
# kgroups = ceil(k / 128), chunks = ceil(kgroups / 64).
EXPECTED = {
    (1, 1): (1, 1, 1, 1),
    (15, 31): (1, 1, 1, 1), (16, 32): (1, 1, 1, 1), (17, 33): (2, 1, 1, 1),
    (31, 63): (2, 1, 1, 1), (32, 64): (2, 1, 1, 1), (33, 65): (4, 1, 1, 1),
    (63, 127): (4, 1, 1, 1), (64, 128): (4, 1, 1, 1), (65, 129): (8, 1, 1, 1),
    (127, 256): (8, 1, 1, 1), (128, 257): (4, 3, 1, 1), (129, 96): (4, 1, 2, 1),
    (8191, 40): (2, 1, 64, 1), (8192, 40): (2, 1, 64, 1), (8193, 40): (2, 1, 65, 2),
    (16385, 8): (1, 1, 129, 3),
    (0, 33): (2, 1, 0, 0), (40, 0): (8, 0, 1, 1),
}

# random mode across the carry of the global frame index from the low Philox counter word into the high one
CARRY_FRAME0, CARRY_B, CARRY_SPLIT = (1 << 32) - 20, 40, 13
CARRY_SHAPES = [(8193, 40), (129, 96)]


def carry_frames():
    return np.arange(CARRY_FRAME0, CARRY_FRAME0 + CARRY_B, dtype=np.uint64)


def _columns_xor(rows, cols):
    """{i: rows[i] holds an odd number of ``cols``}"""
    cols = set(int(c) for c in cols)
    return set(i for i, r in enumerate(rows) if len(r & cols) & 1)


def kr_code(k, r, seed, redundant):
    """Code with n = k + r variables, m = r + redundant checks and GF(2) rank exactly r.

    The columns are permuted at random; the last r of the permutation are the "parity" columns, the first k the "information" columns.
    Row i < r holds parity column i (an identity block: rank r whatever else the rows hold), an information support -- 3 to 5 columns, or
    each column with probability 1/2 when k >= WIDE_K -- and, for i > 0, one earlier parity column (the block becomes unit lower
    triangular, so P is not the information part verbatim).  The ``redundant`` last rows are GF(2) sums of two different earlier rows (copies of the row
    when r = 1).

    Wide codes only: the information column that Encoder(code) places LAST is then overwritten with the GF(2) sum of the encoder's pivot
    columns, which makes the last row of P all ones.  With k = 128 g + 1 that row is the whole last k-group, and a k-group that took no
    part in some parity bit could be dropped by a kernel without a trace there.  The sum lies in the span of the pivot columns, all of
    them left of it (asserted), so neither the pivots nor the rank move; the redundant rows are drawn after it.

    r = 0: one check without edges (k = n, rank 0).  -> Code with ``.k`` / ``.r`` as requested."""
    rng = np.random.RandomState(seed)
    n = k + r
    if r == 0:
        assert redundant == 0
        code = Code.from_edges(1, n, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
        code.k, code.r = k, r
        return code
    perm = rng.permutation(n)
    info_cols, par_cols = perm[:k], perm[k:]
    rows = []
    for i in range(r):
        row = {int(par_cols[i])}
        if k >= WIDE_K:
            row |= set(int(c) for c in info_cols[rng.randint(0, 2, k).astype(bool)])
        elif k:
            row |= set(int(c) for c in rng.choice(info_cols, min(k, 3 + int(rng.randint(3))), replace=False))
        if i:
            row.add(int(par_cols[rng.randint(i)]))
        rows.append(row)
    if k >= WIDE_K:
        from ldpc_decoders_amd.encoder import gf2_systematic

        rank, par_pos, info_pos, _ = gf2_systematic(_from_rows(n, rows))
        last = int(info_pos[-1])
        assert rank == r and par_pos.max() < last
        on = _columns_xor(rows, par_pos)
        for i, row in enumerate(rows):
            row.discard(last)
            if i in on:
                row.add(last)
    for _ in range(redundant):
        if r == 1:  # nothing to add up: copies of the only row
            rows.append(set(rows[0]))
            continue
        while True:
            a, b = (int(x) for x in rng.choice(len(rows), 2, replace=False))
            if rows[a] ^ rows[b]:
                break
        rows.append(rows[a] ^ rows[b])
    code = _from_rows(n, rows)
    code.k, code.r = k, r
    return code


def _from_rows(n, rows):
    chk = np.repeat(np.arange(len(rows)), [len(x) for x in rows]).astype(np.int32)
    var = np.asarray([v for x in rows for v in sorted(x)], dtype=np.int32)
    return Code.from_edges(len(rows), n, chk, var)


_CODES = {}


def shape_code(k, r):
    """The code of a shape of SHAPES / DEGENERATE, built once per process."""
    if (k, r) not in _CODES:
        _CODES[(k, r)] = kr_code(k, r, SEED + 100 * k + r, 0 if (k, r) in DEGENERATE else REDUNDANT)
    return _CODES[(k, r)]


def info_words(k, B, seed):
    """u [B, k] uint8 in {0, 1} from a RandomState"""
    return np.random.RandomState(seed).randint(0, 2, (B, k)).astype(np.uint8)


def philox_info_bits(seed, stream, frame0, B, k):
    """Information bits of frames [frame0, frame0 + B) from the oracle's Philox4x32-10: bit t of word w of block 0x80000000 + j is bit
    128 j + 32 w + t."""
    nblk = (k + 127) // 128
    f = np.arange(frame0, frame0 + B, dtype=np.uint64)
    ctr = np.zeros((B, nblk, 4), dtype=np.uint32)
    ctr[..., 0] = (INFO_BLOCK0 + np.arange(nblk)).astype(np.uint32)[None, :]
    ctr[..., 1] = np.uint32(stream)
    ctr[..., 2] = (f & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[..., 3] = (f >> np.uint64(32)).astype(np.uint32)[:, None]
    key = np.zeros((B, nblk, 2), dtype=np.uint32)
    key[..., 0], key[..., 1] = seed & 0xFFFFFFFF, seed >> 32
    words = np.ascontiguousarray(O.philox4x32(ctr, key), dtype=np.uint32).reshape(B, nblk * 4)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :k]

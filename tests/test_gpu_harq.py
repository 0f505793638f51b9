"""Incremental-redundancy HARQ on the GPU (csrc/ldpc_harq.hip, _device.HarqHandle): the transmit kernel against sums of
``ldpc_channel_pattern`` draws masked by the numpy tables, the syndrome and the tally against the numpy statement, and the composition
around every served handle class against the pipeline written out here -- all with ``torch.equal`` / ``==``."""
import os

import numpy as np
import pytest

import bp_oracle as O
import harq_oracle as HO
import lqmsa_oracle as LQ
from test_gpu_qc import _code, _layers  # the small quasi-cyclic code of the quasi-cyclic tests, as it is

pytestmark = pytest.mark.gpu
SEED, STREAM = 0x4A52C0DE, 5
SHORT = 32.0
CAP = 50
BIG = "1200_3_6_rand_ldpc_1"
SMALL = "4x8"  # 4 x 8 base, Z = 27: n = 216


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _dt(prec):
    return _torch().float64 if prec == "f64" else _torch().float32


# ============================================================================================== 1. the transmit kernel
def _kind(n, rng):
    """A pattern with a punctured and a shortened variable wherever n leaves room for them beside a buffer variable."""
    kind = rng.choice(3, size=n, p=[0.6, 0.2, 0.2]).astype(np.uint8)
    kind[min(1, n - 1)] = 0
    if n >= 3:
        kind[0], kind[n - 1] = 1, 2
    return kind


def _schedule(Ncb):
    """E < Ncb (where the buffer has two positions), E = Ncb, E = 2 Ncb + 3, and a last single bit; starts at 0 and at Ncb - 1."""
    return (max(Ncb // 2, 1), Ncb, 2 * Ncb + 3, 1), (Ncb - 1, 0, Ncb - 1, 0)


def _subset(rng, size, of):
    return np.sort(rng.choice(of, size=size, replace=False)).astype(np.int64)


def _expected(channel, prec, param, sent_dev, kind_host, kind_dev, cnt_t, first_t, frame0, B_sent, orig, base):
    """base (the gathered rows of the old buffer) + the copies of one transmission: for ascending ordinal r the LLRs that
    ``ldpc_channel_pattern`` draws on stream word STREAM + (r << 16) for the frames [frame0, frame0 + B_sent), rows ``orig`` of them, added
    where the oracle's tables say variable v has a copy at r."""
    torch = _torch()
    from ldpc_decoders_amd import _device

    acc = base.clone()
    top = int((first_t + cnt_t).max())
    for r in range(top):
        on = (first_t <= r) & (r < first_t + cnt_t) & (kind_host == 0)
        if not on.any():
            continue
        ref = _device.channel_pattern(channel, prec, param, sent_dev, 0, kind_dev, SHORT, SEED, STREAM + (r << 16), frame0, B_sent)[0]
        ref = ref if orig is None else ref[orig]
        acc = torch.where(_dev(on)[None, :], acc + ref, acc)
    return acc


@pytest.mark.parametrize("B_out", [1, 65])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65])
def test_transmit(n, B_out):
    """Four transmissions of one schedule, each on top of the one before: the first into a fresh buffer for an ascending subset of the
    frames, the second gathering an ascending subset of those rows (src != orig), the third and fourth row for row; and the same schedule
    with no list at all.  Both channels, both types, with sent words and with the all-zero word, frames beyond 2^33."""
    torch = _torch()
    from ldpc_decoders_amd import _device

    rng = np.random.RandomState(100 * n + B_out)
    kind_host = _kind(n, rng)
    Ncb = int((kind_host == 0).sum())
    bits, starts = _schedule(Ncb)
    cnt, first = HO.tables(kind_host, bits, starts)
    assert cnt.max() >= 3 and (cnt[0] == 0)[kind_host == 0].any() == (Ncb > 1)
    kind = _dev(kind_host)
    cnt_d, first_d = _dev(cnt.astype(np.uint8)), _dev(first.astype(np.uint8))
    B_old, B_sent = 2 * B_out + 1, 3 * B_out + 2
    words = _dev(rng.randint(0, 2, size=(B_sent, n)).astype(np.uint8))
    orig0 = _subset(rng, B_old, B_sent)
    src1 = _subset(rng, B_out, B_old)
    lists = [(None, orig0), (src1, orig0[src1]), (None, orig0[src1]), (None, orig0[src1])]
    assert B_out == 1 or (src1 != orig0[src1]).any()
    for channel, param in (("biawgn", 1.5), ("bsc", 0.11)):
        for frame0 in (0, 2 ** 33 + 5):
            for prec in ("f32", "f64"):
                for sent in (words, None):
                    where = (channel, frame0, prec, sent is not None)
                    fresh = torch.where(_dev(kind_host == 2), torch.full((), SHORT, dtype=_dt(prec), device="cuda"), torch.zeros((), dtype=_dt(prec), device="cuda"))
                    # with the lists
                    soft = None
                    for t, (src, orig) in enumerate(lists):
                        base = fresh[None, :].expand(len(orig), n) if soft is None else soft if src is None else soft[_dev(src)]
                        want = _expected(channel, prec, param, sent, kind_host, kind, cnt[t], first[t], frame0, B_sent, _dev(orig), base)
                        soft = _device.harq_transmit(channel, prec, param, sent, 0, kind, cnt_d[t], first_d[t], SHORT, SEED, STREAM, frame0, None,
                                                     None if src is None else _dev(src), _dev(orig), soft)
                        assert soft.dtype == _dt(prec) and tuple(soft.shape) == (len(orig), n)
                        assert torch.equal(soft, want), where + (t,)
                        assert (soft[:, _dev(kind_host == 2)] == SHORT).all()  # a shortened value never changes
                    # without any list: row i is frame frame0 + i
                    soft = None
                    for t in range(2):
                        base = fresh[None, :].expand(B_out, n) if soft is None else soft
                        want = _expected(channel, prec, param, None if sent is None else sent[:B_out].contiguous(), kind_host, kind, cnt[t], first[t],
                                         frame0, B_out, None, base)
                        soft = _device.harq_transmit(channel, prec, param, sent, 0, kind, cnt_d[t], first_d[t], SHORT, SEED, STREAM, frame0, B_out,
                                                     soft_old=soft)
                        assert torch.equal(soft, want), where + ("identity", t)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [64, 65])
def test_one_whole_transmission_is_the_pattern_channel(n):
    """T = 1, E = Ncb, k = 0: ``ldpc_channel_pattern`` itself, on both channels and in both types."""
    torch = _torch()
    from ldpc_decoders_amd import _device, ratematch

    rng = np.random.RandomState(n)
    kind_host = _kind(n, rng)
    pat = ratematch.Pattern(n, np.flatnonzero(kind_host == 1), np.flatnonzero(kind_host == 2))
    h = ratematch.Harq(pat, [pat.n_tx])
    kind, cnt, first = _dev(pat.kind), _dev(h.cnt[0]), _dev(h.first[0])
    B = 33
    words = _dev(rng.randint(0, 2, size=(B, n)).astype(np.uint8))
    for channel, param in (("biawgn", 0.7), ("bsc", 0.2)):
        for prec in ("f32", "f64"):
            for sent in (words, None):
                want = _device.channel_pattern(channel, prec, param, sent, 0, kind, SHORT, SEED, STREAM, 77, B)[0]
                got = _device.harq_transmit(channel, prec, param, sent, 0, kind, cnt, first, SHORT, SEED, STREAM, 77, B)
                assert torch.equal(got, want), (channel, prec, sent is not None)


def test_unaligned_buffers_take_the_scalar_path():
    """n % 4 == 0 with the old buffer, the words or a table off their natural boundary: the bytes-and-scalars path, the same values."""
    torch = _torch()
    from ldpc_decoders_amd import _device

    n, B = 64, 9
    rng = np.random.RandomState(9)
    kind_host = _kind(n, rng)
    bits, starts = _schedule(int((kind_host == 0).sum()))
    cnt, first = HO.tables(kind_host, bits, starts)
    kind, cnt_d, first_d = _dev(kind_host), _dev(cnt.astype(np.uint8)), _dev(first.astype(np.uint8))
    words = _dev(rng.randint(0, 2, size=(B, n)).astype(np.uint8))

    def off(t, by=1):  # the same values, `by` elements behind an aligned address
        big = torch.empty(t.numel() + by, dtype=t.dtype, device="cuda")
        view = big[by:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % (16 if t.dtype != torch.uint8 else 4) != 0
        return view

    for channel, param in (("biawgn", 1.0), ("bsc", 0.1)):
        for prec in ("f32", "f64"):
            s0 = _device.harq_transmit(channel, prec, param, words, 0, kind, cnt_d[0], first_d[0], SHORT, SEED, STREAM, 5, B)
            want = _device.harq_transmit(channel, prec, param, words, 0, kind, cnt_d[2], first_d[2], SHORT, SEED, STREAM, 5, B, soft_old=s0)
            for what in ("soft", "words", "kind", "cnt"):
                got = _device.harq_transmit(channel, prec, param, off(words) if what == "words" else words, 0, off(kind) if what == "kind" else kind,
                                            off(cnt_d[2]) if what == "cnt" else cnt_d[2], first_d[2], SHORT, SEED, STREAM, 5, B,
                                            soft_old=off(s0) if what == "soft" else s0)
                assert torch.equal(got, want), (channel, prec, what)


def test_transmit_refusals():
    """Every LDPC_E_ARG of the entry point, each with a sentence that names it; nothing is written."""
    torch = _torch()
    from ldpc_decoders_amd import _lib

    B, n = 2, 8
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    sent_kind, short_kind = _dev(np.zeros(n, dtype=np.uint8)), _dev(np.array([0, 0, 2, 0, 0, 0, 0, 0], dtype=np.uint8))
    ones, zeros = _dev(np.ones(n, dtype=np.uint8)), _dev(np.zeros(n, dtype=np.uint8))
    soft = torch.full((B, n), 7.0, dtype=torch.float32, device="cuda")

    def call(channel, codeword=0, kind=sent_kind, short_llr=SHORT, stream_id=STREAM, old=None, param=0.1):
        return lib.ldpc_harq_transmit(channel, 0, param, None, 0, codeword, kind.data_ptr(), ones.data_ptr(), zeros.data_ptr(), short_llr, SEED, stream_id, 0,
                                      None, None, old, 0 if old is None else B, B, n, soft.data_ptr(), st)

    for ch in (_lib.CHANNEL["bec"], _lib.CHANNEL["biawgn"] | _lib.CH_RAW_OBSERVATION, _lib.CHANNEL["biawgn"] | _lib.ch_prior_grid(4),
               _lib.CHANNEL["bsc"] | _lib.ch_prior_grid(0), 7):
        assert call(ch) == -1 and lib.ldpc_last_error().startswith(b"ldpc_harq_transmit: "), ch
    for bad in (0.0, -32.0, float("inf"), float("nan")):
        assert call(_lib.CHANNEL["biawgn"], short_llr=bad) == -1 and b"ldpc_harq_transmit: short_llr" in lib.ldpc_last_error()
    for bad in (65536, 2 ** 32, 2 ** 40 + 3):
        assert call(_lib.CHANNEL["biawgn"], stream_id=bad) == -1 and b"ldpc_harq_transmit: stream_id" in lib.ldpc_last_error()
    assert call(_lib.CHANNEL["bsc"], param=1.5) == -1 and b"ldpc_harq_transmit: channel probability" in lib.ldpc_last_error()
    assert call(_lib.CHANNEL["biawgn"], old=soft.data_ptr()) == -1 and b"ping-pong" in lib.ldpc_last_error()
    for ch in ("biawgn", "bsc"):
        assert call(_lib.CHANNEL[ch], codeword=1, kind=short_kind) == -1 and b"ldpc_harq_transmit: the all-one word" in lib.ldpc_last_error()
        assert call(_lib.CHANNEL[ch], codeword=2) == -1
    torch.cuda.synchronize()
    assert (soft == 7.0).all()
    assert call(_lib.CHANNEL["biawgn"], stream_id=65535) == 0 and call(_lib.CHANNEL["bsc"], codeword=1) == 0
    torch.cuda.synchronize()
    assert not (soft == 7.0).any()


# ============================================================================================== 2. the syndrome
_CODES = {}


def _named(name):
    """-> (oracle edge list, codes.Code) of a packaged code"""
    if name not in _CODES:
        from ldpc_decoders_amd import codes

        c = codes.get_code(name)
        _CODES[name] = (O.Edges(c.m, c.n, c.edge_chk, c.edge_var), c)
    return _CODES[name]


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("name", ["7_4_hamming", "1200_rho_x5_rand_ldpc_5"])
def test_syndrome(name, B):
    """Codewords pass; a single flip fails exactly when the flipped variable is on a check (the irregular code has variables of degree 0,
    whose flips no check sees, and of degree 1); random words against the oracle."""
    torch = _torch()
    from ldpc_decoders_amd import _device

    g, c = _named(name)
    rng = np.random.RandomState(B)
    enc = c.encoder()
    words = enc.encode(rng.randint(0, 2, size=(B, enc.k)).astype(np.uint8)).astype(np.uint8)
    assert not c.syndrome(words).any() and (B == 1 or words.any())
    deg = np.bincount(np.asarray(c.edge_var), minlength=c.n)
    if name != "7_4_hamming":
        assert (deg == 0).any() and (deg == 1).any() and len(np.unique(np.bincount(np.asarray(c.edge_chk), minlength=c.m))) > 1
    flips = words.copy()
    where = rng.randint(0, c.n, size=B)
    if name != "7_4_hamming":
        where[0] = np.flatnonzero(deg == 1)[0] if B == 1 else np.flatnonzero(deg == 0)[0]
        if B > 2:
            where[1], where[2] = np.flatnonzero(deg == 1)[0], c.n - 1
    flips[np.arange(B), where] ^= 1
    noise = rng.randint(0, 2, size=(B, c.n)).astype(np.uint8)
    h = _device.code_handle(c)
    for xhat, want in ((words, np.zeros(B, dtype=np.uint8)), (flips, (deg[where] > 0).astype(np.uint8)), (noise, None)):
        oracle = HO.syndrome_fail(c.m, c.edge_chk, c.edge_var, xhat)
        assert want is None or np.array_equal(oracle, want)
        got = _device.harq_syndrome(h, _dev(xhat))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (B,)
        assert torch.equal(got, _dev(oracle))
        assert np.array_equal(oracle == 0, O.syndrome_ok(g, xhat.astype(np.int64)))


# ============================================================================================== 3. the tally
@pytest.mark.parametrize("B", [1, 5, 300])
def test_tally(B):
    """The counters of the numpy statement at the first, a middle and the last transmission, accumulated into; the rows hold every kind:
    failed rows of the last transmission (they leave), failed rows of an earlier one (they do not), acknowledged rows with and without
    errors; errors on shortened bits count nothing."""
    torch = _torch()
    from ldpc_decoders_amd import _device

    n, T, rows = 131, 4, 2 * B + 3
    rng = np.random.RandomState(B)
    kind_host = rng.choice(3, size=n, p=[0.6, 0.2, 0.2]).astype(np.uint8)
    kind = _dev(kind_host)
    sent_host = rng.randint(0, 2, size=(rows, n)).astype(np.uint8)
    orig = _subset(rng, B, rows)
    iters = rng.randint(0, 12, size=B).astype(np.int32)
    for sent, codeword in ((sent_host, 0), (None, 0), (None, 1)):
        base = np.full((B, n), codeword, dtype=np.uint8) if sent is None else sent[orig]
        flips = (rng.random_sample((B, n)) < 0.05).astype(np.uint8)
        flips[::2] = 0
        flips[1::4] &= (kind_host == 2)[None, :]  # errors on shortened bits alone: no error counted
        xhat = base ^ flips
        err = (flips & (kind_host < 2)[None, :]).sum(axis=1)
        fail = rng.randint(0, 2, size=B).astype(np.uint8)
        if B >= 5:
            fail[:4] = [0, 0, 1, 1]  # row 3: errors and a failed syndrome
            assert err[3] > 0 or B == 5
        if B == 300:
            assert ((err > 0) & (fail == 0)).any() and ((err == 0) & (fail == 1)).any()  # an acknowledged row with an error; a failed row without
        for t in (0, 2, T - 1):
            for use_iters, bins in ((True, 0), (True, 8), (False, 8)):
                start = np.arange(4 + bins + T + 2, dtype=np.int64) * 1000 + 17
                want = HO.tally(xhat, sent, codeword, kind_host, iters if use_iters else None, fail, orig, bins, t, T, 800)
                cnt = _dev(start.copy())
                _device.harq_tally(_dev(xhat), None if sent is None else _dev(sent), codeword, kind, _dev(iters) if use_iters else None, _dev(fail), _dev(orig),
                                   bins, t, T, 800, cnt)
                assert np.array_equal(cnt.cpu().numpy(), start + want), (sent is not None, codeword, t, use_iters, bins)
                assert want[4 + bins + T + 1] == 800 * B and want[0] == (B if t == T - 1 else (fail == 0).sum())
                assert want[4 + bins + T] == ((err > 0) & (fail == 0)).sum() and want[1] == ((err > 0) & ((fail == 0) | (t == T - 1))).sum()
    # the two rows the rule turns on, by hand: a failed row of the last transmission leaves with its errors; an acknowledged row with an
    # error is an undetected error
    kind2 = _dev(np.zeros(4, dtype=np.uint8))
    x = _dev(np.array([[1, 0, 0, 0], [0, 1, 1, 0]], dtype=np.uint8))
    cnt = torch.zeros(4 + 2 + 2, dtype=torch.int64, device="cuda")
    _device.harq_tally(x, None, 0, kind2, _dev(np.array([3, 4], dtype=np.int32)), _dev(np.array([1, 0], dtype=np.uint8)), None, 0, 1, 2, 10, cnt)
    assert cnt.cpu().tolist() == [2, 2, 3, 7, 0, 1, 1, 20]
    cnt.zero_()
    _device.harq_tally(x, None, 0, kind2, None, _dev(np.array([1, 0], dtype=np.uint8)), None, 0, 0, 2, 10, cnt)
    assert cnt.cpu().tolist() == [1, 1, 2, 0, 1, 0, 1, 20]


# ============================================================================================== 4. the composition
# 130 frames, CHUNK = 64, T = 3, E = 800 per transmission, rv starts, random codewords of the shortened code, on BI-AWGN.
#
# Every branch of the loop has to be live in such a run: each transmission acknowledges a frame, and a frame is never acknowledged.  With
# the decoders run to their usual cap of 50 sweeps that cannot happen: the third transmission carries three times the energy of the first,
# 4.8 dB, and more where the first leaves buffer bits unsent, while the word-error curve of an n = 1200 code falls from 129 / 130 to
# 1 / 130 within 2 dB (measured: under 27 punctured and 5 shortened bits fp32 MSA first acknowledges at transmission 0 from 4.5 dB and
# last fails transmission 2 at -0.5 dB).  So the composed runs cap the decoder at ONE sweep, where a frame is acknowledged when a single
# sweep leaves no bit wrong -- an event per bit, whose probability moves slowly with the SNR -- and the n = 1200 code shortens its last 373
# variables beside the 27 punctured ones: a buffer of exactly 800, every buffer bit sent once per transmission (from the rv starts
# 0, 400, 600), none left to be filled in by later sweeps.  The 4 x 8, Z = 27 code (n = 216) punctures its first block column and
# shortens 5 bits, a buffer of 184, so each of its transmissions repeats every bit four or five times.  Nothing in the loop depends on
# the cap; the decoders at their usual cap are compared in test_one_whole_transmission_equals_the_pattern_handle.
FRAMES, CHUNK, T_TX, E_TX, BINS = 130, 64, 3, 800, 8
FRAME0 = 2 ** 33 + 1000
CSTREAM = STREAM  # the stream of the runs below that are not in POINT
CCAP = 1  # the sweep cap of the composed runs
CASES = [(BIG, ("f32", "fused")), (BIG, ("f32", "stream")), (BIG, ("f64", "fused")), (BIG, ("f64", "stream")), (BIG, "lmsa"), (BIG, "lqmsa"),
         (SMALL, "qc"), (SMALL, "slq")]
# (SNR in dB per transmitted symbol, stream) of every case, found on one MI355X by a scan in 0.25 dB steps (LMSA: 0.125) over a few
# streams, and observed there: ack = frames acknowledged at transmission 0, 1, 2; never = frames of the 130 never acknowledged.
#   n = 1200, flooding MSA, fp32 and fp64, both backends   4.75 dB, stream 5   ack [3, 121, 5]    never 1
#   n = 1200, LMSA                                         2.75 dB, stream 121 ack [3, 121, 5]    never 1   (streams 0 .. 127 scanned)
#   n = 1200, LQMSA                                        2.75 dB, stream 2   ack [1, 121, 7]    never 1
#   n = 216, QCMSA and SLQMSA (equal counters)            -2.75 dB, stream 2   ack [3, 109, 17]   never 1
POINT = {(BIG, ("f32", "fused")): (4.75, 5), (BIG, ("f32", "stream")): (4.75, 5), (BIG, ("f64", "fused")): (4.75, 5), (BIG, ("f64", "stream")): (4.75, 5),
         (BIG, "lmsa"): (2.75, 121), (BIG, "lqmsa"): (2.75, 2), (SMALL, "qc"): (-2.75, 2), (SMALL, "slq"): (-2.75, 2)}
_HANDLES, _RUNS = {}, {}


def _setup(key):
    return _named(key) if key == BIG else _code(key)[:2]


def _pattern(key):
    from ldpc_decoders_amd import ratematch

    c = _setup(key)[1]
    if key == BIG:
        p = ratematch.Pattern(c.n, punctured=range(27), shortened=[40, 41, 100, 500, 1199])
    else:
        Z = _code(key)[3]
        p = ratematch.Pattern(c.n, punctured=ratematch.block_columns([0], Z), shortened=[Z + 1, Z + 2, 2 * Z + 1, 3 * Z + 2, 4 * Z + 2])
    assert p.unrecoverable(c).size == 0
    return p


def _composed_pattern(key):
    """The pattern of the composed runs: the n = 1200 code shortens its last 373 variables beside the 27 punctured ones, a buffer of
    exactly 800, so that every transmission sends every buffer bit once; the small code keeps ``_pattern``."""
    from ldpc_decoders_amd import ratematch

    if key != BIG:
        return _pattern(key)
    c = _setup(key)[1]
    p = ratematch.Pattern(c.n, punctured=range(27), shortened=range(c.n - 373, c.n))
    assert p.unrecoverable(c).size == 0 and p.n_tx == E_TX
    return p


def _harq(key, bits=None, rv=True):
    from ldpc_decoders_amd import ratematch

    p = _composed_pattern(key)
    bits = (E_TX,) * T_TX if bits is None else bits
    return ratematch.Harq(p, bits, ratematch.rv_starts(p.n_tx, len(bits)) if rv else None)


def _inner(key, which):
    """-> (handle, layers for the integer statement or None)"""
    from ldpc_decoders_amd import _device

    if (key, which) not in _HANDLES:
        c = _setup(key)[1]
        if which == "qc":
            h, lay = _device.QcHandle(c, _code(key)[3]), _layers(key)
        elif which == "lqmsa":
            h = _device.LqmsaHandle(c)
            lay = h.layers()[1].astype(np.int64)
        elif which == "slq":
            h = _device.SlqHandle(c)
            lay = h.layers()[1].astype(np.int64)
        elif which == "lmsa":
            h, lay = _device.DecoderHandle(c, "LMSA", "f32", "auto"), None
        else:
            h, lay = _device.DecoderHandle(c, "MSA", which[0], which[1]), None
        _HANDLES[(key, which)] = (h, lay)
    return _HANDLES[(key, which)]


def _ran_on(inner, which):
    """A flooding decoder's last call ran on the kernels its case names."""
    if isinstance(which, tuple):
        assert inner.last_stats()[0] == which[1], (inner.last_stats(), which)


def _words(c, pattern, frame0, B, stream):
    """The sent words of codeword -1, written out: the encoder of the shortened code, scattered through the index map on the host."""
    short, index = pattern.shortened_code(c)
    w = short.encoder().handle(_torch().cuda.current_device()).encode_random(SEED, stream, frame0, B).cpu().numpy()
    full = np.zeros((B, c.n), dtype=np.uint8)
    full[:, index] = w
    return full


def _written_out(key, which, harq, snr, frame0, B, chunk, keep=None, cap=CAP, stream=CSTREAM):
    """The pipeline of HarqHandle.simulate from its calls: per chunk the words, then transmit -> decode -> syndrome -> the numpy tally ->
    the ascending survivor list made on the host.  ``keep``: a dict that receives the priors, decisions and iteration counts of the first
    chunk's second transmission."""
    torch = _torch()
    from ldpc_decoders_amd import _device

    inner = _inner(key, which)[0]
    g, c = _setup(key)
    kind_host = harq.pattern.kind
    kind, cnt, first = _dev(kind_host), _dev(harq.cnt), _dev(harq.first)
    total = np.zeros(4 + BINS + harq.T + 2, dtype=np.int64)
    for start in range(frame0, frame0 + B, chunk):
        rows = min(chunk, frame0 + B - start)
        sent_host = _words(c, harq.pattern, start, rows, stream)
        assert not c.syndrome(sent_host).any() and not sent_host[:, harq.pattern.shortened].any() and sent_host.any()
        sent = _dev(sent_host)
        src = orig = soft = None
        for t in range(harq.T):
            soft = _device.harq_transmit("biawgn", inner.precision, snr, sent, 0, kind, cnt[t], first[t], SHORT, SEED, stream, start, rows,
                                         None if src is None else _dev(src), None if orig is None else _dev(orig), soft)
            xhat, iters = inner.decode_device(soft, None, cap)[:2]
            _ran_on(inner, which)
            fail = _device.harq_syndrome(inner.code_handle, xhat)
            torch.cuda.synchronize()
            xhat_h, iters_h, fail_h = xhat.cpu().numpy(), iters.cpu().numpy(), fail.cpu().numpy()
            assert np.array_equal(fail_h == 0, O.syndrome_ok(g, xhat_h.astype(np.int64)))
            total += HO.tally(xhat_h, sent_host, 0, kind_host, iters_h, fail_h, orig, BINS, t, harq.T, harq.tx_bits[t])
            if keep is not None and t == 1 and start == frame0:
                keep.update(priors=soft.cpu().numpy(), xhat=xhat_h, iters=iters_h)
            src = np.flatnonzero(fail_h).astype(np.int64)
            if src.size == 0:
                break
            orig = src if orig is None else orig[src]
            rows = src.size
    return total


def _simulate(key, which, harq, snr, frame0, B, chunk, monkeypatch, codeword=-1, cap=CAP, stream=CSTREAM):
    torch = _torch()
    from ldpc_decoders_amd import _device

    monkeypatch.setattr(_device.HarqHandle, "CHUNK", chunk)
    hh = _device.HarqHandle(_inner(key, which)[0], harq)
    assert hh.extra_counters == harq.T + 2
    cnt = torch.zeros(4 + BINS + harq.T + 2, dtype=torch.int64, device="cuda")
    hh.simulate("biawgn", snr, codeword, SEED, stream, frame0, B, cap, cnt, hist_bins=BINS)
    return cnt.cpu().numpy()


def _run(key, which, monkeypatch):
    """The composed run of a case, made once."""
    if (key, which) not in _RUNS:
        snr, stream = POINT[(key, which)]
        _RUNS[(key, which)] = _simulate(key, which, _harq(key), snr, FRAME0, FRAMES, CHUNK, monkeypatch, cap=CCAP, stream=stream)
        print(key, which, "snr", snr, "stream", stream, "counters", _RUNS[(key, which)].tolist())
    return _RUNS[(key, which)]


@pytest.mark.parametrize("key,which", CASES, ids=str)
def test_simulate_equals_the_pipeline_written_out(key, which, monkeypatch):
    """All 4 + hist + T + 2 counters of HarqHandle.simulate equal the pipeline written out; they do not depend on the chunk size or on
    how the frame range is split over calls; the counter identities hold; for the integer families the integer statement decodes the
    combined priors of the second transmission to the same decisions."""
    harq = _harq(key)
    snr, stream = POINT[(key, which)]
    got = _run(key, which, monkeypatch)
    keep = {}
    want = _written_out(key, which, harq, snr, FRAME0, FRAMES, CHUNK, keep, cap=CCAP, stream=stream)
    assert np.array_equal(got, want), (got, want)
    assert got[0] == FRAMES
    HO.check_identities(got, BINS, harq.tx_bits)
    assert np.array_equal(_simulate(key, which, harq, snr, FRAME0, FRAMES, FRAMES, monkeypatch, cap=CCAP, stream=stream), got)
    split = _simulate(key, which, harq, snr, FRAME0, 50, CHUNK, monkeypatch, cap=CCAP, stream=stream) \
        + _simulate(key, which, harq, snr, FRAME0 + 50, FRAMES - 50, CHUNK, monkeypatch, cap=CCAP, stream=stream)
    assert np.array_equal(split, got), (split, got)
    g, lay = _setup(key)[0], _inner(key, which)[1]
    if lay is not None:
        assert keep, "no second transmission in the first chunk"
        rows = min(12, keep["priors"].shape[0])
        x, it, _, _ = LQ.lqmsa_decode(g, None, keep["priors"][:rows], CCAP, layers=lay)
        assert np.array_equal(x, keep["xhat"][:rows]) and np.array_equal(it, keep["iters"][:rows])


@pytest.mark.parametrize("key,which", CASES, ids=str)
def test_every_branch_is_live(key, which, monkeypatch):
    """At the point of the case every transmission acknowledges at least one frame, and at least one frame is never acknowledged (the
    values observed are in the comment at POINT), so no branch of the loop, of the tally or of the survivor gather idles in the run that
    test_simulate_equals_the_pipeline_written_out compares."""
    got = _run(key, which, monkeypatch)
    ack = got[4 + BINS:4 + BINS + T_TX].tolist()
    print(key, which, "point", POINT[(key, which)], "ack", ack, "never", FRAMES - sum(ack))
    assert all(a >= 1 for a in ack) and FRAMES - sum(ack) >= 1, (ack, FRAMES - sum(ack))


@pytest.mark.parametrize("key,which", CASES, ids=str)
def test_one_whole_transmission_equals_the_pattern_handle(key, which, monkeypatch):
    """T = 1, E = Ncb, k = 0 on BI-AWGN: the first four counters (and the histogram) are PatternHandle's."""
    torch = _torch()
    from ldpc_decoders_amd import _device, ratematch

    p = _pattern(key)
    harq = ratematch.Harq(p, [p.n_tx])
    snr = 1.75 if key == BIG else 2.5
    inner = _inner(key, which)[0]
    for codeword in (-1, 0):
        got = _simulate(key, which, harq, snr, FRAME0, FRAMES, CHUNK, monkeypatch, codeword)
        monkeypatch.setattr(_device.PatternHandle, "CHUNK", CHUNK)
        want = torch.zeros(4 + BINS, dtype=torch.int64, device="cuda")
        _device.PatternHandle(inner, p).simulate("biawgn", snr, codeword, SEED, CSTREAM, FRAME0, FRAMES, CAP, want, hist_bins=BINS)
        want = want.cpu().numpy()
        assert np.array_equal(got[:4 + BINS], want), (got, want)
        assert got[0] == FRAMES and 0 < got[1] < FRAMES
        assert got[4 + BINS] + got[1] - got[4 + BINS + 1] == FRAMES and got[4 + BINS + 2] == FRAMES * p.n_tx


def test_all_one_word_and_the_bsc(monkeypatch):
    """codeword 1 (words of ones on the device, no shortened bit) and the BSC run through the same loop: identities and chunk independence."""
    torch = _torch()
    from ldpc_decoders_amd import _device, ratematch

    c = _setup(SMALL)[1]
    p = ratematch.Pattern(c.n, punctured=_pattern(SMALL).punctured)
    harq = ratematch.Harq(p, (150, 150, 150), ratematch.rv_starts(p.n_tx, 3))
    inner = _inner(SMALL, "qc")[0]
    hh = _device.HarqHandle(inner, harq)
    for channel, param, codeword in (("biawgn", 1.0, 1), ("bsc", 0.06, 0), ("bsc", 0.06, -1)):
        rows = []
        for chunk in (CHUNK, 33):
            monkeypatch.setattr(_device.HarqHandle, "CHUNK", chunk)
            cnt = torch.zeros(4 + harq.T + 2, dtype=torch.int64, device="cuda")
            hh.simulate(channel, param, codeword, SEED, CSTREAM, 11, FRAMES, CAP, cnt)
            rows.append(cnt.cpu().numpy())
        assert np.array_equal(rows[0], rows[1]) and rows[0][0] == FRAMES, (channel, rows)
        HO.check_identities(rows[0], 0, harq.tx_bits)


def test_refusals():
    """Each a ValueError with one sentence, before any device call."""
    torch = _torch()
    from ldpc_decoders_amd import _device, _lib, ratematch

    harq = _harq(SMALL)
    for cls in (_device.OsdHandle, _device.HardHandle, _device.AdmmHandle, _device.MlHandle, _device.BecMlHandle):
        with pytest.raises(ValueError):
            _device.HarqHandle(cls.__new__(cls), harq)
    with pytest.raises(ValueError, match="OSD"):
        _device.HarqHandle(_device.OsdHandle.__new__(_device.OsdHandle), harq)
    bec = _device.DecoderHandle.__new__(_device.DecoderHandle)
    bec.alg = "BEC"
    for bad in (bec, object()):
        with pytest.raises(ValueError):
            _device.HarqHandle(bad, harq)
    inner = _inner(SMALL, "qc")[0]
    with pytest.raises(ValueError):
        _device.HarqHandle(inner, ratematch.Harq(ratematch.Pattern(inner.code.n + 1), [5]))
    with pytest.raises(ValueError):
        _device.HarqHandle(inner, harq, short_llr=0.0)
    hh = _device.HarqHandle(inner, harq)
    cnt = torch.zeros(4 + harq.T + 2, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="bec"):
        hh.simulate("bec", 0.1, 0, SEED, CSTREAM, 0, 4, CAP, cnt)
    with pytest.raises(ValueError, match="prior-grid"):
        hh.simulate("biawgn", 2.0, 0, SEED, CSTREAM, 0, 4, CAP, cnt, flags=_lib.flag_prior_grid(4))
    with pytest.raises(ValueError, match="all-one"):
        hh.simulate("biawgn", 2.0, 1, SEED, CSTREAM, 0, 4, CAP, cnt)
    with pytest.raises(ValueError, match="65536"):
        hh.simulate("biawgn", 2.0, 0, SEED, 65536, 0, 4, CAP, cnt)
    assert not cnt.cpu().numpy().any()


def test_cli(tmp_path, monkeypatch):
    """One command-line run under a schedule: the result file carries the id keys and the HARQ fields, and they satisfy the identities."""
    import json

    from ldpc_decoders_amd import codes, main, qc

    code_dir = tmp_path / "codes"
    monkeypatch.setenv(codes.file_codes_dir_string, str(code_dir))
    qc.gen_rand_qc(qc.setup_parser().parse_args("1 4 8 27 --seed 5 --dir".split() + [str(code_dir)]))
    argv = "biawgn 216_qc_4x8_z27_1 QCMSA --params 0.0 --max-iter 20 --batch 2048 --max-frames 2048 --codeword -1".split()
    main.main(argv + ["--puncture-cols", "7", "--shorten", "30:35", "--harq-bits", "150,100,100", "--harq-starts", "rv", "--data_dir", str(tmp_path), "--console"])
    name = "biawgn-216_qc_4x8_z27_1-QCMSA--1-100-20-6-2-0.8125-0.0-27-189:216-30:35-150,100,100-0,81,135.json"
    with open(os.path.join(str(tmp_path), name)) as fp:
        res = json.load(fp)
    assert res["harq_bits"] == "150,100,100" and res["harq_starts"] == "0,81,135" and res["puncture"] == "189:216"
    tot, wec, ack, und, sym = res["tot"]["0.0"], res["wec"]["0.0"], res["ack"]["0.0"], res["undetected"]["0.0"], res["sym"]["0.0"]
    assert tot == 2048 and len(ack) == 3 and wec == und + tot - sum(ack)
    assert sym == 150 * tot + 100 * (tot - ack[0]) + 100 * (tot - ack[0] - ack[1])
    assert res["avg_tx"]["0.0"] == pytest.approx((3 * tot - 2 * ack[0] - ack[1]) / tot)
    from ldpc_decoders_amd import ratematch

    code = codes.get_code("216_qc_4x8_z27_1")
    K = ratematch.Pattern(code.n, shortened=range(30, 35)).shortened_code(code)[0].encoder().k
    assert 216 - 108 - 5 <= K < 216 - 5
    assert res["tput"]["0.0"] == pytest.approx((tot - wec) * K / sym) and 0 < res["tput"]["0.0"] < 1

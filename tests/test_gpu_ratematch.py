"""Punctured and shortened transmission on the GPU (csrc/ldpc_ratematch.hip, _device.PatternHandle): the pattern channel against
``ldpc_channel_sent`` / ``ldpc_channel`` and the numpy statement, the masked tally against the numpy statement, and the composition around
every LLR handle class -- all with ``==``.

The composition runs at the SNR that ``test_gpu_qc._batch`` bisects for the all-sent code.  Under the pattern used here (one punctured block
column, 5 shortened bits) the integer statement on numpy noise at that SNR leaves a codeword in 20 .. 27 of 49 frames of the dense Z = 7
code and in 7 .. 18 of 49 frames of the 4 x 8 code (three noise seeds each), so a batch of 49 frames holds both kinds of frame for any
seed; both are asserted present."""
import json
import os

import numpy as np
import pytest

import bp_oracle as O
import lqmsa_oracle as LQ
import ratematch_oracle as RO
from test_gpu_qc import _batch, _code, _layers  # the codes and the SNR bisection of the quasi-cyclic tests, as they are

pytestmark = pytest.mark.gpu
SEED, STREAM = 0x7A7E3A7C, 3
SHORT = 32.0
CAP = 50
KEYS = [("dense", 7), "4x8"]


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


# ============================================================================================== 1. the channel kernel
def _patterns(n, rng):
    half = rng.permutation(n)[:n // 2]
    mixed = np.zeros(n, dtype=np.uint8)
    mixed[half] = rng.randint(1, 3, size=half.size)
    pats = {"all sent": np.zeros(n, dtype=np.uint8), "all punctured": np.full(n, 1, dtype=np.uint8), "all shortened": np.full(n, 2, dtype=np.uint8),
            "random half": mixed}
    for name, idx in (("variable 0", [0]), ("variable n-1", [n - 1]), ("{3, 4}", [v for v in (3, 4) if v < n])):
        for k in (1, 2):
            kind = np.zeros(n, dtype=np.uint8)
            kind[idx] = k
            pats["%s kind %d" % (name, k)] = kind
    return pats


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65, 1201])
def test_channel_pattern(n, B):
    """kind 0: the draws of ldpc_channel_sent / ldpc_channel, bit for bit; kind 1: +0.0; kind 2: short_llr; the BSC equal to the numpy
    statement.  Byte path (n % 4 != 0) and dword path, one thread per frame (n <= 4), a ragged last block, frames beyond 2^33."""
    torch = _torch()
    from ldpc_decoders_amd import _device, _lib

    rng = np.random.RandomState(1000 * n + B)
    pats = _patterns(n, rng)
    words_host = rng.randint(0, 2, size=(B, n)).astype(np.uint8)
    words = _dev(words_host)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    for channel, param in (("biawgn", 1.5), ("bsc", 0.11)):
        for frame0 in (0, 2 ** 33 + 5):
            philox = RO.philox_words(SEED, STREAM, frame0, B, n) if channel == "bsc" else None
            for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
                ref_s = _device.channel_sent(channel, prec, param, words, SEED, STREAM, frame0)
                ref_0 = (torch.empty((B, n), dtype=dt, device="cuda"), torch.empty((B, n), dtype=torch.uint8, device="cuda") if channel == "bsc" else None)
                _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE[prec], param, 0, SEED, STREAM, frame0, B, n, ref_0[0].data_ptr(),
                                            None if ref_0[1] is None else ref_0[1].data_ptr(), st))
                for name, kind_host in pats.items():
                    kind = _dev(kind_host)
                    k0, k1, k2 = (torch.from_numpy(np.flatnonzero(kind_host == k)).cuda() for k in (0, 1, 2))
                    for sent, sent_host, ref in ((None, None, ref_0), (words, words_host, ref_s)):
                        where = (channel, frame0, prec, name, sent is not None)
                        pri, y = _device.channel_pattern(channel, prec, param, sent, 0, kind, SHORT, SEED, STREAM, frame0, B)
                        assert pri.dtype == dt and tuple(pri.shape) == (B, n)
                        assert torch.equal(pri[:, k0], ref[0][:, k0]), where
                        assert torch.equal(pri[:, k1], torch.zeros((B, k1.numel()), dtype=dt, device="cuda")) and not torch.signbit(pri[:, k1]).any(), where
                        assert torch.equal(pri[:, k2], torch.full((B, k2.numel()), SHORT, dtype=dt, device="cuda")), where
                        if channel == "bsc":
                            assert torch.equal(y[:, k0], ref[1][:, k0]) and not y[:, k1].any() and not y[:, k2].any(), where
                            want_pri, want_y = RO.bsc_pattern(param, sent_host, 0, kind_host, SHORT, SEED, STREAM, frame0, B,
                                                              np.float32 if prec == "f32" else np.float64, words=philox)
                            assert torch.equal(y, _dev(want_y)) and torch.equal(pri, _dev(want_pri)), where
                        else:
                            assert y is None
    torch.cuda.synchronize()


def test_channel_pattern_all_one_word_and_y_only():
    """codeword 1 without a shortened bit is ldpc_channel(codeword = 1) on the sent bits; the BSC without a priors buffer writes y alone."""
    torch = _torch()
    from ldpc_decoders_amd import _device, _lib

    B, n = 9, 70
    kind_host = np.zeros(n, dtype=np.uint8)
    kind_host[[0, 5, 69]] = 1
    kind = _dev(kind_host)
    k0 = torch.from_numpy(np.flatnonzero(kind_host == 0)).cuda()
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    for channel, param in (("biawgn", 2.0), ("bsc", 0.2)):
        ref = torch.empty((B, n), dtype=torch.float32, device="cuda")
        ry = torch.empty((B, n), dtype=torch.uint8, device="cuda")
        _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], 0, param, 1, SEED, STREAM, 77, B, n, ref.data_ptr(), ry.data_ptr(), st))
        pri, y = _device.channel_pattern(channel, "f32", param, None, 1, kind, SHORT, SEED, STREAM, 77, B)
        assert torch.equal(pri[:, k0], ref[:, k0]) and (channel == "biawgn" or torch.equal(y[:, k0], ry[:, k0]))
    y2 = torch.full((B, n), 9, dtype=torch.uint8, device="cuda")
    _lib.check(lib.ldpc_channel_pattern(_lib.CHANNEL["bsc"], 0, 0.2, None, 1, kind.data_ptr(), SHORT, SEED, STREAM, 77, B, n, None, y2.data_ptr(), st))
    assert torch.equal(y2, y)


def test_channel_pattern_refusals():
    """Every LDPC_E_ARG of the entry point, each with a sentence that names it; nothing is written."""
    torch = _torch()
    from ldpc_decoders_amd import _device, _lib

    B, n = 2, 8
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    sent_kind, short_kind = _dev(np.zeros(n, dtype=np.uint8)), _dev(np.array([0, 0, 2, 0, 0, 0, 0, 0], dtype=np.uint8))
    pri = torch.full((B, n), 7.0, dtype=torch.float32, device="cuda")
    y = torch.full((B, n), 7, dtype=torch.uint8, device="cuda")

    def call(channel, codeword=0, kind=sent_kind, short_llr=SHORT, sent=None):
        return lib.ldpc_channel_pattern(channel, 0, 0.1, sent, codeword, kind.data_ptr(), short_llr, SEED, STREAM, 0, B, n, pri.data_ptr(), y.data_ptr(), st)

    for ch in (_lib.CHANNEL["bec"], _lib.CHANNEL["biawgn"] | _lib.CH_RAW_OBSERVATION, _lib.CHANNEL["biawgn"] | _lib.ch_prior_grid(4),
               _lib.CHANNEL["bsc"] | _lib.ch_prior_grid(0)):
        assert call(ch) == -1 and lib.ldpc_last_error().startswith(b"ldpc_channel_pattern: "), ch
    for bad in (0.0, -32.0, float("inf"), float("nan")):
        assert call(_lib.CHANNEL["biawgn"], short_llr=bad) == -1 and b"ldpc_channel_pattern: short_llr" in lib.ldpc_last_error()
    for ch in ("biawgn", "bsc"):
        assert call(_lib.CHANNEL[ch], codeword=1, kind=short_kind) == -1 and b"ldpc_channel_pattern: the all-one word" in lib.ldpc_last_error()
        assert call(_lib.CHANNEL[ch], codeword=1, kind=sent_kind) == 0  # no shortened bit: the all-one word is sent
        assert call(_lib.CHANNEL[ch], codeword=0, kind=short_kind) == 0
        assert call(_lib.CHANNEL[ch], codeword=2) == -1
    with pytest.raises(_lib.LdpcHipError, match="ldpc_channel_pattern"):
        _device.channel_pattern("bec", "f32", 0.1, None, 0, sent_kind, SHORT, SEED, STREAM, 0, B)
    pri.fill_(7.0), y.fill_(7)
    assert call(_lib.CHANNEL["bec"]) == -1 and call(_lib.CHANNEL["biawgn"], short_llr=0.0) == -1
    torch.cuda.synchronize()
    assert (pri == 7.0).all() and (y == 7).all()


# ============================================================================================== 2. the tally
@pytest.mark.parametrize("B", [1, 4, 5, 2049])
def test_tally(B):
    """The counters of the numpy statement: errors on shortened bits count nothing, errors on punctured bits count; with and without
    per-frame words, with and without iteration counts, with and without a histogram; counters are accumulated into."""
    torch = _torch()
    from ldpc_decoders_amd import _lib

    n = 131
    rng = np.random.RandomState(B)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    kind_host = rng.choice(3, size=n, p=[0.6, 0.2, 0.2]).astype(np.uint8)
    kind = _dev(kind_host)
    sent_host = rng.randint(0, 2, size=(B, n)).astype(np.uint8)
    iters_host = rng.randint(0, 12, size=B).astype(np.int32)

    def run(xhat_host, sent, codeword, iters, bins, into):
        x, s, it = _dev(xhat_host), None if sent is None else _dev(sent), None if iters is None else _dev(iters)
        _lib.check(lib.ldpc_count_errors_pattern(x.data_ptr(), None if s is None else s.data_ptr(), codeword, kind.data_ptr(),
                                                 None if it is None else it.data_ptr(), B, n, bins, into.data_ptr(), st))
        torch.cuda.synchronize()
        return into.cpu().numpy()

    for sent, codeword in ((None, 0), (None, 1), (sent_host, 0)):
        base = np.full((B, n), codeword, dtype=np.uint8) if sent is None else sent
        flips = (rng.random_sample((B, n)) < 0.1).astype(np.uint8)
        flips[::3] = 0  # frames without an error
        only_short = base ^ (flips & (kind_host == 2)[None, :])
        only_punct = base ^ (flips & (kind_host == 1)[None, :])
        anywhere = base ^ flips
        for iters, bins in ((None, 0), (iters_host, 0), (iters_host, 8), (None, 8)):
            start = np.arange(4 + bins, dtype=np.int64) * 1000 + 17
            for xhat in (only_short, only_punct, anywhere):
                want = RO.tally(xhat, sent, codeword, kind_host, iters, bins)
                got = run(xhat, sent, codeword, iters, bins, _dev(start.copy()))
                assert np.array_equal(got, start + want), (sent is not None, codeword, iters is not None, bins)
            got = run(only_short, sent, codeword, iters, bins, torch.zeros(4 + bins, dtype=torch.int64, device="cuda"))
            assert got[0] == B and got[1] == 0 and got[2] == 0
            got = run(only_punct, sent, codeword, iters, bins, torch.zeros(4 + bins, dtype=torch.int64, device="cuda"))
            assert got[2] == (flips & (kind_host == 1)[None, :]).sum() and (B < 2049 or got[2] > 0)


# ============================================================================================== 3. the composition
# The flooding decoder runs on both of its backends on the two quasi-cyclic codes, and on the packaged (3,6) n = 1200 code in fp32 and fp64
# on both backends and with fp16 storage: every backend and precision a pattern can meet.  Each case asserts which kernels ran
# (``_ran_on``); a code without the backend a case names fails the case at ``DecoderHandle``'s refusal, it is not passed over.
# The pattern of the n = 1200 code punctures 27 bits and shortens 5; at 1.75 dB the C statement of min-sum on numpy noise under that pattern
# leaves a codeword in 16 .. 22 of 49 frames (three noise seeds, fp32 and fp64 alike), so 49 frames hold both kinds of frame for any seed.
BIG = "1200_3_6_rand_ldpc_1"
INTEGER = ["qc", "lqmsa", "slq"]
FLOODING_QC = [("f32", "stream"), ("f32", "fused")]
FLOODING_BIG = [("f32", "fused"), ("f32", "stream"), ("f64", "fused"), ("f64", "stream"), ("f16", "stream")]
COMPOSED = [(k, w) for k in KEYS for w in INTEGER + FLOODING_QC] + [(BIG, w) for w in FLOODING_BIG]
_HANDLES, _BIG = {}, {}


def _setup(key):
    """-> (oracle edge list, codes.Code)"""
    if key != BIG:
        return _code(key)[:2]
    if not _BIG:
        from ldpc_decoders_amd import codes

        c = codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, BIG + ".txt"))
        _BIG[0] = (O.Edges(c.m, c.n, c.edge_chk, c.edge_var), c)
    return _BIG[0]


def _snr(key):
    return 1.75 if key == BIG else _batch(key)[1]


def _pattern(key):
    from ldpc_decoders_amd import ratematch

    c = _setup(key)[1]
    if key == BIG:
        p = ratematch.Pattern(c.n, punctured=range(27), shortened=[40, 41, 100, 500, 1199])
    else:
        Z = _code(key)[3]
        p = ratematch.Pattern(c.n, punctured=ratematch.block_columns([0], Z), shortened=[Z + 1, Z + 2, 2 * Z + 1, 3 * Z + 2, 4 * Z + 2])
    assert p.unrecoverable(c).size == 0 and p.n_tx == c.n - p.punctured.size - 5
    return p


def _inner(key, which):
    """-> (handle, layers for the integer statement or None); ``which``: an integer family, "osd", or (precision, backend) of flooding MSA"""
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
        elif which == "osd":
            h, lay = _device.OsdHandle(_device.DecoderHandle(c, "NMSA", "f32", "auto")), None
        else:
            h, lay = _device.DecoderHandle(c, "MSA", which[0], which[1]), None
        _HANDLES[(key, which)] = (h, lay)
    return _HANDLES[(key, which)]


def _ran_on(inner, which):
    """A flooding decoder's last call ran on the kernels its case names."""
    if isinstance(which, tuple):
        assert inner.last_stats()[0] == which[1], (inner.last_stats(), which)
        assert (inner.kernel_name() != "") == (which[1] == "fused")


def _words(c, pattern, frame0, B):
    """The sent words of codeword -1, written out: the encoder of the shortened code, scattered through the index map on the host."""
    torch = _torch()
    short, index = pattern.shortened_code(c)
    w = short.encoder().handle(torch.cuda.current_device()).encode_random(SEED, STREAM, frame0, B).cpu().numpy()
    full = np.zeros((B, c.n), dtype=np.uint8)
    full[:, index] = w
    return full


def _counters(bins=0):
    return _torch().zeros(4 + bins, dtype=_torch().int64, device="cuda")


@pytest.mark.parametrize("codeword", [0, -1])
@pytest.mark.parametrize("key,which", COMPOSED, ids=str)
def test_simulate_equals_the_pipeline_written_out(key, which, codeword, monkeypatch):
    """PatternHandle.simulate over 3 chunks + 1 frame == ldpc_channel_pattern -> the inner decode -> the numpy tally, at codeword 0 and -1; the
    counters do not depend on the chunk size; for the integer families the integer statement decodes the device priors to the same
    counters; with shortened bits every sent word is a codeword that is zero on the shortened set."""
    torch = _torch()
    from ldpc_decoders_amd import _device

    inner, lay = _inner(key, which)
    g, c = _setup(key)
    snr = _snr(key)
    pattern = _pattern(key)
    bins, frame0, chunk = 8, 2 ** 33 + 1000, 16
    B = 3 * chunk + 1
    ph = _device.PatternHandle(inner, pattern)
    monkeypatch.setattr(_device.PatternHandle, "CHUNK", chunk)
    cnt = _counters(bins)
    ph.simulate("biawgn", snr, codeword, SEED, STREAM, frame0, B, CAP, cnt, hist_bins=bins)
    got = cnt.cpu().numpy()
    _ran_on(inner, which)
    # the same pipeline, written out
    sent_host = _words(c, pattern, frame0, B) if codeword == -1 else None
    if sent_host is not None:
        assert not c.syndrome(sent_host).any() and not sent_host[:, pattern.shortened].any() and sent_host.any()
        assert torch.equal(ph.sent_words(SEED, STREAM, frame0, B), _dev(sent_host))
    kind = _dev(pattern.kind)
    pri, y = _device.channel_pattern("biawgn", inner.precision, snr, None if sent_host is None else _dev(sent_host), max(codeword, 0), kind, SHORT,
                                     SEED, STREAM, frame0, B)
    assert pri.dtype == (torch.float64 if inner.precision == "f64" else torch.float32)
    xhat, iters = inner.decode_device(pri, y, CAP)[:2]
    torch.cuda.synchronize()
    xhat, iters = xhat.cpu().numpy(), iters.cpu().numpy()
    want = RO.tally(xhat, sent_host, max(codeword, 0), pattern.kind, iters, bins)
    print(key, which, codeword, "snr", snr, "counters", got.tolist())
    assert np.array_equal(got, want), (got, want)
    reached = O.syndrome_ok(g, xhat.astype(np.int64))
    assert 0 < reached.sum() < B, reached.sum()  # frames that reach a codeword and frames that do not
    # any chunk size
    for other in (7, None):
        monkeypatch.setattr(_device.PatternHandle, "CHUNK", other)
        cnt2 = _counters(bins)
        ph.simulate("biawgn", snr, codeword, SEED, STREAM, frame0, B, CAP, cnt2, hist_bins=bins)
        assert np.array_equal(cnt2.cpu().numpy(), got), other
    # the integer statement on the device priors
    if lay is not None:
        x, it, _, _ = LQ.lqmsa_decode(g, None, pri.cpu().numpy(), CAP, layers=lay)
        assert np.array_equal(RO.tally(x, sent_host, max(codeword, 0), pattern.kind, it, bins), got)


@pytest.mark.parametrize("key,which", [(("dense", 7), "qc"), (BIG, ("f32", "fused"))], ids=str)
def test_the_all_one_word(key, which, monkeypatch):
    """codeword 1 under a pattern without a shortened bit (every check of both codes has degree 6): the handle sends words of ones, so no
    call waits for the stream; the counters are those of ldpc_channel_pattern without words at codeword 1, the decode and the numpy tally."""
    torch = _torch()
    from ldpc_decoders_amd import _device, ratematch

    inner = _inner(key, which)[0]
    c = _setup(key)[1]
    pattern = ratematch.Pattern(c.n, punctured=_pattern(key).punctured)
    B, frame0 = 49, 321
    monkeypatch.setattr(_device.PatternHandle, "CHUNK", 16)
    cnt = _counters()
    _device.PatternHandle(inner, pattern).simulate("biawgn", _snr(key), 1, SEED, STREAM, frame0, B, CAP, cnt)
    _ran_on(inner, which)
    pri, y = _device.channel_pattern("biawgn", inner.precision, _snr(key), None, 1, _dev(pattern.kind), SHORT, SEED, STREAM, frame0, B)
    xhat, iters = inner.decode_device(pri, y, CAP)[:2]
    torch.cuda.synchronize()
    want = RO.tally(xhat.cpu().numpy(), None, 1, pattern.kind, iters.cpu().numpy(), 0)
    assert np.array_equal(cnt.cpu().numpy(), want) and 0 < want[1] < B, (cnt, want)


def test_a_byte_above_two_reads_as_shortened():
    """Not a kind; the channel and the tally agree on it: the prior of a shortened bit, and no error counted."""
    torch = _torch()
    from ldpc_decoders_amd import _device, _lib

    B, n = 3, 8
    kind = _dev(np.array([0, 3, 255, 2, 1, 0, 0, 7], dtype=np.uint8))
    for channel, param in (("biawgn", 2.0), ("bsc", 0.1)):
        pri, y = _device.channel_pattern(channel, "f32", param, None, 0, kind, SHORT, SEED, STREAM, 0, B)
        assert (pri[:, [1, 2, 3, 7]] == SHORT).all() and (pri[:, 4] == 0).all() and (y is None or not y[:, [1, 2, 3, 4, 7]].any())
    cnt = _counters()
    xhat = _dev(np.array([[0, 1, 1, 1, 0, 0, 0, 1], [0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint8))
    _lib.check(_lib.load().ldpc_count_errors_pattern(xhat.data_ptr(), None, 0, kind.data_ptr(), None, B, n, 0, cnt.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert cnt.cpu().tolist() == [3, 1, 1, 0]


@pytest.mark.parametrize("codeword", [0, -1])
@pytest.mark.parametrize("which", INTEGER + ["osd"])
@pytest.mark.parametrize("key", KEYS, ids=str)
def test_empty_pattern_equals_the_inner_simulate(key, which, codeword):
    """With every bit sent the counters are those of the inner handle's own simulate (its C pass draws with the channel kernel)."""
    from ldpc_decoders_amd import _device, ratematch

    inner = _inner(key, which)[0]
    c = _setup(key)[1]
    snr = _snr(key)
    B, frame0, bins = 49, 5000, 8
    want, got = _counters(bins), _counters(bins)
    inner.simulate("biawgn", snr, codeword, SEED, STREAM, frame0, B, CAP, want, hist_bins=bins)
    _device.PatternHandle(inner, ratematch.Pattern(c.n)).simulate("biawgn", snr, codeword, SEED, STREAM, frame0, B, CAP, got, hist_bins=bins)
    want, got = want.cpu().numpy(), got.cpu().numpy()
    assert np.array_equal(got, want) and got[0] == B and (which == "osd" or 0 < got[1] < B), (got, want)


@pytest.mark.parametrize("channel,param", [("biawgn", None), ("bsc", 0.06)])
@pytest.mark.parametrize("key,which", [(k, w) for k in KEYS for w in FLOODING_QC] + [(BIG, w) for w in FLOODING_BIG], ids=str)
def test_empty_pattern_equals_channel_decode_count(key, which, channel, param):
    """DecoderHandle: against channel_device + decode + ldpc_count_errors (the fused simulate draws inside its kernel; its equality is not
    claimed)."""
    torch = _torch()
    from ldpc_decoders_amd import _device, _lib, ratematch

    inner = _inner(key, which)[0]
    c = _setup(key)[1]
    param = _snr(key) if param is None else param
    B, frame0, bins = 49, 5000, 8
    pri, y = inner.channel_device(channel, param, 0, SEED, STREAM, frame0, B)
    xhat, iters = inner.decode_device(pri, y, CAP)
    want, got = _counters(bins), _counters(bins)
    _lib.check(_lib.load().ldpc_count_errors(xhat.data_ptr(), None, 0, iters.data_ptr(), B, c.n, bins, want.data_ptr(), torch.cuda.current_stream().cuda_stream))
    _device.PatternHandle(inner, ratematch.Pattern(c.n)).simulate(channel, param, 0, SEED, STREAM, frame0, B, CAP, got, hist_bins=bins)
    _ran_on(inner, which)
    want, got = want.cpu().numpy(), got.cpu().numpy()
    assert np.array_equal(got, want) and got[0] == B and (channel == "bsc" or 0 < got[1] < B), (got, want)


def test_bsc_composition_equals_the_numpy_channel():
    """Over the BSC the whole pass is integers: the numpy channel of the pattern, the integer statement and the numpy tally give the counters."""
    from ldpc_decoders_amd import _device

    key = ("dense", 7)
    g = _code(key)[0]
    inner, lay = _inner(key, "qc")
    pattern = _pattern(key)
    B, frame0, p = 33, 123, 0.05
    cnt = _counters()
    _device.PatternHandle(inner, pattern).simulate("bsc", p, 0, SEED, STREAM, frame0, B, CAP, cnt)
    pri, y = RO.bsc_pattern(p, None, 0, pattern.kind, SHORT, SEED, STREAM, frame0, B, np.float32)
    x, it, _, _ = LQ.lqmsa_decode(g, y, pri, CAP, layers=lay)
    assert np.array_equal(cnt.cpu().numpy(), RO.tally(x, None, 0, pattern.kind, it, 0))


def test_refusals():
    """Each a ValueError with one sentence, before any device call (the refused handles are never created on the device)."""
    from ldpc_decoders_amd import _device, _lib, ratematch

    key = ("dense", 7)
    c = _code(key)[1]
    pattern = _pattern(key)
    for cls in (_device.HardHandle, _device.AdmmHandle, _device.MlHandle, _device.BecMlHandle):
        with pytest.raises(ValueError):
            _device.PatternHandle(cls.__new__(cls), pattern)
    bec = _device.DecoderHandle.__new__(_device.DecoderHandle)
    bec.alg = "BEC"
    for bad in (bec, object()):
        with pytest.raises(ValueError):
            _device.PatternHandle(bad, pattern)
    inner = _inner(key, "qc")[0]
    with pytest.raises(ValueError):
        _device.PatternHandle(inner, ratematch.Pattern(c.n + 1))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            _device.PatternHandle(inner, pattern, short_llr=bad)
    ph = _device.PatternHandle(inner, pattern)
    cnt = _counters()
    with pytest.raises(ValueError, match="bec"):
        ph.simulate("bec", 0.1, 0, SEED, STREAM, 0, 4, CAP, cnt)
    with pytest.raises(ValueError, match="prior-grid"):
        ph.simulate("biawgn", 2.0, 0, SEED, STREAM, 0, 4, CAP, cnt, flags=_lib.flag_prior_grid(4))
    with pytest.raises(ValueError, match="all-one"):
        ph.simulate("biawgn", 2.0, 1, SEED, STREAM, 0, 4, CAP, cnt)
    with pytest.raises(ValueError, match="--exact"):
        _device.check_pattern_run("biawgn", exact=True)
    assert not cnt.cpu().numpy().any()


def test_cli(tmp_path, monkeypatch):
    """One command-line run under a pattern: the result file carries the puncture / shorten keys, and the BER is over the counted bits."""
    from ldpc_decoders_amd import codes, main, qc

    code_dir = tmp_path / "codes"
    monkeypatch.setenv(codes.file_codes_dir_string, str(code_dir))
    qc.gen_rand_qc(qc.setup_parser().parse_args("1 4 8 27 --seed 5 --dir".split() + [str(code_dir)]))
    argv = "biawgn 216_qc_4x8_z27_1 QCMSA --params 3.0 --max-iter 20 --batch 4096 --max-frames 4096 --codeword -1".split()
    main.main(argv + ["--puncture-cols", "7", "--shorten", "30:35", "--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-216_qc_4x8_z27_1-QCMSA--1-100-20-6-2-0.8125-0.0-27-189:216-30:35.json")) as fp:
        res = json.load(fp)
    assert res["puncture"] == "189:216" and res["shorten"] == "30:35" and res["qc_lift"] == 27
    tot, wec, bec = res["tot"]["3.0"], res["wec"]["3.0"], res["bec"]["3.0"]
    assert tot == 4096 and 4 <= wec < tot and wec <= bec <= wec * 211
    assert res["ber"]["3.0"] == pytest.approx(bec / (tot * 211)) and res["wer"]["3.0"] == pytest.approx(wec / tot)

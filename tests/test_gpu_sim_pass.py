"""The second and the ragged last pass of every *_simulate (csrc/ldpc_sim.hpp) and of the random-codeword loop (_device.simulate_random_codewords):
150 frames from frame 1000 on in passes of 64, 64 and 22, against the same frames in one piece -- the channel kernel for the whole range, the
family's decode_device, ldpc_count_errors -- whose parts the family's own test file holds to its oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED, STREAM = 0x5151FA55, 9
B, FRAME0, PASS, CAP = 150, 1000, 64, 10
BINS = CAP + 1

# family -> (channel, param) pairs; the smallest code of the family's own test file: 12_3_4_ldpc, and for QC the dense 3 x 6 base (Z = 7)
FAMILIES = {
    "hard-stream": [("bsc", 0.08), ("biawgn", 3.0)],
    "hard-fused": [("bsc", 0.08), ("biawgn", 3.0)],
    "osd": [("biawgn", 1.5), ("bsc", 0.08)],
    "bec_ml": [("bec", 0.4)],
    "lqmsa": [("biawgn", 2.0), ("bsc", 0.08)],
    "qc": [("biawgn", 1.0), ("bsc", 0.06)],
    "slq": [("biawgn", 2.0), ("bsc", 0.08)],
}
CASES = [(f, ch, p) for f, chans in FAMILIES.items() for ch, p in chans]


def _family(name):
    """-> (handle with simulate(), code, decode(fp32 priors or None, y or None, frame0) -> (xhat, iters or None))"""
    import torch

    from ldpc_decoders_amd import _device as D
    from ldpc_decoders_amd import codes, qc

    code = codes.get_code("12_3_4_ldpc")
    if name.startswith("hard"):
        h = D.HardHandle(code, name.split("-")[1])
        return h, code, lambda pri, y, f0: h.decode_device(y if y is not None else (pri < 0).to(torch.uint8), CAP)
    if name == "osd":
        bp = D.DecoderHandle(code, "NMSA", "f32")
        bp.set_correction(0.8125, 0.0)
        h = D.OsdHandle(bp, order=1, depth=8)
        return h, code, lambda pri, y, f0: h.decode_device(pri, y, CAP)[:2]
    if name == "bec_ml":
        h = D.BecMlHandle(code)
        return h, code, lambda pri, y, f0: (h.decode_device(y, SEED, STREAM, f0)[0], None)
    if name == "qc":
        code = qc.rand_qc_ldpc(np.ones((3, 6), dtype=bool), 7, np.random.RandomState(107), girth6=True)
        h = D.QcHandle(code, 7)
    else:
        h = {"lqmsa": D.LqmsaHandle, "slq": D.SlqHandle}[name](code)
    return h, code, lambda pri, y, f0: h.decode_device(pri, y, CAP)


def _channel(channel, param, code, codeword, sent=None):
    """the channel kernel for frames [FRAME0, FRAME0 + B) in one piece: of the all-`codeword` word, or of the words `sent`"""
    import torch

    from ldpc_decoders_amd import _lib

    lib, n, st = _lib.load(), code.n, torch.cuda.current_stream().cuda_stream
    pri = None if channel == "bec" else torch.empty((B, n), dtype=torch.float32, device="cuda")
    y = None if channel == "biawgn" else torch.empty((B, n), dtype=torch.uint8, device="cuda")
    ptr = (None if pri is None else pri.data_ptr(), None if y is None else y.data_ptr(), st)
    if sent is None:
        _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE["f32"], float(param), codeword, SEED, STREAM, FRAME0, B, n, *ptr))
    else:
        _lib.check(lib.ldpc_channel_sent(_lib.CHANNEL[channel], _lib.DTYPE["f32"], float(param), sent.data_ptr(), SEED, STREAM, FRAME0, B, n, *ptr))
    return pri, y


def _counters(bins):
    import torch

    return torch.zeros(4 + bins, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("family,channel,param", CASES)
def test_simulate_in_three_passes_counts_what_one_piece_counts(family, channel, param, monkeypatch):
    import torch

    from ldpc_decoders_amd import _lib

    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    h, code, decode = _family(family)
    bins = 0 if family == "bec_ml" else BINS  # the elimination decoder has no iterations to count
    monkeypatch.setenv("LDPC_SIM_PASS_FRAMES", str(PASS))
    for codeword in (0, 1):  # every check of these codes has even degree
        got = _counters(bins)
        h.simulate(channel, param, codeword, SEED, STREAM, FRAME0, B, CAP, got, hist_bins=bins)
        pri, y = _channel(channel, param, code, codeword)
        xhat, iters = decode(pri, y, FRAME0)
        want = _counters(bins)
        _lib.check(lib.ldpc_count_errors(xhat.data_ptr(), None, codeword, None if iters is None else iters.data_ptr(), B, code.n, bins,
                                         want.data_ptr(), st))
        print(family, channel, "codeword", codeword, "simulate", got.tolist(), "one piece", want.tolist())
        assert torch.equal(got, want) and int(got[_lib.CNT_TOT]) == B and int(got[_lib.CNT_BEC]) > 0


def test_the_knob_lowers_the_pass_and_ignores_what_is_no_positive_integer(monkeypatch):
    """SlqHandle's profile counts decode calls, one per pass: three with the knob at 64, one where the knob is unset, 0, not a number, or
    above the family's own rule; the counters are those of the frames in one piece every time."""
    import torch

    from ldpc_decoders_amd import _lib

    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    h, code, decode = _family("slq")
    pri, y = _channel("bsc", 0.08, code, 0)
    xhat, iters = decode(pri, y, FRAME0)
    want = _counters(BINS)
    _lib.check(lib.ldpc_count_errors(xhat.data_ptr(), None, 0, iters.data_ptr(), B, code.n, BINS, want.data_ptr(), st))
    h.profile(True)
    for value, passes in ((str(PASS), 3), (None, 1), ("0", 1), ("-64", 1), ("sixty-four", 1), ("64 frames", 1), (str(1 << 40), 1)):
        if value is None:
            monkeypatch.delenv("LDPC_SIM_PASS_FRAMES", raising=False)
        else:
            monkeypatch.setenv("LDPC_SIM_PASS_FRAMES", value)
        h.read_profile(reset=True)
        got = _counters(BINS)
        h.simulate("bsc", 0.08, 0, SEED, STREAM, FRAME0, B, CAP, got, hist_bins=BINS)
        assert torch.equal(got, want), value
        assert h.read_profile()["decode_total"][1] == passes, value


RANDOM = ["decoder", "bec_ml", "osd", "hard-stream", "hard-fused", "lqmsa", "qc", "slq"]


@pytest.mark.parametrize("family", RANDOM)
def test_random_codewords_in_three_chunks_count_what_one_piece_counts(family, monkeypatch):
    import torch

    from ldpc_decoders_amd import _device as D
    from ldpc_decoders_amd import _lib, codes

    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    if family == "decoder":  # a code without a code book: the built-in toy codes take the code-book path
        code = codes.get_code("512_3_6_rand_ldpc_1")
        assert getattr(code, "cb", None) is None
        h = D.DecoderHandle(code, "MSA", "f32")
        decode = lambda pri, y, f0: h.decode_device(pri, y, CAP)  # noqa: E731
        channel, param = "bsc", 0.05
    else:
        h, code, decode = _family(family)
        channel, param = FAMILIES[family][-1]
    bins = 0 if family == "bec_ml" else BINS
    monkeypatch.setattr(h, "words_chunk", lambda channel: PASS)
    got = _counters(bins)
    h.simulate(channel, param, -1, SEED, STREAM, FRAME0, B, CAP, got, hist_bins=bins)
    sent = code.encoder().handle().encode_random(SEED, STREAM, FRAME0, B)
    assert int(sent.sum()) > 0
    pri, y = _channel(channel, param, code, 0, sent=sent)
    xhat, iters = decode(pri, y, FRAME0)
    want = _counters(bins)
    _lib.check(lib.ldpc_count_errors_words(xhat.data_ptr(), sent.data_ptr(), None if iters is None else iters.data_ptr(), B, code.n, bins,
                                           want.data_ptr(), st))
    print(family, channel, "simulate", got.tolist(), "one piece", want.tolist())
    assert torch.equal(got, want) and int(got[_lib.CNT_TOT]) == B and int(got[_lib.CNT_BEC]) > 0

"""The GF(2) encoder (csrc/ldpc_encode.hip: k_info, k_encode<1 | 2 | 4 | 8>) and ldpc_channel_sent at their shape, batch and counter edges,
on the (k, r) family of tests/encoder_codes.py (held to its promises by test_encoder_codes_cpu.py).

Every statement is exact.  A word is compared with (a) sent[info positions] == u and H . sent == 0 -- the information positions are an
information set, so this pins the word without P -- (b) the numpy int64 statement Encoder.encode, and, in random mode, (c) u from the
oracle's Philox.  The only tolerance in the file is the BI-AWGN bound that test_gpu_channel_sim.py already holds the zero-word kernel to.
"""
import math

import numpy as np
import pytest

import bp_oracle as O
import encoder_codes as EC

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 8
SEED, STREAM, FRAME0 = 0x5EED0123456789, 6, 7_000_000_123


def _setup(k, r):
    code = EC.shape_code(k, r)
    enc = code.encoder()
    h = enc.handle()
    info = h.info()
    assert (info["nt"], info["cgroups"], info["kgroups"], info["chunks"]) == EC.EXPECTED[(k, r)]  # what this shape is here to reach
    return code, enc, h


def _buffer(B, n):
    import torch

    return torch.full((B + GUARD, n), POISON, dtype=torch.uint8, device="cuda")


def _encode(h, u, B):
    """given-u mode into the first B rows of a poisoned [B + 8, n] buffer -> the B rows (numpy); the guard rows must come back untouched"""
    import torch

    buf = _buffer(B, h.enc.n)
    h.encode(torch.from_numpy(np.ascontiguousarray(u)).cuda(), out=buf[:B])
    got = buf.cpu().numpy()
    assert (got[B:] == POISON).all()
    return got[:B]


def _random(h, frame0, B):
    buf = _buffer(B, h.enc.n)
    h.encode_random(SEED, STREAM, frame0, B, out=buf[:B])
    got = buf.cpu().numpy()
    assert (got[B:] == POISON).all()
    return got[:B]


def _hold(code, enc, sent, u, tag):
    u = u & 1
    assert sent.shape == (len(u), code.n) and (sent <= 1).all(), tag  # every position written, with a bit
    assert (sent[:, enc.info_positions] == u).all(), tag
    assert not ((sent.astype(np.int64) @ code.parity_mtx.T) & 1).any(), tag  # (a) with the line above
    assert (sent == enc.encode(u)).all(), tag  # (b)


def _both_modes(code, enc, h, B, tag):
    u = EC.info_words(enc.k, B, 17 + B)
    _hold(code, enc, _encode(h, u, B), u, (tag, B, "given u"))
    _hold(code, enc, _random(h, FRAME0, B), EC.philox_info_bits(SEED, STREAM, FRAME0, B, enc.k), (tag, B, "random"))  # (c)


@pytest.mark.parametrize("B", [33, 129])
@pytest.mark.parametrize("k,r", EC.SHAPES)
def test_every_shape_both_modes(k, r, B):
    code, enc, h = _setup(k, r)
    _both_modes(code, enc, h, B, (k, r))


@pytest.mark.parametrize("k,r", [(17, 33), (128, 257), (8193, 40)])
def test_batch_sweep(k, r):
    """nt = 2; nt = 4 in three column groups, three tiles of them padding; two chunks of k_info (B = 33: 66 waves in 17 blocks, two idle).
    B around the 32-frame MFMA tile (fr < B) and the 128-frame block (fbase >= B)."""
    import torch

    from ldpc_decoders_amd import _lib

    code, enc, h = _setup(k, r)
    for B in (1, 31, 32, 33, 127, 128, 129):
        _both_modes(code, enc, h, B, (k, r))
    # B = 0: nothing is written, by the handle or by the library
    assert _encode(h, np.zeros((0, k), dtype=np.uint8), 0).shape == (0, code.n) and _random(h, FRAME0, 0).shape == (0, code.n)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    buf, u = _buffer(0, code.n), torch.zeros((1, k), dtype=torch.uint8, device="cuda")
    _lib.check(lib.ldpc_encode(h.h, u.data_ptr(), 0, buf.data_ptr(), st))
    _lib.check(lib.ldpc_encode_random(h.h, SEED, STREAM, FRAME0, 0, buf.data_ptr(), st))
    assert (buf.cpu().numpy() == POISON).all()


def test_words_buffer_is_reused_across_batch_sizes():
    """The packed information words of given-u mode live in a workspace of the handle: a large, a small and a large batch again."""
    code, enc, h = _setup(8193, 40)
    for i, B in enumerate((129, 1, 129)):
        u = EC.info_words(enc.k, B, 300 + i)
        _hold(code, enc, _encode(h, u, B), u, ("reuse", i, B))


@pytest.mark.parametrize("k,r", [(17, 33), (129, 96)])
def test_information_bytes_count_by_their_low_bit(k, r):
    code, enc, h = _setup(k, r)
    B = 33
    u = EC.info_words(k, B, 5)
    high = EC.info_words(k, B, 6) << 1
    assert set(np.unique(u | high)) == {0, 1, 2, 3}
    got = _encode(h, u | high, B)
    _hold(code, enc, got, u, (k, r, "bytes 2 and 3"))


@pytest.mark.parametrize("k,r", EC.CARRY_SHAPES)
def test_random_mode_across_the_frame_counter_carry(k, r):
    """Frames 2^32 - 20 .. 2^32 + 19: the global frame index carries from the low Philox counter word into the high one; and the same
    frames in two calls split at 13."""
    code, enc, h = _setup(k, r)
    f0, B, cut = EC.CARRY_FRAME0, EC.CARRY_B, EC.CARRY_SPLIT
    whole = _random(h, f0, B)
    _hold(code, enc, whole, EC.philox_info_bits(SEED, STREAM, f0, B, k), (k, r, "carry"))
    two = np.concatenate([_random(h, f0, cut), _random(h, f0 + cut, B - cut)])
    assert (two == whole).all()
    # the carry took place: frame 2^32 + j is not frame j
    assert (_random(h, 0, 20)[:, enc.info_positions] != whole[20:, enc.info_positions]).any(axis=1).all()


@pytest.mark.parametrize("B", [33, 129])
def test_rank_n_code_has_only_the_zero_word(B):
    code, enc, h = _setup(0, 33)
    assert enc.k == 0 and code.n == 33
    for got in (_encode(h, np.zeros((B, 0), dtype=np.uint8), B), _random(h, FRAME0, B)):
        assert got.shape == (B, 33) and not got.any()


@pytest.mark.parametrize("B", [33, 129])
def test_rank_0_code_sends_the_information_word(B):
    code, enc, h = _setup(40, 0)
    assert enc.rank == 0 and (enc.info_positions == np.arange(40)).all()
    u = EC.info_words(40, B, 9)
    assert (_encode(h, u, B) == u).all()
    assert (_random(h, FRAME0, B) == EC.philox_info_bits(SEED, STREAM, FRAME0, B, 40)).all()


# ---- ldpc_channel_sent: the channel of a given word per frame ---------------------------------------------------------------------------

CH_FRAME0 = (1 << 32) - 100  # B = 257 crosses the carry of the frame counter here as well
CH_SHAPES = [(n, B) for n in (5, 6, 7, 8, 33) for B in (1, 257)]  # every n mod 4 and one n above 32; a 256-thread block ends mid-frame


def _sent(n, B):
    return np.random.RandomState(1000 * n + B).randint(0, 2, (B, n)).astype(np.uint8)


def _channel_sent(channel, prec, param, sent, want_priors=True, want_y=True):
    """ldpc_channel_sent on `sent` (numpy [B, n]) -> (priors or None, y or None); each output lies in front of 8 poisoned elements that
    must come back untouched"""
    import torch

    from ldpc_decoders_amd import _lib

    B, n = sent.shape
    dt = torch.float64 if prec == "f64" else torch.float32
    pri = torch.full((B * n + GUARD,), -77.0, dtype=dt, device="cuda") if want_priors else None
    y = torch.full((B * n + GUARD,), POISON, dtype=torch.uint8, device="cuda") if want_y else None
    s = torch.from_numpy(sent).cuda()
    _lib.check(_lib.load().ldpc_channel_sent(_lib.CHANNEL[channel], _lib.DTYPE[prec], float(param), s.data_ptr(), SEED, STREAM, CH_FRAME0, B, n,
                                             None if pri is None else pri.data_ptr(), None if y is None else y.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    out = []
    for t, fill in ((pri, -77.0), (y, POISON)):
        if t is None:
            out.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[B * n:] == fill).all()
        out.append(a[:B * n].reshape(B, n))
    return out


def _channel_zero_word(channel, prec, param, B, n):
    """ldpc_channel(codeword = 0) for the same frames"""
    import torch

    from ldpc_decoders_amd import _lib

    dt = torch.float64 if prec == "f64" else torch.float32
    pri = None if channel == "bec" else torch.empty((B, n), dtype=dt, device="cuda")
    y = None if channel == "biawgn" else torch.empty((B, n), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE[prec], float(param), 0, SEED, STREAM, CH_FRAME0, B, n,
                                        None if pri is None else pri.data_ptr(), None if y is None else y.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    return None if pri is None else pri.cpu().numpy(), None if y is None else y.cpu().numpy()


def _hits(p, B, n):
    thr = int(np.ceil(p * 4294967296.0 - 0.5))
    return np.stack([O.philox_frame_words(SEED, STREAM, CH_FRAME0 + f, n).astype(np.uint64) < thr for f in range(B)])


@pytest.mark.parametrize("n,B", CH_SHAPES)
def test_bsc_of_a_sent_word(n, B):
    p = 0.11
    sent, hit = _sent(n, B), _hits(p, B, n)
    want_y = sent ^ hit.astype(np.uint8)
    llr = math.log(1.0 - p) - math.log(p)  # the library's double; rounded once to the type below
    if B > 1:
        assert hit.any() and (sent[hit] == 0).any() and (sent[hit] == 1).any()  # flips of both bits: y and sent differ where it matters
    for prec, dt in (("f64", np.float64), ("f32", np.float32)):
        pri, y = _channel_sent("bsc", prec, p, sent)
        assert (y == want_y).all(), prec
        assert pri.dtype == dt and (pri == dt(llr) * (1 - 2 * want_y.astype(np.int64)).astype(dt)).all(), prec
        _, y_only = _channel_sent("bsc", prec, p, sent, want_priors=False)
        assert (y_only == want_y).all(), prec
        p0, y0 = _channel_zero_word("bsc", prec, p, B, n)
        pz, yz = _channel_sent("bsc", prec, p, np.zeros_like(sent))
        assert (yz == y0).all() and pz.tobytes() == p0.tobytes(), prec


@pytest.mark.parametrize("n,B", CH_SHAPES)
def test_bec_of_a_sent_word(n, B):
    p = 0.37
    sent, hit = _sent(n, B), _hits(p, B, n)
    if B > 1:
        assert hit.any() and not hit.all() and sent[~hit].any()
    _, y = _channel_sent("bec", "f32", p, sent, want_priors=False)
    assert (y == np.where(hit, 2, sent)).all()
    _, yz = _channel_sent("bec", "f32", p, np.zeros_like(sent), want_priors=False)
    assert (yz == _channel_zero_word("bec", "f32", p, B, n)[1]).all()


@pytest.mark.parametrize("prec,tol", [("f64", 1e-9), ("f32", 3e-5)])
@pytest.mark.parametrize("n,B", CH_SHAPES)
def test_biawgn_of_a_sent_word(n, B, prec, tol):
    """Measure and bounds of test_gpu_channel_sim.py::test_biawgn_priors_match_fp64_model (the zero-word kernel).  Measured on an MI355X over
    the ten shapes: at most 4.9e-15 in fp64 and 1.6e-6 in fp32 (the fp32 kernel draws its normals in fp32; the model is fp64)."""
    snr = 2.0
    sent = _sent(n, B)
    var = O.biawgn_noise_var(snr)
    z = np.stack([O.device_biawgn_noise(SEED, STREAM, CH_FRAME0 + f, n) for f in range(B)])
    want = -2 * ((2.0 * sent - 1) + np.sqrt(var) * z) / var
    pri, _ = _channel_sent("biawgn", prec, snr, sent, want_y=False)
    assert pri.dtype == (np.float64 if prec == "f64" else np.float32)
    err = np.max(np.abs(pri.astype(np.float64) - want) / (1 + np.abs(want)))
    print("biawgn_sent %s n=%d B=%d: max |got - want| / (1 + |want|) = %.3e (bound %.0e)" % (prec, n, B, err, tol))
    assert err <= tol
    # an all-zero word gives the bytes of ldpc_channel(codeword = 0)
    pz, _ = _channel_sent("biawgn", prec, snr, np.zeros_like(sent), want_y=False)
    assert pz.tobytes() == _channel_zero_word("biawgn", prec, snr, B, n)[0].tobytes()

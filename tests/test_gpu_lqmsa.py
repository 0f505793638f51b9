"""Layered fixed-point min-sum on the GPU (csrc/ldpc_lqmsa.hip, ldpc_lqmsa_*): decisions -- as bytes and as packed words -- iteration counts
and soft outputs equal to the integer statement of lqmsa_oracle.py with ``==``: every code shape and check degree, fp32 and fp64 priors,
the iteration-0 rule, every wave count, any batch size and frame position, custom layerings, the refusals, the simulate composition and the
command line."""
import json
import os

import numpy as np
import pytest

import bp_oracle as O
import edge_codes as EC
import lmsa_oracle as L
import lqmsa_oracle as LQ
from helpers import CODES_DIR

pytestmark = pytest.mark.gpu
SEED, STREAM = 0x1A7E5EED, 5
E_ARG, E_UNSUPPORTED = -1, -4  # include/ldpc_hip.h
NO_EARLY_EXIT = 1
DEFAULT = (6, 2, 0.8125, 0)
PARAMS = [DEFAULT, (2, 0, 1.0, 0), (8, 1, 1.0, 1), (5, 1, 1 / 64, 0), (6, 2, 0.5, 3)]
SHIPPED = ["12_3_4_ldpc", "512_3_6_rand_ldpc_1", "1200_3_6_rand_ldpc_1", "1200_rho_x5_rand_ldpc_1", "margulis"]
SHAPES = [(9, 31, 3), (63, 96, 3), (64, 127, 3), (65, 128, 3), (129, 200, 3)]
DEGREES = [2, 3, 7, 8, 9, 16, 17, 33]
# Checks of degree 2 only say "these two bits are equal": the code is a repetition code on every connected component, min-sum on it is a
# consensus and reaches a codeword at every SNR, so no SNR leaves a third of the frames at the cap.  That code is run at -9 dB instead,
# where the frames leave after 1 .. 6 sweeps (asserted: at least four different counts).
CONSENSUS = ("dc", 2)
_CODES, _BATCH, _WANT = {}, {}, {}


def _code(key):
    """key: a shipped name, ("shape", m, n, redundant) or ("dc", d) -> (oracle edge list, codes.Code)"""
    from ldpc_decoders_amd import codes

    if key not in _CODES:
        if isinstance(key, str):
            c = codes.get_code(key)
        elif key[0] == "shape":
            c = EC.shape_code(*key[1:])
        else:  # (3, dc)-regular at the smallest n that gives at least 65 checks: n = 22 dc, m = 66
            c = codes.rand_reg_ldpc(22 * key[1], 3, key[1], np.random.RandomState(100 + key[1]))
            assert c.m == 66
        _CODES[key] = (O.Edges(c.m, c.n, c.edge_chk, c.edge_var), c)
    return _CODES[key]


def _handle(key, params=None, layers=None):
    from ldpc_decoders_amd._device import LqmsaHandle

    h = LqmsaHandle(_code(key)[1])
    if params is not None:
        h.set_fixed_point(*params)
    if layers is not None:
        h.set_layers(layers)
    return h


def _priors(g, snr, z):
    return O.biawgn_priors(-1 + np.sqrt(O.biawgn_noise_var(snr)) * z, snr)


def _batch(key, B=64, cap=50):
    """fp64 BI-AWGN priors [B, n] at an SNR where the oracle (default parameters, greedy layers) says that between a third and two thirds of
    the frames leave before the cap -- found by bisection on the same noise draws, as edge_codes._snr_half picks its SNR -- with a frame
    of +-inf priors and an all-zero frame planted in the last two rows.  -> (priors, snr)"""
    if (key, B, cap) not in _BATCH:
        g = _code(key)[0]
        z = np.random.RandomState(77).standard_normal((B, g.n))
        lo, hi, snr, frac = -6.0, 12.0, None, None
        for _ in range(0 if key == CONSENSUS else 14):
            snr = 0.5 * (lo + hi)
            frac = (LQ.lqmsa_decode(g, None, _priors(g, snr, z)[:B - 2], cap)[1] < cap).mean()
            if frac < 1 / 3:
                lo = snr
            elif frac > 2 / 3:
                hi = snr
            else:
                break
        if key == CONSENSUS:
            snr = -9.0
            it = LQ.lqmsa_decode(g, None, _priors(g, snr, z)[:B - 2], cap)[1]
            assert it.max() < cap and len(np.unique(it)) >= 4, np.bincount(it)
        else:
            assert 1 / 3 <= frac <= 2 / 3, (key, snr, frac)
        pri = _priors(g, snr, z)
        pri[B - 2] = np.where(z[B - 2] < 0.5, np.inf, -np.inf)
        pri[B - 1] = 0.0
        _BATCH[(key, B, cap)] = (np.ascontiguousarray(pri), snr)
    return _BATCH[(key, B, cap)]


def _want(key, tag, y0, pri, cap, params=DEFAULT, layers=None, early=True):
    """the oracle's (xhat, iters, soft, peak), computed once per distinct case"""
    k = (key, tag, cap, params, None if layers is None else tuple(int(v) for v in layers), early, pri.dtype.str, y0 is not None)
    if k not in _WANT:
        _WANT[k] = LQ.lqmsa_decode(_code(key)[0], y0, pri, cap, *params, layers=layers, early_exit=early)
    return _WANT[k]


def _run(h, pri, y0, cap, flags=0):
    import torch

    p = torch.from_numpy(np.ascontiguousarray(pri)).cuda()
    y = None if y0 is None else torch.from_numpy(np.ascontiguousarray(y0)).cuda()
    x, it, words, soft = h.decode_device(p, y, cap, flags, bits=True, soft=True)
    torch.cuda.synchronize()
    return x.cpu().numpy(), it.cpu().numpy(), words.cpu().numpy().view(np.uint32), soft.cpu().numpy()


def _same(got, want, where):
    x, it, words, soft = got
    xr, ir, sr = want[:3]
    assert np.array_equal(it, ir), (where, np.flatnonzero(it != ir)[:8], it[:8], ir[:8])
    assert np.array_equal(x, xr), (where, np.flatnonzero((x != xr).any(axis=1))[:8])
    assert np.array_equal(words, LQ.pack_words(xr)), where
    assert soft.dtype == np.int16 and np.array_equal(soft, sr), (where, np.flatnonzero((soft != sr).any(axis=1))[:8])


ALL_KEYS = SHIPPED + [("shape",) + s for s in SHAPES] + [("dc", d) for d in DEGREES]


# ---------------------------------------------------------------------------------------------- 1. every code, both prior types
@pytest.mark.parametrize("key", ALL_KEYS, ids=str)
def test_equals_the_integer_statement(key):
    """64 frames (48 on Margulis), cap 50, default parameters, greedy layers; fp64 and fp32 priors; the +-inf frame and the all-zero frame.
    The handle reports the size rule's bytes and the wave rule's waves."""
    from ldpc_decoders_amd import layered

    g, c = _code(key)
    B = 48 if key == "margulis" else 64
    pri, _ = _batch(key, B)
    h = _handle(key)
    assert h.fixed_point() == DEFAULT
    nl, lay = h.layers()
    assert np.array_equal(lay, L.greedy_layers(g)) and nl == lay.max() + 1
    info = h.info()
    need = layered.lqmsa_lds_bytes(c.m, c.n, c.E, int(c.row_degrees().max()))
    assert info["lds_bytes_per_frame"] == need and info["waves_per_frame"] == layered.lqmsa_waves(layered.LDS_BYTES // need)
    assert info["frames_per_cu"] == min(layered.LDS_BYTES // need, 32 // info["waves_per_frame"]) and info["workgroups"] % info["frames_per_cu"] == 0
    for dt in (np.float64, np.float32):
        p = pri.astype(dt)
        want = _want(key, "parity", None, p, 50)
        assert want[1][B - 1] == 1 and (key == CONSENSUS or B / 3 - 2 <= (want[1] < 50).sum() <= 2 * B / 3 + 2)
        _same(_run(h, p, None, 50), want, (key, dt.__name__))
    _same(_run(h, p[:1], None, 50), tuple(a[:1] for a in want[:3]), (key, "B = 1"))


# ---------------------------------------------------------------------------------------------- 2. parameters, caps, flags, y0
@pytest.mark.parametrize("key", ["512_3_6_rand_ldpc_1", ("shape", 63, 96, 3), ("dc", 9)], ids=str)
def test_parameters_caps_and_flags(key):
    """Five parameter sets at cap 50; max_iter 1 and 2; LDPC_FLAG_NO_EARLY_EXIT; max_iter <= 0 runs to the frame's own exit."""
    pri = _batch(key)[0].astype(np.float32)
    h = _handle(key)
    for params in PARAMS:
        h.set_fixed_point(*params)
        assert h.fixed_point() == params
        _same(_run(h, pri, None, 50), _want(key, "params", None, pri, 50, params), (key, params))
    h.set_fixed_point(*DEFAULT)
    for cap in (1, 2):
        _same(_run(h, pri, None, cap), _want(key, "caps", None, pri, cap), (key, cap))
    want = _want(key, "free", None, pri, 7, early=False)
    assert (want[1] == 7).all()
    _same(_run(h, pri, None, 7, NO_EARLY_EXIT), want, (key, "no early exit"))
    easy = pri[np.flatnonzero(_want(key, "params", None, pri, 50)[1] < 50)[:16]]  # frames that leave on their own
    want = _want(key, "unbounded", None, easy, 0)
    assert len(easy) == 16 and want[1].max() < 50
    _same(_run(h, easy, None, 0), want, (key, "max_iter 0"))
    _same(_run(h, easy, None, -3), want, (key, "max_iter -3"))


@pytest.mark.parametrize("key,p", [("512_3_6_rand_ldpc_1", 0.055), ("1200_3_6_rand_ldpc_1", 0.08), (("shape", 65, 128, 3), 0.04), (("dc", 7), 0.03)], ids=str)
def test_bsc_with_the_received_word(key, p):
    """Every prior is +-L: every minimum ties.  A received codeword leaves at iteration 0 with x_hat = y0, iters = 0 and soft output 0;
    with LDPC_FLAG_NO_EARLY_EXIT it does not."""
    g = _code(key)[0]
    B, cap = 64, 50
    y = (np.random.RandomState(9).random_sample((B, g.n)) < p).astype(np.uint8)
    y[0] = 0
    for dt in (np.float64, np.float32):
        pri = O.bsc_priors(y.astype(np.int64), p).astype(dt)
        want = _want(key, "bsc", y, pri, cap)
        assert want[1][0] == 0 and 0 < (want[1] < cap).sum() < B and len(np.unique(want[1])) > 2
        h = _handle(key)
        got = _run(h, pri, y, cap)
        _same(got, want, (key, "bsc", dt.__name__))
        assert not got[3][0].any()
    _same(_run(h, pri, y, 3, NO_EARLY_EXIT), _want(key, "bsc free", y, pri, 3, early=False), (key, "bsc, no early exit"))
    # without y0 the same priors run at least one sweep
    want = _want(key, "bsc no y0", None, pri, cap)
    assert want[1][0] == 1
    _same(_run(h, pri, None, cap), want, (key, "bsc priors without y0"))


# ---------------------------------------------------------------------------------------------- 3. waves per frame
@pytest.mark.parametrize("nw", ["1", "2", "4", "8"])
@pytest.mark.parametrize("key", ["512_3_6_rand_ldpc_1", "1200_3_6_rand_ldpc_1", "margulis", ("dc", 33), ("shape", 129, 200, 3)], ids=str)
def test_any_number_of_waves(key, nw, monkeypatch):
    monkeypatch.setenv("LDPC_LQMSA_NW", nw)
    B = 48 if key == "margulis" else 64
    pri = _batch(key, B)[0].astype(np.float32)
    h = _handle(key)
    assert h.info()["waves_per_frame"] == int(nw) and h.info()["frames_per_cu"] <= 32 // int(nw)
    _same(_run(h, pri, None, 50), _want(key, "parity", None, pri, 50), (key, nw))
    if key == "512_3_6_rand_ldpc_1":
        params = PARAMS[2]
        h.set_fixed_point(*params)
        _same(_run(h, pri, None, 50), _want(key, "params", None, pri, 50, params), (key, nw, params))


# ---------------------------------------------------------------------------------------------- 4. batch size and frame position
@pytest.mark.parametrize("key", ["512_3_6_rand_ldpc_1", ("shape", 64, 127, 3)], ids=str)
def test_any_batch_size_and_position(key, monkeypatch):
    pri = _batch(key)[0].astype(np.float32)
    want = _want(key, "parity", None, pri, 50)
    h = _handle(key)
    ext = np.concatenate([pri, pri[:1]])
    for B in (1, 63, 64, 65):
        idx = np.arange(B) % 64
        _same(_run(h, ext[:B], None, 50), tuple(a[idx] for a in want[:3]), (key, B))
    # several times the grid: every workgroup takes several frames with mixed exit times; a frame gives the same result at any position
    monkeypatch.setenv("LDPC_LQMSA_NW", "8")  # at most 4 frames per CU: the smallest grid
    small = _handle(key)
    for hh in (small, h) if key != "512_3_6_rand_ldpc_1" else (small,):
        B = 3 * hh.info()["workgroups"] + 17
        idx = np.random.RandomState(5).randint(0, 64, size=B)
        _same(_run(hh, pri[idx], None, 50), tuple(a[idx] for a in want[:3]), (key, "B = %d" % B))


# ---------------------------------------------------------------------------------------------- 5. layerings
@pytest.mark.parametrize("key", ["12_3_4_ldpc", ("shape", 63, 96, 3)], ids=str)
def test_layerings(key):
    from ldpc_decoders_amd import _lib

    g, c = _code(key)
    pri = _batch(key)[0].astype(np.float32)
    greedy = L.greedy_layers(g)
    h = _handle(key)
    lib = _lib.load()
    for name, lay in (("reversed", greedy.max() - greedy), ("one check per layer", np.arange(g.m)), ("one per layer, backwards", 2 * (g.m - np.arange(g.m)))):
        h.set_layers(lay)
        nl, got_lay = h.layers()
        assert nl == len(np.unique(lay)) and np.array_equal(got_lay, lay)
        want = _want(key, "layers", None, pri, 50, layers=lay)
        _same(_run(h, pri, None, 50), want, (key, name))
    # refused layerings leave the previous one in force and the handle usable
    bad = [np.zeros(g.m, dtype=np.int32), np.where(np.arange(g.m) == 2, -1, np.arange(g.m)).astype(np.int32), np.arange(g.m - 1, dtype=np.int32)]
    for lay in bad:
        assert lib.ldpc_lqmsa_set_layers(h.h, lay.ctypes.data, lay.size) == E_ARG
        assert np.array_equal(h.layers()[1], 2 * (g.m - np.arange(g.m)))
    with pytest.raises(ValueError):
        h.set_layers(bad[0])
    _same(_run(h, pri, None, 50), want, (key, "after the refusals"))
    h.set_layers(None)
    assert np.array_equal(h.layers()[1], greedy)
    _same(_run(h, pri, None, 50), _want(key, "parity", None, pri, 50), (key, "greedy again"))
    # the Python class carries a layering to the handle
    from ldpc_decoders_amd import layered

    dec = layered.LQMSA(c, max_iter=50, layers=greedy.max() - greedy)
    assert np.array_equal(dec.layers, greedy.max() - greedy)
    x, it = dec.decode_batch(None, pri)
    want = _want(key, "layers", None, pri, 50, layers=greedy.max() - greedy)
    assert np.array_equal(x, want[0]) and np.array_equal(it, want[1]) and np.array_equal(dec.last_iters, want[1])


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    import torch

    from ldpc_decoders_amd import _lib, codes, layered
    from ldpc_decoders_amd._device import LqmsaHandle

    key = "12_3_4_ldpc"
    h = _handle(key)
    for bad in ((9, 2, 0.8125, 0), (1, 2, 0.8125, 0), (6, 9, 0.8125, 0), (6, 2, 0.8, 0), (6, 2, 0.0, 0), (6, 2, 0.8125, -1)):
        with pytest.raises(_lib.LdpcHipError, match="error %d.*ldpc_lqmsa_set_fixed_point" % E_ARG):
            h.set_fixed_point(*bad)
        assert h.fixed_point() == DEFAULT
    pri = torch.zeros((4, 12), dtype=torch.float32, device="cuda")
    for bad_pri in (pri[:, :11].contiguous(), pri.half(), pri.cpu(), pri.t(), pri[0]):
        with pytest.raises(ValueError):
            h.decode_device(bad_pri, None, 5)
    with pytest.raises(ValueError):
        h.decode_device(pri, torch.zeros((3, 12), dtype=torch.uint8, device="cuda"), 5)
    with pytest.raises(_lib.LdpcHipError, match="error %d.*LDPC_FLAG_NO_EARLY_EXIT" % E_UNSUPPORTED):
        h.decode_device(pri, None, 5, flags=2)
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        h.simulate("bec", 0.1, 0, SEED, STREAM, 0, 64, 5, cnt)
    odd = LqmsaHandle(codes.rand_reg_ldpc(40, 3, 5, np.random.RandomState(3)))  # checks of degree 5: the all-ones word is no codeword
    with pytest.raises(_lib.LdpcHipError, match="odd degree"):
        odd.simulate("bsc", 0.1, 1, SEED, STREAM, 0, 64, 5, cnt)
    with pytest.raises(_lib.LdpcHipError, match="codeword must be 0 or 1"):
        odd.simulate("bsc", 0.1, 2, SEED, STREAM, 0, 64, 5, cnt)
    # a check of degree 1, past the Python checks
    one = codes.Code.from_edges(2, 3, np.array([0, 0, 1], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32))
    with pytest.raises(_lib.LdpcHipError, match="error %d.*degree 1" % E_UNSUPPORTED):
        LqmsaHandle(one)
    # weight-6 rows on either side of the LDS rule: 2 n + 8 m + 16 = 163840 is accepted and decodes, one check more is refused
    n = 4096
    m_ok = (layered.LDS_BYTES - 16 - 2 * n) // 8
    with pytest.raises(_lib.LdpcHipError, match="error %d.*LDPC_ALG_LMSA" % E_UNSUPPORTED) as e:
        LqmsaHandle(EC.limit_code(m_ok + 1, n))
    assert "bytes of LDS" in str(e.value)
    c = EC.limit_code(m_ok, n)
    assert layered.lqmsa_lds_bytes(c.m, c.n, c.E, 6) == layered.LDS_BYTES and c.col_degrees().max() <= layered.MAX_DV
    big = LqmsaHandle(c)
    assert big.info() == dict(lds_bytes_per_frame=layered.LDS_BYTES, waves_per_frame=8, frames_per_cu=1, workgroups=big.info()["workgroups"])
    g = O.Edges(c.m, c.n, c.edge_chk, c.edge_var)
    z = np.random.RandomState(8).standard_normal((8, n))
    p32 = _priors(g, -3.0, z).astype(np.float32)
    want = LQ.lqmsa_decode(g, None, p32, 4)
    _same(_run(big, p32, None, 4), want, "the largest accepted frame")


# ---------------------------------------------------------------------------------------------- 7. simulate
@pytest.mark.parametrize("channel,param", [("biawgn", 2.5), ("bsc", 0.05)])
def test_simulate_equals_channel_decode_count(channel, param):
    """ldpc_lqmsa_simulate's counters are the oracle's on the priors ldpc_channel writes for the same (seed, stream, frame0): 256 frames
    from frame 1000 on, two calls accumulate."""
    import torch

    from ldpc_decoders_amd import _lib

    key, B, cap, frame0, bins = "512_3_6_rand_ldpc_1", 256, 20, 1000, 21
    g, c = _code(key)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    pri = torch.empty((B, g.n), dtype=torch.float32, device="cuda")
    y = torch.empty((B, g.n), dtype=torch.uint8, device="cuda") if channel == "bsc" else None
    _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE["f32"], float(param), 0, SEED, STREAM, frame0, B, g.n, pri.data_ptr(),
                                None if y is None else y.data_ptr(), st))
    x, it, _, _ = LQ.lqmsa_decode(g, None if y is None else y.cpu().numpy(), pri.cpu().numpy(), cap)
    wrong = x.any(axis=1)
    assert 0 < wrong.sum() < B
    h = _handle(key)
    cnt = torch.zeros(_lib.CNT_HIST0 + bins, dtype=torch.int64, device="cuda")
    h.simulate(channel, param, 0, SEED, STREAM, frame0, B, cap, cnt, hist_bins=bins)
    got = cnt.cpu().numpy()
    assert got[_lib.CNT_TOT] == B and got[_lib.CNT_WEC] == wrong.sum() and got[_lib.CNT_BEC] == x.sum() and got[_lib.CNT_ITER_SUM] == it.sum()
    assert np.array_equal(got[_lib.CNT_HIST0:], np.bincount(it, minlength=bins))
    h.simulate(channel, param, 0, SEED, STREAM, frame0, 100, cap, cnt, hist_bins=bins)  # accumulates; the first 100 frames again
    got2 = cnt.cpu().numpy()
    assert got2[_lib.CNT_TOT] == B + 100 and got2[_lib.CNT_WEC] == wrong.sum() + wrong[:100].sum()
    # the all-ones word: the channel negates, the counters count against it
    cnt.zero_()
    h.simulate(channel, param, 1, SEED, STREAM, frame0, B, cap, cnt)
    got1 = cnt.cpu().numpy()
    assert got1[_lib.CNT_TOT] == B and 0 < got1[_lib.CNT_WEC] < B


def test_simulate_random_codewords():
    """codeword = -1 through the handle: encoder words, ldpc_channel_sent, decode, ldpc_count_errors_words -- the same steps on the oracle."""
    import torch

    from ldpc_decoders_amd import _lib

    key, B, cap, frame0 = "512_3_6_rand_ldpc_1", 128, 20, 64
    g, c = _code(key)
    h = _handle(key)
    cnt = torch.zeros(_lib.CNT_HIST0, dtype=torch.int64, device="cuda")
    h.simulate("biawgn", 2.5, -1, SEED, STREAM, frame0, B, cap, cnt)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    sent = c.encoder().handle(h.device).encode_random(SEED, STREAM, frame0, B)
    pri = torch.empty((B, g.n), dtype=torch.float32, device="cuda")
    _lib.check(lib.ldpc_channel_sent(_lib.CHANNEL["biawgn"], _lib.DTYPE["f32"], 2.5, sent.data_ptr(), SEED, STREAM, frame0, B, g.n, pri.data_ptr(), None, st))
    x, it, _, _ = LQ.lqmsa_decode(g, None, pri.cpu().numpy(), cap)
    s = sent.cpu().numpy()
    assert s.any() and 0 < (x != s).any(axis=1).sum() < B
    got = cnt.cpu().numpy()
    assert (got[_lib.CNT_TOT], got[_lib.CNT_WEC], got[_lib.CNT_BEC], got[_lib.CNT_ITER_SUM]) == (B, (x != s).any(axis=1).sum(), (x != s).sum(), it.sum())


# ---------------------------------------------------------------------------------------------- 8. Python classes and the command line
def test_channel_classes_decode_what_the_handle_decodes():
    from ldpc_decoders_amd import biawgn, bsc

    key = "512_3_6_rand_ldpc_1"
    g, c = _code(key)
    p = 0.055
    y = (np.random.RandomState(9).random_sample((64, g.n)) < p).astype(np.uint8)
    y[0] = 0
    want = _want(key, "bsc", y, O.bsc_priors(y.astype(np.int64), p).astype(np.float32), 50)
    dec = bsc.LQMSA(p, c, max_iter=50)
    yi = y.astype(np.int64)  # (int64 words, as the reference's channel hands them over)
    x, it = dec.decode_batch(yi)
    assert np.array_equal(x, want[0]) and np.array_equal(it, want[1])
    assert np.array_equal(np.asarray(dec.decode(yi[5])), want[0][5]) and int(dec.dec.last_iters[0]) == want[1][5]
    assert not np.asarray(dec.decode(yi[0])).any() and int(dec.dec.last_iters[0]) == 0
    import torch

    xd, itd = dec.decode_batch(torch.from_numpy(y).cuda())
    assert np.array_equal(xd.cpu().numpy(), want[0]) and np.array_equal(itd.cpu().numpy(), want[1])
    # biawgn: observations in, the LLR -2 y / sigma^2 quantised in fp32 (and in fp64 with precision="f64")
    snr = _batch(key)[1]
    obs = -1 + np.sqrt(O.biawgn_noise_var(snr)) * np.random.RandomState(77).standard_normal((64, g.n))
    for prec, dt in (("f32", np.float32), ("f64", np.float64)):
        soft = biawgn.LQMSA(snr, c, max_iter=50, msa_bits=5, msa_frac_bits=1, msa_scale=0.75, msa_offset=1, precision=prec)
        pri = soft.priors(obs).astype(dt)
        want = LQ.lqmsa_decode(g, None, pri, 50, 5, 1, 0.75, 1)
        xs, its = soft.decode_batch(obs)
        assert np.array_equal(xs, want[0]) and np.array_equal(its, want[1])
    assert soft.dec.handle.fixed_point() == (5, 1, 0.75, 1)


def test_cli(tmp_path, monkeypatch):
    from ldpc_decoders_amd import codes, main

    monkeypatch.setenv(codes.file_codes_dir_string, CODES_DIR)
    argv = "biawgn 512_3_6_rand_ldpc_1 LQMSA --params 2.5 --max-iter 20 --batch 4096 --max-frames 4096".split()
    main.main(argv + ["--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-512_3_6_rand_ldpc_1-LQMSA-0-100-20-6-2-0.8125-0.0.json")) as fp:
        res = json.load(fp)
    assert res["decoder"] == "LQMSA" and res["max_iter"] == 20 and (res["msa_bits"], res["msa_frac_bits"], res["msa_scale"], res["msa_offset"]) == (6, 2, 0.8125, 0.0)
    tot, wec, bec = res["tot"]["2.5"], res["wec"]["2.5"], res["bec"]["2.5"]
    assert tot == 4096 and 4 <= wec < tot // 4 and wec <= bec <= wec * 512 and res["wer"]["2.5"] == pytest.approx(wec / tot)
    # random codewords and the fused backend through the same driver
    main.main(argv + ["--codeword", "-1", "--backend", "fused", "--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-512_3_6_rand_ldpc_1-LQMSA--1-100-20-6-2-0.8125-0.0.json")) as fp:
        res = json.load(fp)
    assert res["tot"]["2.5"] == 4096 and 4 <= res["wec"]["2.5"] < 1024

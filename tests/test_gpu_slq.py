"""Streaming layered fixed-point min-sum on the GPU (csrc/ldpc_slq.hip, ldpc_slq_*): decisions -- as bytes and as packed words -- iteration
counts and int16 soft outputs equal to the integer statement of lqmsa_oracle.py with ``==``: every degree class of the layer pass and its
successor, the shape edges, codes LQMSA refuses (n > 2^16; the LDS bound), fp32 and fp64 priors, the iteration-0 rule, caps and flags, any
batch size, a thinning batch under every repack setting, custom layerings, LqmsaHandle and QcHandle at the same layering, the refusals, the
simulate composition across a chunk boundary, the profile slots and the command line.

Codes, batches and oracle results are those of test_gpu_lqmsa.py where the two files decode the same case (its caches are shared)."""
import json
import os

import numpy as np
import pytest

import bp_oracle as O
import lmsa_oracle as L
import lqmsa_oracle as LQ
import test_gpu_lqmsa as TL
import test_gpu_qc as TQ
from helpers import CODES_DIR
from test_slq_cpu import padded_code

pytestmark = pytest.mark.gpu
SEED, STREAM = TL.SEED, TL.STREAM
E_ARG, E_UNSUPPORTED = -1, -4  # include/ldpc_hip.h
NO_EARLY_EXIT = 1
DEFAULT, PARAMS = TL.DEFAULT, TL.PARAMS  # the five parameter sets of DESIGN.md section 21
SHIPPED = ["12_3_4_ldpc", "512_3_6_rand_ldpc_1", "1200_rho_x5_rand_ldpc_1"]
# (3, dc)-regular codes of 66 checks: every degree class of the layer pass -- 4, 6 (regular and not), 8, 16, 32, 64, the two-pass kernel
# above 64 -- and its successor
DEGREES = [2, 3, 6, 7, 8, 9, 16, 17, 33, 64, 65]
ALL_KEYS = SHIPPED + [("shape",) + s for s in TL.SHAPES] + [("dc", d) for d in DEGREES]
_code, _want, _same, _priors = TL._code, TL._want, TL._same, TL._priors
_BIG = {}


def _shape(key):
    """(frames, cap) of a code's batch: the rows of degree 64 and 65 cost the oracle dc^2 per check, so they get half the frames and cap 20"""
    return (32, 20) if key in (("dc", 64), ("dc", 65)) else (64, 50)


def _batch(key):
    return TL._batch(key, *_shape(key))


def _handle(key_or_code, params=None, layers=None):
    from ldpc_decoders_amd._device import SlqHandle

    h = SlqHandle(key_or_code if hasattr(key_or_code, "edge_var") else _code(key_or_code)[1])
    if params is not None:
        h.set_fixed_point(*params)
    if layers is not None:
        h.set_layers(layers)
    return h


def _run(h, pri, y0, cap, flags=0, soft=True):
    """-> (xhat, iters, words, soft); without ``soft`` the decode may repack and does not freeze: the oracle's soft output is not compared"""
    import torch

    p = torch.from_numpy(np.ascontiguousarray(pri)).cuda()
    y = None if y0 is None else torch.from_numpy(np.ascontiguousarray(y0)).cuda()
    out = h.decode_device(p, y, cap, flags, bits=True, soft=soft)
    torch.cuda.synchronize()
    x, it, words = (t.cpu().numpy() for t in out[:3])
    return x, it, words.view(np.uint32), out[3].cpu().numpy() if soft else None


def _same_hard(got, want, where):
    x, it, words, _ = got
    assert np.array_equal(it, want[1]), (where, np.flatnonzero(it != want[1])[:8], it[:8], want[1][:8])
    assert np.array_equal(x, want[0]), (where, np.flatnonzero((x != want[0]).any(axis=1))[:8])
    assert np.array_equal(words, LQ.pack_words(want[0])), where


def _both(h, pri, y0, cap, want, where, flags=0):
    """the soft-output decode (frozen lanes, never repacked) and the plain one (no freeze, repack allowed)"""
    _same(_run(h, pri, y0, cap, flags), want, (where, "soft"))
    _same_hard(_run(h, pri, y0, cap, flags, soft=False), want, (where, "hard"))


# ---------------------------------------------------------------------------------------------- 1. every code, both prior types
@pytest.mark.parametrize("key", ALL_KEYS, ids=str)
def test_equals_the_integer_statement(key):
    """Default parameters, greedy layers; fp64 and fp32 priors; the +-inf frame and the all-zero frame; one frame alone."""
    g, c = _code(key)
    B, cap = _shape(key)
    pri, _ = _batch(key)
    h = _handle(key)
    assert h.fixed_point() == DEFAULT
    nl, lay = h.layers()
    assert np.array_equal(lay, L.greedy_layers(g)) and nl == lay.max() + 1
    info = h.info()
    assert info["state_bytes_per_frame"] == 2 * c.n + c.E and info["layers"] == nl and info["launches_per_sweep"] == nl + 1 and info["tiles_per_chunk"] >= 1
    for dt in (np.float64, np.float32):
        p = pri.astype(dt)
        want = _want(key, "parity", None, p, cap)
        assert want[1][B - 1] == 1 and (key == TL.CONSENSUS or B / 3 - 2 <= (want[1] < cap).sum() <= 2 * B / 3 + 2)
        _both(h, p, None, cap, want, (key, dt.__name__))
    _same(_run(h, p[:1], None, cap), tuple(a[:1] for a in want[:3]), (key, "B = 1"))
    assert h.last_stats()[2] == 1


# ---------------------------------------------------------------------------------------------- 2. parameters, caps, flags, y0
@pytest.mark.parametrize("key", ["512_3_6_rand_ldpc_1", ("shape", 63, 96, 3), ("dc", 9)], ids=str)
def test_parameters_caps_and_flags(key):
    """Five parameter sets at cap 50; max_iter 1, 2 and 50; LDPC_FLAG_NO_EARLY_EXIT; max_iter <= 0 runs to the frame's own exit."""
    pri = _batch(key)[0].astype(np.float32)
    h = _handle(key)
    for params in PARAMS:
        h.set_fixed_point(*params)
        assert h.fixed_point() == params
        _both(h, pri, None, 50, _want(key, "params", None, pri, 50, params), (key, params))
    h.set_fixed_point(*DEFAULT)
    for cap in (1, 2):
        _both(h, pri, None, cap, _want(key, "caps", None, pri, cap), (key, cap))
    want = _want(key, "free", None, pri, 7, early=False)
    assert (want[1] == 7).all()
    _both(h, pri, None, 7, want, (key, "no early exit"), NO_EARLY_EXIT)
    easy = pri[np.flatnonzero(_want(key, "params", None, pri, 50)[1] < 50)[:16]]  # frames that leave on their own
    want = _want(key, "unbounded", None, easy, 0)
    assert len(easy) == 16 and want[1].max() < 50
    _both(h, easy, None, 0, want, (key, "max_iter 0"))
    _both(h, easy, None, -3, want, (key, "max_iter -3"))


@pytest.mark.parametrize("key,p", [("512_3_6_rand_ldpc_1", 0.055), (("shape", 65, 128, 3), 0.04), (("dc", 7), 0.03)], ids=str)
def test_bsc_with_the_received_word(key, p):
    """Every prior is +-L: every minimum ties.  A received codeword leaves at iteration 0 with x_hat = y0, iters = 0 and soft output 0;
    with LDPC_FLAG_NO_EARLY_EXIT it does not."""
    g = _code(key)[0]
    B, cap = 64, 50
    y = (np.random.RandomState(9).random_sample((B, g.n)) < p).astype(np.uint8)
    y[0] = 0
    h = _handle(key)
    for dt in (np.float64, np.float32):
        pri = O.bsc_priors(y.astype(np.int64), p).astype(dt)
        want = _want(key, "bsc", y, pri, cap)
        assert want[1][0] == 0 and 0 < (want[1] < cap).sum() < B and len(np.unique(want[1])) > 2
        got = _run(h, pri, y, cap)
        _same(got, want, (key, "bsc", dt.__name__))
        assert not got[3][0].any()
        _same_hard(_run(h, pri, y, cap, soft=False), want, (key, "bsc, hard", dt.__name__))
    _both(h, pri, y, 3, _want(key, "bsc free", y, pri, 3, early=False), (key, "bsc, no early exit"), NO_EARLY_EXIT)
    # a received codeword alone: nothing is ever swept
    got = _run(h, pri[:1], y[:1], cap)
    assert got[1].tolist() == [0] and not got[0].any() and not got[3].any()
    # without y0 the same priors run at least one sweep
    want = _want(key, "bsc no y0", None, pri, cap)
    assert want[1][0] == 1
    _both(h, pri, None, cap, want, (key, "bsc priors without y0"))


# ---------------------------------------------------------------------------------------------- 3. batch sizes, thinning batches, repack
@pytest.mark.parametrize("key", ["512_3_6_rand_ldpc_1", ("shape", 64, 127, 3)], ids=str)
def test_any_batch_size_and_position(key):
    pri = _batch(key)[0].astype(np.float32)
    want = _want(key, "parity", None, pri, 50)
    h = _handle(key)
    ext = np.concatenate([pri, pri, pri[:1]])
    for B in (1, 63, 64, 65, 129):
        idx = np.arange(B) % 64
        _both(h, ext[:B], None, 50, tuple(a[idx] for a in want[:3]), (key, B))


def _thinning(key):
    """64 * 9 + 17 frames drawn from the code's batch: three tiles of frames that all leave, three that keep exactly one frame to the cap,
    the rest a shuffled mix -> (row of the batch per frame)"""
    want = _want(key, "parity", None, _batch(key)[0].astype(np.float32), 50)
    easy, hard = np.flatnonzero(want[1] < 50), np.flatnonzero(want[1] == 50)
    rng = np.random.RandomState(31)
    idx = rng.randint(0, 64, size=64 * 9 + 17)
    idx[:192] = rng.choice(easy, 192)
    idx[192:384] = rng.choice(easy, 192)
    idx[[200, 300, 383]] = rng.choice(hard, 3)  # one straggler in each of tiles 3, 4, 5
    return idx, want


@pytest.mark.parametrize("key", ["512_3_6_rand_ldpc_1", ("shape", 129, 200, 3)], ids=str)
def test_a_thinning_batch_is_the_same_under_every_repack_setting(key, monkeypatch):
    """LDPC_STREAM_REPACK=0, the eager LDPC_STREAM_REPACK_FILL setting and the default (both read at every decode): identical outputs, equal
    to the oracle's; the eager setting does repack, the switch does turn it off; a soft-output decode never repacks and freezes."""
    pri = _batch(key)[0].astype(np.float32)
    idx, want = _thinning(key)
    want = tuple(a[idx] for a in want[:3])
    h = _handle(key)
    outs = {}
    for name, env in (("off", {"LDPC_STREAM_REPACK": "0"}), ("eager", {"LDPC_STREAM_REPACK_FILL": "0.95"}), ("default", {})):
        for k in ("LDPC_STREAM_REPACK", "LDPC_STREAM_REPACK_FILL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        outs[name] = _run(h, pri[idx], None, 50, soft=False)
        _same_hard(outs[name], want, (key, name))
        sweeps, repacks, chunks = h.last_stats()
        assert sweeps == 50 and chunks == 1 and (repacks == 0 if name == "off" else repacks >= (1 if name == "eager" else 0)), (name, repacks)
        if name == "eager":  # a second kind of call on the repacked path: bytes only / words only
            import torch

            p = torch.from_numpy(pri[idx]).cuda()
            x, it = h.decode_device(p, None, 50)
            assert np.array_equal(x.cpu().numpy(), want[0]) and np.array_equal(it.cpu().numpy(), want[1]) and h.last_stats()[1] >= 1
    for name in ("eager", "default"):
        assert all(np.array_equal(a, b) for a, b in zip(outs["off"][:3], outs[name][:3])), name
    monkeypatch.setenv("LDPC_STREAM_REPACK_FILL", "0.95")
    _same(_run(h, pri[idx], None, 50), want, (key, "soft output: frozen at each frame's last sweep"))
    assert h.last_stats()[1] == 0


# ---------------------------------------------------------------------------------------------- 4. layerings
@pytest.mark.parametrize("key", ["12_3_4_ldpc", ("shape", 63, 96, 3)], ids=str)
def test_layerings(key):
    from ldpc_decoders_amd import _lib, layered
    from ldpc_decoders_amd._device import LqmsaHandle

    g, c = _code(key)
    pri = _batch(key)[0].astype(np.float32)
    greedy = L.greedy_layers(g)
    h, lds = _handle(key), LqmsaHandle(c)
    lib = _lib.load()
    for name, lay in (("reversed", greedy.max() - greedy), ("one check per layer", np.arange(g.m)), ("one per layer, backwards", 2 * (g.m - np.arange(g.m)))):
        h.set_layers(lay)
        nl, got_lay = h.layers()
        assert nl == len(np.unique(lay)) and np.array_equal(got_lay, lay) and h.info()["launches_per_sweep"] == nl + 1
        want = _want(key, "layers", None, pri, 50, layers=lay)
        got = _run(h, pri, None, 50)
        _same(got, want, (key, name))
        _same_hard(_run(h, pri, None, 50, soft=False), want, (key, name))
        lds.set_layers(lay)  # the LDS-resident kernel at the same layering: identical tensors
        assert all(np.array_equal(a, b) for a, b in zip(got, TL._run(lds, pri, None, 50))), (key, name)
    # refused layerings leave the previous one in force and the handle usable
    bad = [np.zeros(g.m, dtype=np.int32), np.where(np.arange(g.m) == 2, -1, np.arange(g.m)).astype(np.int32), np.arange(g.m - 1, dtype=np.int32)]
    for lay in bad:
        assert lib.ldpc_slq_set_layers(h.h, lay.ctypes.data, lay.size) == E_ARG
        assert np.array_equal(h.layers()[1], 2 * (g.m - np.arange(g.m)))
    with pytest.raises(ValueError):
        h.set_layers(bad[0])
    _same(_run(h, pri, None, 50), want, (key, "after the refusals"))
    h.set_layers(None)
    assert np.array_equal(h.layers()[1], greedy)
    _same(_run(h, pri, None, 50), _want(key, "parity", None, pri, 50), (key, "greedy again"))
    # the Python class carries a layering to the handle
    dec = layered.SLQMSA(c, max_iter=50, layers=greedy.max() - greedy)
    assert np.array_equal(dec.layers, greedy.max() - greedy)
    x, it = dec.decode_batch(None, pri)
    want = _want(key, "layers", None, pri, 50, layers=greedy.max() - greedy)
    assert np.array_equal(x, want[0]) and np.array_equal(it, want[1]) and np.array_equal(dec.last_iters, want[1])
    assert np.array_equal(np.asarray(dec.decode(None, pri[5])), want[0][5]) and int(dec.last_iters[0]) == want[1][5]


def test_the_quasi_cyclic_kernel_returns_the_same_tensors():
    """QcHandle on a quasi-cyclic code against SlqHandle at layers = check // Z; irregular block rows (degrees 2, 3, 7, 8, 8)."""
    from ldpc_decoders_amd import qc
    from ldpc_decoders_amd._device import QcHandle

    for mask, Z, seed in ((np.ones((3, 6), dtype=bool), 65, 165), (TQ.IRREGULAR, 65, 11)):
        c = qc.rand_qc_ldpc(mask, Z, np.random.RandomState(seed))
        g = O.Edges(c.m, c.n, c.edge_chk, c.edge_var)
        pri = _priors(g, 1.5 if mask.all() else 3.0, np.random.RandomState(77).standard_normal((65, g.n))).astype(np.float32)
        a = TL._run(QcHandle(c, Z), pri, None, 30)
        b = _run(_handle(c, layers=qc.layers_of(Z, np.arange(mask.shape[0]))), pri, None, 30)
        assert 0 < (a[1] < 30).sum() and len(np.unique(a[1])) > 2, np.bincount(a[1])
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), Z


# ---------------------------------------------------------------------------------------------- 5. codes LQMSA refuses
def _big(name):
    """-> (code, edges, fp32 priors [B, n], cap, layers or None), the SNR bisected on the oracle as in test_gpu_lqmsa._batch"""
    from ldpc_decoders_amd import codes, qc

    if name not in _BIG:
        if name == "padded":  # the degree-0 variables take part in nothing: the bisection runs on the 1200 variables of the code itself
            c, B, cap, lay = padded_code(), 64, 50, None
            small = codes.get_code("1200_3_6_rand_ldpc_1")
            gs = O.Edges(small.m, small.n, small.edge_chk, small.edge_var)
            z = np.random.RandomState(77).standard_normal((B, c.n))
            lo, hi = -6.0, 12.0
            for _ in range(14):
                snr = 0.5 * (lo + hi)
                frac = (LQ.lqmsa_decode(gs, None, _priors(gs, snr, z[:, :small.n]), cap)[1] < cap).mean()
                if frac < 1 / 3:
                    lo = snr
                elif frac > 2 / 3:
                    hi = snr
                else:
                    break
            assert 1 / 3 <= frac <= 2 / 3, (snr, frac)
        else:  # dense 3 x 6 at Z = 4551, one lifting size above the LDS bound (test_gpu_qc.test_create_refusals): n = 27 306
            # 1.5 dB lies in the bisection's bracket for these draws (on the oracle, 6 s a step: 1.45 dB leaves 22 % of the frames before the
            # cap, 1.5 dB 48 %, 1.55 dB 76 %); the test asserts the fraction
            c, B, cap, snr = qc.rand_qc_ldpc(np.ones((3, 6), dtype=bool), 4551, np.random.RandomState(21)), 65, 12, 1.5
            lay = qc.layers_of(4551, np.arange(3))
            z = np.random.RandomState(77).standard_normal((B, c.n))
        g = O.Edges(c.m, c.n, c.edge_chk, c.edge_var)
        pri = _priors(g, snr, z)
        pri[B - 2] = np.where(z[B - 2] < 0.5, np.inf, -np.inf)
        pri[B - 1] = 0.0
        _BIG[name] = (c, g, np.ascontiguousarray(pri.astype(np.float32)), cap, lay)
    return _BIG[name]


@pytest.mark.parametrize("name", ["padded", "qc4551"])
def test_codes_beyond_the_lds(name):
    """n = 82 944 (indices beyond 2^16, 2 n bytes above the LDS bound) and the quasi-cyclic code one lifting size above the LDS bound with
    65 frames: ldpc_lqmsa_create refuses, SLQMSA decodes what the oracle decodes."""
    from ldpc_decoders_amd import _lib
    from ldpc_decoders_amd._device import LqmsaHandle

    c, g, pri, cap, lay = _big(name)
    with pytest.raises(_lib.LdpcHipError, match="error %d.*LDPC_ALG_LMSA" % E_UNSUPPORTED):
        LqmsaHandle(c)
    h = _handle(c, layers=lay)
    assert h.info()["state_bytes_per_frame"] == 2 * c.n + c.E
    want = LQ.lqmsa_decode(g, None, pri, cap, layers=lay)
    B = len(pri)
    assert B / 3 - 2 <= (want[1] < cap).sum() <= 2 * B / 3 + 2, np.bincount(want[1])
    _both(h, pri, None, cap, want, name)
    if name == "padded":  # a degree-0 variable keeps its level; fp64 priors; the last variable of the last frame
        assert np.array_equal(want[2][:B - 1, 1200:], np.clip(np.rint(pri[:B - 1, 1200:] * 4), -31, 31).astype(np.int16))
        p64 = pri.astype(np.float64)
        _both(h, p64, None, cap, LQ.lqmsa_decode(g, None, p64, cap), (name, "fp64"))


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    import torch

    from ldpc_decoders_amd import _lib, codes
    from ldpc_decoders_amd._device import SlqHandle

    h = _handle("12_3_4_ldpc")
    for bad in ((9, 2, 0.8125, 0), (1, 2, 0.8125, 0), (6, 9, 0.8125, 0), (6, 2, 0.8, 0), (6, 2, 0.0, 0), (6, 2, 0.8125, -1)):
        with pytest.raises(_lib.LdpcHipError, match="error %d.*ldpc_slq_set_fixed_point" % E_ARG):
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
    x, it = h.decode_device(pri[:0], None, 5)
    assert tuple(x.shape) == (0, 12) and tuple(it.shape) == (0,)
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        h.simulate("bec", 0.1, 0, SEED, STREAM, 0, 64, 5, cnt)
    odd = SlqHandle(codes.rand_reg_ldpc(40, 3, 5, np.random.RandomState(3)))  # checks of degree 5: the all-ones word is no codeword
    with pytest.raises(_lib.LdpcHipError, match="odd degree"):
        odd.simulate("bsc", 0.1, 1, SEED, STREAM, 0, 64, 5, cnt)
    with pytest.raises(_lib.LdpcHipError, match="codeword must be 0 or 1"):
        odd.simulate("bsc", 0.1, 2, SEED, STREAM, 0, 64, 5, cnt)
    # the two refusals of create, past the Python checks: a check of degree 1, a variable of degree 256 (255 is taken)
    one = codes.Code.from_edges(2, 3, np.array([0, 0, 1], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32))
    with pytest.raises(_lib.LdpcHipError, match="error %d.*degree 1" % E_UNSUPPORTED):
        SlqHandle(one)
    chk = np.repeat(np.arange(256), 2).astype(np.int32)
    var = np.stack([np.zeros(256, dtype=np.int32), 1 + np.arange(256, dtype=np.int32)], axis=1).reshape(-1)
    with pytest.raises(_lib.LdpcHipError, match="error %d.*degree 256" % E_UNSUPPORTED):
        SlqHandle(codes.Code.from_edges(256, 257, chk, var))
    star = codes.Code.from_edges(255, 256, chk[:510], var[:510])  # 255 checks {0, 1 + c}: 255 layers, the marginal of variable 0 reaches V (1 + 255)
    g = O.Edges(star.m, star.n, star.edge_chk, star.edge_var)
    p = np.full((3, 256), 200.0, dtype=np.float32)
    p[1, 0], p[2] = -200.0, -200.0
    want = LQ.lqmsa_decode(g, None, p, 3, 8, 0, 1.0, 0, early_exit=False)
    assert np.abs(want[2]).max() == 127 * 256
    _same(_run(_handle(star, params=(8, 0, 1.0, 0)), p, None, 3, NO_EARLY_EXIT), want, "a variable of degree 255")


# ---------------------------------------------------------------------------------------------- 7. simulate, chunks, profile
@pytest.mark.parametrize("channel,param", [("biawgn", 2.5), ("bsc", 0.05)])
def test_simulate_equals_channel_decode_count(channel, param, monkeypatch):
    """ldpc_slq_simulate's counters are the oracle's on the priors ldpc_channel writes for the same (seed, stream, frame0): 256 frames from
    frame 1000 on, two calls accumulate; the same under a workspace bound of 1 MiB, which cuts the 256 frames into chunks of 3 tiles."""
    import torch

    from ldpc_decoders_amd import _lib

    key, B, cap, frame0, bins = "512_3_6_rand_ldpc_1", 256, 20, 1000, 21
    g, c = _code(key)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    pri = torch.empty((B, g.n), dtype=torch.float32, device="cuda")
    y = torch.empty((B, g.n), dtype=torch.uint8, device="cuda") if channel == "bsc" else None
    _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE["f32"], float(param), 0, SEED, STREAM, frame0, B, g.n, pri.data_ptr(),
                                None if y is None else y.data_ptr(), st))
    y_host = None if y is None else y.cpu().numpy()
    want = LQ.lqmsa_decode(g, y_host, pri.cpu().numpy(), cap)
    x, it = want[:2]
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
    # a chunk boundary: 1 MiB holds twice the state of 3 tiles of this code (2 * 3 * 64 * 2560 B + planes)
    monkeypatch.setenv("LDPC_SLQ_WORKSPACE_MB", "1")
    assert h.info()["tiles_per_chunk"] == 3
    _both(h, pri.cpu().numpy(), y_host, cap, want, (channel, "two chunks"))
    assert h.last_stats()[2] == 2  # 4 tiles in chunks of equal size: 2 + 2
    _both(h, pri.cpu().numpy()[:B - 27], None if y_host is None else y_host[:B - 27], cap, tuple(a[:B - 27] for a in want[:3]), (channel, "chunks, ragged"))
    cnt.zero_()
    h.simulate(channel, param, 0, SEED, STREAM, frame0, B, cap, cnt, hist_bins=bins)
    assert np.array_equal(cnt.cpu().numpy(), got)


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


def test_profile_slots():
    """[0] the layer passes and [1] the decision pass once per sweep enqueued, [2] once per decode; the outputs do not change."""
    key = "512_3_6_rand_ldpc_1"
    pri = _batch(key)[0].astype(np.float32)
    h = _handle(key)
    h.profile(True)
    _same(_run(h, pri, None, 50), _want(key, "parity", None, pri, 50), (key, "profiled"))
    prof = h.read_profile()
    sweeps = h.last_stats()[0]
    assert sweeps == 50 and prof["layer_passes"][1] == prof["decision_pass"][1] == sweeps and prof["decode_total"][1] == 1
    assert 0 < prof["layer_passes"][0] + prof["decision_pass"][0] <= prof["decode_total"][0]
    assert h.read_profile()["decode_total"] == (0.0, 0)
    h.profile(False)
    _run(h, pri, None, 5)
    assert h.read_profile()["decode_total"] == (0.0, 0)


# ---------------------------------------------------------------------------------------------- 8. the command line
def test_cli(tmp_path, monkeypatch):
    from ldpc_decoders_amd import codes, main

    monkeypatch.setenv(codes.file_codes_dir_string, CODES_DIR)
    argv = "biawgn 512_3_6_rand_ldpc_1 SLQMSA --params 2.5 --max-iter 20 --batch 4096 --max-frames 4096".split()
    main.main(argv + ["--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-512_3_6_rand_ldpc_1-SLQMSA-0-100-20-6-2-0.8125-0.0.json")) as fp:
        res = json.load(fp)
    assert res["decoder"] == "SLQMSA" and res["max_iter"] == 20 and (res["msa_bits"], res["msa_frac_bits"], res["msa_scale"], res["msa_offset"]) == (6, 2, 0.8125, 0.0)
    tot, wec, bec = res["tot"]["2.5"], res["wec"]["2.5"], res["bec"]["2.5"]
    assert tot == 4096 and 4 <= wec < tot // 4 and wec <= bec <= wec * 512 and res["wer"]["2.5"] == pytest.approx(wec / tot)
    # the same frames through LQMSA: one contract, the same counters
    main.main([a if a != "SLQMSA" else "LQMSA" for a in argv] + ["--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-512_3_6_rand_ldpc_1-LQMSA-0-100-20-6-2-0.8125-0.0.json")) as fp:
        lds = json.load(fp)
    assert (lds["tot"], lds["wec"], lds["bec"]) == (res["tot"], res["wec"], res["bec"])
    # random codewords and the streaming backend through the same driver
    main.main(argv + ["--codeword", "-1", "--backend", "stream", "--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-512_3_6_rand_ldpc_1-SLQMSA--1-100-20-6-2-0.8125-0.0.json")) as fp:
        res = json.load(fp)
    assert res["tot"]["2.5"] == 4096 and 4 <= res["wec"]["2.5"] < 1024

"""Quasi-cyclic layered fixed-point min-sum on the GPU (csrc/ldpc_qc.hip, ldpc_qc_*): decisions -- as bytes and as packed words -- iteration
counts and soft outputs equal to the integer statement of lqmsa_oracle.py on the expanded H with the block rows as layers, with ``==``:
every lifting size around the pass edges, irregular block rows, the loop form, fp32 and fp64 priors, the iteration-0 rule, every wave
count, any batch size and frame position, any order of the block rows, the refusals, the simulate composition and the command line.

One shape differs from the list this file was written to: an irregular mask with block-row degrees 2, 3, 7, 8, 8, a block column of
degree 1 and an all-zero block column cannot have 9 columns (two rows of degree 8 on the 8 columns that are left make every one of them
degree >= 2), so the mask is 5 x 10; every property asked of it is kept."""
import json
import os

import numpy as np
import pytest

import bp_oracle as O
import lqmsa_oracle as LQ

pytestmark = pytest.mark.gpu
SEED, STREAM = 0x1A7E5EED, 5
E_ARG, E_UNSUPPORTED = -1, -4  # include/ldpc_hip.h
NO_EARLY_EXIT = 1
DEFAULT = (6, 2, 0.8125, 0)
PARAMS = [DEFAULT, (2, 0, 1.0, 0), (8, 1, 1.0, 1), (5, 1, 1 / 64, 0), (6, 2, 0.5, 3)]  # the five sets of test_gpu_lqmsa.PARAMS
DENSE = [1, 2, 7, 63, 64, 65, 129, 200]  # dense 3 x 6 base: below a pass, the pass edges, a tail of 8 lanes
# Z = 1: three copies of one check on all six bits.  Min-sum on a single parity check satisfies it after one sweep for more than two
# thirds of the frames at every SNR of the bisection's range, so no SNR there leaves a third of the frames at the cap.  That code runs
# at -3 dB, where some frames leave after one sweep and some stay to the cap (asserted), as the consensus code of test_gpu_lqmsa does.
TINY = (("dense", 1),)
IRREGULAR = np.array([[1, 1, 0, 0, 0, 0, 0, 0, 0, 0],
                      [0, 1, 1, 1, 0, 0, 0, 0, 0, 0],
                      [1, 1, 1, 1, 1, 1, 1, 0, 0, 0],
                      [1, 1, 1, 1, 1, 1, 1, 1, 0, 0],
                      [0, 1, 1, 1, 1, 1, 1, 1, 1, 0]], dtype=bool)  # degrees 2, 3, 7, 8, 8; column 8 has degree 1, column 9 is zero
LOOP = np.zeros((4, 33), dtype=bool)  # degrees 9, 16, 17, 33: every row takes the loop form
LOOP[0, :9] = LOOP[1, :16] = LOOP[2, 16:] = LOOP[3, :] = True
ALL_KEYS = [("dense", z) for z in DENSE] + ["irregular", "loop", "extremes", "4x8"]
_CODES, _BATCH, _WANT = {}, {}, {}


def _code(key):
    """-> (oracle edge list, codes.Code, base, Z)"""
    from ldpc_decoders_amd import qc

    if key not in _CODES:
        if key == "irregular":
            c = qc.rand_qc_ldpc(IRREGULAR, 65, np.random.RandomState(11))
            assert (c.qc[0] >= 0).sum(axis=1).tolist() == [2, 3, 7, 8, 8] and sorted(np.unique(c.col_degrees())) == [0, 1, 2, 3, 4, 5]
        elif key == "loop":
            c = qc.rand_qc_ldpc(LOOP, 66, np.random.RandomState(12))
            assert (c.qc[0] >= 0).sum(axis=1).tolist() == [9, 16, 17, 33]
        elif key == "extremes":  # shift 0 and shift Z - 1 side by side in one block row
            base = qc.rand_qc_ldpc(np.ones((3, 6), dtype=bool), 65, np.random.RandomState(13)).qc[0].copy()
            base[0, 0], base[0, 1], base[2, 5] = 0, 64, 64
            c = qc.expand(base, 65)
        elif key == "4x8":
            c = qc.rand_qc_ldpc(qc.regular_mask(4, 8, 3), 27, np.random.RandomState(14))
        else:
            c = qc.rand_qc_ldpc(np.ones((3, 6), dtype=bool), key[1], np.random.RandomState(100 + key[1]), girth6=key[1] > 2)
        _CODES[key] = (O.Edges(c.m, c.n, c.edge_chk, c.edge_var), c, c.qc[0], c.qc[1])
    return _CODES[key]


def _layers(key, order=None):
    from ldpc_decoders_amd import qc

    _, _, base, Z = _code(key)
    return qc.layers_of(Z, np.arange(base.shape[0]) if order is None else order)


def _handle(key, params=None, order=None):
    from ldpc_decoders_amd._device import QcHandle

    _, c, _, Z = _code(key)
    h = QcHandle(c, Z)
    if params is not None:
        h.set_fixed_point(*params)
    if order is not None:
        h.set_order(order)
    return h


def _priors(g, snr, z):
    return O.biawgn_priors(-1 + np.sqrt(O.biawgn_noise_var(snr)) * z, snr)


def _batch(key, B=32, cap=50):
    """fp64 BI-AWGN priors [B, n] at an SNR where the oracle (default parameters, block rows in natural order) says that between a third and
    two thirds of the frames leave before the cap -- the bisection of test_gpu_lqmsa._batch on the same noise draws -- with a frame of
    +-inf priors and an all-zero frame planted in the last two rows.  -> (priors, snr)"""
    if (key, B, cap) not in _BATCH:
        g = _code(key)[0]
        lay = _layers(key)
        z = np.random.RandomState(77).standard_normal((B, g.n))
        lo, hi, snr, frac = -6.0, 12.0, None, None
        for _ in range(0 if key in TINY else 14):
            snr = 0.5 * (lo + hi)
            frac = (LQ.lqmsa_decode(g, None, _priors(g, snr, z)[:B - 2], cap, layers=lay)[1] < cap).mean()
            if frac < 1 / 3:
                lo = snr
            elif frac > 2 / 3:
                hi = snr
            else:
                break
        if key in TINY:
            snr = -3.0
            it = LQ.lqmsa_decode(g, None, _priors(g, snr, z)[:B - 2], cap, layers=lay)[1]
            assert len(np.unique(it)) >= 2, np.bincount(it)
        else:
            assert 1 / 3 <= frac <= 2 / 3, (key, snr, frac)
        pri = _priors(g, snr, z)
        pri[B - 2] = np.where(z[B - 2] < 0.5, np.inf, -np.inf)
        pri[B - 1] = 0.0
        _BATCH[(key, B, cap)] = (np.ascontiguousarray(pri), snr)
    return _BATCH[(key, B, cap)]


def _want(key, tag, y0, pri, cap, params=DEFAULT, order=None, early=True):
    """the oracle's (xhat, iters, soft, peak), computed once per distinct case"""
    k = (key, tag, cap, params, None if order is None else tuple(int(v) for v in order), early, pri.dtype.str, y0 is not None)
    if k not in _WANT:
        _WANT[k] = LQ.lqmsa_decode(_code(key)[0], y0, pri, cap, *params, layers=_layers(key, order), early_exit=early)
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


# ---------------------------------------------------------------------------------------------- 1. every shape, both prior types
@pytest.mark.parametrize("key", ALL_KEYS, ids=str)
def test_equals_the_integer_statement(key):
    """32 frames, cap 50, default parameters, natural order; fp64 and fp32 priors; the +-inf frame and the all-zero frame.  The handle
    reports the detected base, the size rule's bytes and the wave rule's waves."""
    from ldpc_decoders_amd import layered, qc

    g, c, base, Z = _code(key)
    B = 32
    pri, _ = _batch(key, B)
    h = _handle(key)
    assert h.fixed_point() == DEFAULT and h.order().tolist() == list(range(base.shape[0]))
    got_base, got_Z = h.base()
    want_base, _ = qc.find_structure(c, Z)
    assert got_Z == Z and np.array_equal(got_base, want_base) and np.array_equal(got_base, base)
    info = h.info()
    need = layered.lqmsa_lds_bytes(c.m, c.n, c.E, int((base >= 0).sum(axis=1).max()))
    assert info["lds_bytes_per_frame"] == need and info["waves_per_frame"] == qc.qc_waves(layered.LDS_BYTES // need, Z)
    assert info["frames_per_cu"] == min(layered.LDS_BYTES // need, 32 // info["waves_per_frame"]) and info["workgroups"] % info["frames_per_cu"] == 0
    for dt in (np.float64, np.float32):
        p = pri.astype(dt)
        want = _want(key, "parity", None, p, 50)
        assert want[1][B - 1] == 1 and (key in TINY or B / 3 - 2 <= (want[1] < 50).sum() <= 2 * B / 3 + 2)
        _same(_run(h, p, None, 50), want, (key, dt.__name__))
    _same(_run(h, p[:1], None, 50), tuple(a[:1] for a in want[:3]), (key, "B = 1"))


def test_shift_extremes_are_present():
    base, Z = _code("extremes")[2:]
    assert Z == 65 and 0 in base and Z - 1 in base and base[0, 0] == 0 and base[0, 1] == Z - 1


# ---------------------------------------------------------------------------------------------- 2. parameters, caps, flags, y0
@pytest.mark.parametrize("key", [("dense", 65), "irregular", "loop"], ids=str)
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
    easy = pri[np.flatnonzero(_want(key, "params", None, pri, 50)[1] < 50)[:8]]  # frames that leave on their own
    want = _want(key, "unbounded", None, easy, 0)
    assert len(easy) == 8 and want[1].max() < 50
    _same(_run(h, easy, None, 0), want, (key, "max_iter 0"))
    _same(_run(h, easy, None, -3), want, (key, "max_iter -3"))


@pytest.mark.parametrize("key,p", [(("dense", 64), 0.07), (("dense", 200), 0.07), ("irregular", 0.04), ("loop", 0.003)], ids=str)
def test_bsc_with_the_received_word(key, p):
    """Every prior is +-L: every minimum ties.  A received codeword leaves at iteration 0 with x_hat = y0, iters = 0 and soft output 0;
    with LDPC_FLAG_NO_EARLY_EXIT it does not; without y0 the same priors run at least one sweep."""
    g = _code(key)[0]
    B, cap = 32, 50
    y = (np.random.RandomState(9).random_sample((B, g.n)) < p).astype(np.uint8)
    y[0] = 0
    for dt in (np.float64, np.float32):
        pri = O.bsc_priors(y.astype(np.int64), p).astype(dt)
        want = _want(key, "bsc", y, pri, cap)
        assert want[1][0] == 0 and 0 < (want[1] < cap).sum() < B and len(np.unique(want[1])) > 2, np.bincount(want[1])
        h = _handle(key)
        got = _run(h, pri, y, cap)
        _same(got, want, (key, "bsc", dt.__name__))
        assert not got[3][0].any()
    _same(_run(h, pri, y, 3, NO_EARLY_EXIT), _want(key, "bsc free", y, pri, 3, early=False), (key, "bsc, no early exit"))
    want = _want(key, "bsc no y0", None, pri, cap)
    assert want[1][0] == 1
    _same(_run(h, pri, None, cap), want, (key, "bsc priors without y0"))


# ---------------------------------------------------------------------------------------------- 3. waves per frame
@pytest.mark.parametrize("nw", ["1", "2", "4", "8"])
@pytest.mark.parametrize("key", [("dense", 129), ("dense", 200), "loop"], ids=str)
def test_any_number_of_waves(key, nw, monkeypatch):
    """LDPC_QC_NW, read at create: a fresh handle per wave count; Z = 129 leaves waves without a pass from four waves on."""
    monkeypatch.setenv("LDPC_QC_NW", nw)
    pri = _batch(key)[0].astype(np.float32)
    h = _handle(key)
    assert h.info()["waves_per_frame"] == int(nw) and h.info()["frames_per_cu"] <= 32 // int(nw)
    _same(_run(h, pri, None, 50), _want(key, "parity", None, pri, 50), (key, nw))
    if key == ("dense", 200):
        params = PARAMS[2]
        h.set_fixed_point(*params)
        _same(_run(h, pri, None, 50), _want(key, "params", None, pri, 50, params), (key, nw, params))


# ---------------------------------------------------------------------------------------------- 4. batch size and frame position
@pytest.mark.parametrize("key", [("dense", 65), "4x8"], ids=str)
def test_any_batch_size_and_position(key, monkeypatch):
    pri = _batch(key, 64)[0].astype(np.float32)
    want = _want(key, "parity 64", None, pri, 50)
    h = _handle(key)
    ext = np.concatenate([pri, pri[:1]])
    for B in (1, 63, 64, 65):
        idx = np.arange(B) % 64
        _same(_run(h, ext[:B], None, 50), tuple(a[idx] for a in want[:3]), (key, B))
    # three times the grid and 17: every workgroup takes several frames with mixed exit times; a frame gives the same result at any position
    monkeypatch.setenv("LDPC_QC_NW", "8")  # at most 4 frames per CU: the smallest grid
    small = _handle(key)
    B = 3 * small.info()["workgroups"] + 17
    idx = np.random.RandomState(5).randint(0, 64, size=B)
    _same(_run(small, pri[idx], None, 50), tuple(a[idx] for a in want[:3]), (key, "B = %d" % B))


# ---------------------------------------------------------------------------------------------- 5. the order of the block rows
@pytest.mark.parametrize("key", [("dense", 63), "irregular"], ids=str)
def test_block_row_order(key):
    from ldpc_decoders_amd import _lib, qc

    g, c, base, Z = _code(key)
    mb = base.shape[0]
    pri = _batch(key)[0].astype(np.float32)
    h = _handle(key)
    lib = _lib.load()
    perm = np.random.RandomState(3).permutation(mb)
    assert not np.array_equal(perm, np.arange(mb))
    for name, order in (("reversed", np.arange(mb)[::-1].copy()), ("random", perm)):
        h.set_order(order)
        assert np.array_equal(h.order(), order)
        want = _want(key, "order", None, pri, 50, order=order)
        _same(_run(h, pri, None, 50), want, (key, name))
    assert not np.array_equal(want[1], _want(key, "parity", None, pri, 50)[1]) or not np.array_equal(want[2], _want(key, "parity", None, pri, 50)[2])
    # refused orders leave the previous one in force and the handle usable
    bad = [np.zeros(mb, dtype=np.int32), np.arange(1, mb + 1, dtype=np.int32), np.where(np.arange(mb) == 1, -1, np.arange(mb)).astype(np.int32),
           np.arange(mb - 1, dtype=np.int32), np.arange(mb + 1, dtype=np.int32)]
    for order in bad:
        assert lib.ldpc_qc_set_order(h.h, order.ctypes.data, order.size) == E_ARG
        assert np.array_equal(h.order(), perm)
    _same(_run(h, pri, None, 50), want, (key, "after the refusals"))
    h.set_order(None)
    assert np.array_equal(h.order(), np.arange(mb))
    _same(_run(h, pri, None, 50), _want(key, "parity", None, pri, 50), (key, "natural again"))
    # the Python class carries an order to the handle
    dec = qc.QCMSA(c, max_iter=50, qc_order=perm)
    assert dec.qc_lift == Z and np.array_equal(dec.layers, qc.layers_of(Z, perm))
    x, it = dec.decode_batch(None, pri)
    assert np.array_equal(x, want[0]) and np.array_equal(it, want[1]) and np.array_equal(dec.last_iters, want[1])


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_create_refusals():
    import torch

    from ldpc_decoders_amd import _lib, codes, layered, qc
    from ldpc_decoders_amd._device import QcHandle

    g, c, base, Z = _code(("dense", 7))
    with pytest.raises(_lib.LdpcHipError, match="error %d.*divide" % E_ARG):
        QcHandle(c, 5)
    with pytest.raises(_lib.LdpcHipError, match="error %d.*divide" % E_ARG):
        QcHandle(c, 0)
    # one edge moved inside its block: the block is named and LQMSA is pointed to
    var = c.edge_var.copy()
    k = int(np.flatnonzero((c.edge_chk == 2 * Z + 3) & (c.edge_var // Z == 4))[0])
    var[k] = 4 * Z + (var[k] + 1) % Z
    with pytest.raises(_lib.LdpcHipError, match=r"error %d.*block \(2, 4\).*ldpc_lqmsa_create" % E_UNSUPPORTED):
        QcHandle(codes.Code.from_edges(c.m, c.n, c.edge_chk, var), Z)
    with pytest.raises(_lib.LdpcHipError, match="error %d.*block" % E_UNSUPPORTED):
        QcHandle(codes.get_code("12_3_4_ldpc"), 3)
    # a block row of degree 1, past the Python checks
    with pytest.raises(_lib.LdpcHipError, match="error %d.*degree 1" % E_UNSUPPORTED):
        QcHandle(qc.expand(np.array([[0, 1, -1], [-1, -1, 2]]), 5), 5)
    # dense 3 x 6 on either side of the LDS rule: 12 Z + 24 Z + 16 <= 163840 up to Z = 4550
    z_ok = (layered.LDS_BYTES - 16) // 36
    assert layered.lqmsa_lds_bytes(3 * z_ok, 6 * z_ok, 18 * z_ok, 6) <= layered.LDS_BYTES < layered.lqmsa_lds_bytes(3 * z_ok + 3, 6 * z_ok + 6, 18 * z_ok + 18, 6)
    rng = np.random.RandomState(21)
    with pytest.raises(_lib.LdpcHipError, match="error %d.*LDPC_ALG_LMSA" % E_UNSUPPORTED) as e:
        QcHandle(qc.rand_qc_ldpc(np.ones((3, 6), dtype=bool), z_ok + 1, rng), z_ok + 1)
    assert "bytes of LDS" in str(e.value)
    big_code = qc.rand_qc_ldpc(np.ones((3, 6), dtype=bool), z_ok, rng)
    big = QcHandle(big_code, z_ok)
    assert big.info()["waves_per_frame"] == 8 and big.info()["frames_per_cu"] == 1
    gb = O.Edges(big_code.m, big_code.n, big_code.edge_chk, big_code.edge_var)
    p32 = _priors(gb, 0.0, np.random.RandomState(8).standard_normal((4, big_code.n))).astype(np.float32)
    _same(_run(big, p32, None, 3), LQ.lqmsa_decode(gb, None, p32, 3, layers=qc.layers_of(z_ok, np.arange(3))), "the largest accepted frame")
    # the calls of the handle
    h = _handle(("dense", 7))
    for bad in ((9, 2, 0.8125, 0), (1, 2, 0.8125, 0), (6, 9, 0.8125, 0), (6, 2, 0.8, 0), (6, 2, 0.0, 0), (6, 2, 0.8125, -1)):
        with pytest.raises(_lib.LdpcHipError, match="error %d.*ldpc_qc_set_fixed_point" % E_ARG):
            h.set_fixed_point(*bad)
        assert h.fixed_point() == DEFAULT
    pri = torch.zeros((4, c.n), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.LdpcHipError, match="error %d.*LDPC_FLAG_NO_EARLY_EXIT" % E_UNSUPPORTED):
        h.decode_device(pri, None, 5, flags=2)
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        h.simulate("bec", 0.1, 0, SEED, STREAM, 0, 64, 5, cnt)
    odd = _handle("irregular")  # block rows of degree 3 and 7: the all-ones word is no codeword
    with pytest.raises(_lib.LdpcHipError, match="odd degree"):
        odd.simulate("bsc", 0.1, 1, SEED, STREAM, 0, 64, 5, cnt)
    with pytest.raises(_lib.LdpcHipError, match="codeword must be 0 or 1"):
        odd.simulate("bsc", 0.1, 2, SEED, STREAM, 0, 64, 5, cnt)


# ---------------------------------------------------------------------------------------------- 7. the generic kernel agrees
@pytest.mark.parametrize("key", [("dense", 129), "irregular", "loop"], ids=str)
def test_the_generic_kernel_returns_the_same_tensors(key):
    """LqmsaHandle with layers = c // Z and QcHandle: identical bytes, words, iteration counts and soft outputs."""
    import torch

    from ldpc_decoders_amd._device import LqmsaHandle

    g, c, base, Z = _code(key)
    pri = torch.from_numpy(_batch(key)[0].astype(np.float32)).cuda()
    generic = LqmsaHandle(c)
    generic.set_layers(np.arange(c.m) // Z)
    a = generic.decode_device(pri, None, 50, bits=True, soft=True)
    b = _handle(key).decode_device(pri, None, 50, bits=True, soft=True)
    assert len(a) == len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert 0 < (a[1] < 50).sum() < len(a[1])


# ---------------------------------------------------------------------------------------------- 8. simulate
@pytest.mark.parametrize("channel,param", [("biawgn", 2.5), ("bsc", 0.07)])
def test_simulate_equals_channel_decode_count(channel, param):
    """ldpc_qc_simulate's counters are the oracle's on the priors ldpc_channel writes for the same (seed, stream, frame0): 128 frames from
    frame 1000 on, two calls accumulate."""
    import torch

    from ldpc_decoders_amd import _lib

    key, B, cap, frame0, bins = ("dense", 65), 128, 20, 1000, 21
    g = _code(key)[0]
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    pri = torch.empty((B, g.n), dtype=torch.float32, device="cuda")
    y = torch.empty((B, g.n), dtype=torch.uint8, device="cuda") if channel == "bsc" else None
    _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE["f32"], float(param), 0, SEED, STREAM, frame0, B, g.n, pri.data_ptr(),
                                None if y is None else y.data_ptr(), st))
    x, it, _, _ = LQ.lqmsa_decode(g, None if y is None else y.cpu().numpy(), pri.cpu().numpy(), cap, layers=_layers(key))
    wrong = x.any(axis=1)
    assert 0 < wrong.sum() < B
    h = _handle(key)
    cnt = torch.zeros(_lib.CNT_HIST0 + bins, dtype=torch.int64, device="cuda")
    h.simulate(channel, param, 0, SEED, STREAM, frame0, B, cap, cnt, hist_bins=bins)
    got = cnt.cpu().numpy()
    assert got[_lib.CNT_TOT] == B and got[_lib.CNT_WEC] == wrong.sum() and got[_lib.CNT_BEC] == x.sum() and got[_lib.CNT_ITER_SUM] == it.sum()
    assert np.array_equal(got[_lib.CNT_HIST0:], np.bincount(it, minlength=bins))
    h.simulate(channel, param, 0, SEED, STREAM, frame0, 50, cap, cnt, hist_bins=bins)  # accumulates; the first 50 frames again
    got2 = cnt.cpu().numpy()
    assert got2[_lib.CNT_TOT] == B + 50 and got2[_lib.CNT_WEC] == wrong.sum() + wrong[:50].sum()
    # the all-ones word (every block row has degree 6): the channel negates, the counters count against it
    cnt.zero_()
    h.simulate(channel, param, 1, SEED, STREAM, frame0, B, cap, cnt)
    got1 = cnt.cpu().numpy()
    assert got1[_lib.CNT_TOT] == B and 0 < got1[_lib.CNT_WEC] < B


def test_simulate_random_codewords():
    """codeword = -1 through the handle: encoder words, ldpc_channel_sent, decode, ldpc_count_errors_words -- the same steps on the oracle."""
    import torch

    from ldpc_decoders_amd import _lib

    key, B, cap, frame0 = ("dense", 65), 128, 20, 64
    g, c = _code(key)[:2]
    h = _handle(key)
    cnt = torch.zeros(_lib.CNT_HIST0, dtype=torch.int64, device="cuda")
    h.simulate("biawgn", 2.5, -1, SEED, STREAM, frame0, B, cap, cnt)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    sent = c.encoder().handle(h.device).encode_random(SEED, STREAM, frame0, B)
    pri = torch.empty((B, g.n), dtype=torch.float32, device="cuda")
    _lib.check(lib.ldpc_channel_sent(_lib.CHANNEL["biawgn"], _lib.DTYPE["f32"], 2.5, sent.data_ptr(), SEED, STREAM, frame0, B, g.n, pri.data_ptr(), None, st))
    x, it, _, _ = LQ.lqmsa_decode(g, None, pri.cpu().numpy(), cap, layers=_layers(key))
    s = sent.cpu().numpy()
    assert s.any() and 0 < (x != s).any(axis=1).sum() < B
    got = cnt.cpu().numpy()
    assert (got[_lib.CNT_TOT], got[_lib.CNT_WEC], got[_lib.CNT_BEC], got[_lib.CNT_ITER_SUM]) == (B, (x != s).any(axis=1).sum(), (x != s).sum(), it.sum())


# ---------------------------------------------------------------------------------------------- 9. the command line
def test_cli(tmp_path, monkeypatch):
    """A generated code in the ordinary text format, found again from H: the result file carries the lifting size the decoder ran with."""
    from ldpc_decoders_amd import codes, main, qc

    code_dir = tmp_path / "codes"
    monkeypatch.setenv(codes.file_codes_dir_string, str(code_dir))
    path, = qc.gen_rand_qc(qc.setup_parser().parse_args("1 4 8 27 --seed 5 --dir".split() + [str(code_dir)]))
    assert os.path.basename(path) == "216_qc_4x8_z27_1.txt"
    argv = "biawgn 216_qc_4x8_z27_1 QCMSA --params 3.0 --max-iter 20 --batch 4096 --max-frames 4096".split()
    main.main(argv + ["--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-216_qc_4x8_z27_1-QCMSA-0-100-20-6-2-0.8125-0.0-27.json")) as fp:
        res = json.load(fp)
    assert res["decoder"] == "QCMSA" and res["max_iter"] == 20 and res["qc_lift"] == 27
    assert (res["msa_bits"], res["msa_frac_bits"], res["msa_scale"], res["msa_offset"]) == (6, 2, 0.8125, 0.0)
    tot, wec, bec = res["tot"]["3.0"], res["wec"]["3.0"], res["bec"]["3.0"]
    assert tot == 4096 and 4 <= wec < tot // 2 and wec <= bec <= wec * 216 and res["wer"]["3.0"] == pytest.approx(wec / tot)
    # random codewords and a given lifting size (a divisor of 27 for which the blocks are still shifted identities is as good)
    main.main(argv + ["--codeword", "-1", "--qc-lift", "27", "--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-216_qc_4x8_z27_1-QCMSA--1-100-20-6-2-0.8125-0.0-27.json")) as fp:
        res = json.load(fp)
    assert res["tot"]["3.0"] == 4096 and 4 <= res["wec"]["3.0"] < 2048

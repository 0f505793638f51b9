"""Layered min-sum on the GPU (LDPC_ALG_LMSA, bpa.LMSA): decisions, iteration counts and soft outputs bit for bit those of the numpy
restatement (tests/lmsa_oracle.py) in fp64 and fp32 -- every code shape, the BSC with its iteration-0 rule, every entry point, frame
repacks, custom layerings, the Monte-Carlo entry points, the refusals, what the schedule is worth, OSD behind it and the command line."""
import ctypes
import json
import os

import numpy as np
import pytest

import bp_oracle as O
import lmsa_oracle as L
import nmsa_oracle as N
import osd_oracle as OSD

pytestmark = pytest.mark.gpu

CORRECTIONS = [(1.0, 0.0), (0.8125, 0.0), (1.0, 0.25)]
PREC = [("f64", np.float64), ("f32", np.float32)]
_CACHE = {}


def _code(name):
    """-> (oracle edge list, codes.Code)"""
    from ldpc_decoders_amd import codes

    if name not in _CACHE:
        c = codes.get_code(name)
        _CACHE[name] = (O.Edges(c.m, c.n, c.edge_chk, c.edge_var), c)
    return _CACHE[name]


def _handle(name, prec, corr=None, backend="auto", alg="LMSA"):
    from ldpc_decoders_amd._device import DecoderHandle

    h = DecoderHandle(_code(name)[1], alg, prec, backend)
    if corr is not None:
        h.set_correction(*corr)
    return h


def _biawgn(g, snr, B, seed):
    rng = np.random.RandomState(seed)
    return O.biawgn_priors(-1 + rng.normal(0, np.sqrt(O.biawgn_noise_var(snr)), (B, g.n)), snr)


def _soft(h, pri, y0, max_iter, flags=0):
    import torch

    p = torch.from_numpy(np.ascontiguousarray(pri)).cuda()
    y = None if y0 is None else torch.from_numpy(np.ascontiguousarray(y0)).cuda()
    x, it, soft = h.decode_soft_device(p, y, max_iter, flags)
    return x.cpu().numpy(), it.cpu().numpy(), soft.cpu().numpy()


def _same(got, want, where):
    x, it, soft = got
    xr, ir, sr = want
    assert np.array_equal(it, ir), (where, np.flatnonzero(it != ir)[:8], it[:8], ir[:8])
    assert np.array_equal(x, xr), (where, np.flatnonzero((x != xr).any(axis=1))[:8])
    assert soft.dtype == sr.dtype and np.array_equal(soft, sr), (where, np.flatnonzero((soft != sr).any(axis=1))[:8])


# ---------------------------------------------------------------------------------------------- 1. parity with the restatement
# (code, SNR in dB, frames, sweep cap): B = 70 is two tiles, the second with 6 live lanes
PARITY = [("7_4_hamming", 2.0, 70, 25), ("4_2_test", 2.0, 70, 25), ("12_3_4_ldpc", 2.0, 70, 25), ("512_3_6_rand_ldpc_1", 2.0, 70, 25),
          ("1200_3_6_rand_ldpc_1", 2.0, 70, 25), ("1200_rho_x5_rand_ldpc_5", 1.5, 70, 25), ("margulis", 2.0, 20, 15)]


@pytest.mark.parametrize("prec,dt", PREC)
@pytest.mark.parametrize("name,snr,B,cap", PARITY)
def test_parity_with_the_restatement(name, snr, B, cap, prec, dt):
    """array_equal on decisions, iteration counts and soft outputs; three corrections; B frames and a single frame."""
    g = _code(name)[0]
    pri = _biawgn(g, snr, B, 40).astype(dt)
    h = _handle(name, prec)
    assert h.correction() == (1.0, 0.0) and h.kernel_name() == "" and h.fused_info()["waves_per_frame"] == 0
    nl, lay = h.layers()
    assert np.array_equal(lay, L.greedy_layers(g)) and nl == lay.max() + 1
    for scale, offset in CORRECTIONS:
        h.set_correction(scale, offset)
        want = L.lmsa_decode(g, None, pri, cap, scale, offset, dtype=dt)
        _same(_soft(h, pri, None, cap), want, (name, prec, scale, offset))
        assert h.last_stats()[0] == "stream"
        if name in ("1200_3_6_rand_ldpc_1", "512_3_6_rand_ldpc_1", "margulis") and scale < 1:
            assert 0 < (want[1] < cap).sum(), "the case must have frames that leave"
        _same(_soft(h, pri[:1], None, cap), tuple(a[:1] for a in want), (name, prec, scale, offset, "B = 1"))


# ---------------------------------------------------------------------------------------------- 2. BSC, iteration-0 rule
def test_bsc_with_the_received_word():
    """fp64, p = 0.07 (62 of the 70 frames leave after 2 .. 24 sweeps, 8 never do); every prior is +-L, so every minimum ties; the
    all-zero and the all-one row are codewords and leave at iteration 0: iters = 0, x_hat = y0, soft output 0."""
    name, p, B, cap = "1200_3_6_rand_ldpc_1", 0.07, 70, 25
    g = _code(name)[0]
    y = (np.random.RandomState(7).random_sample((B, g.n)) < p).astype(np.int64)
    y[0], y[1] = 0, 1
    pri, y0 = O.bsc_priors(y, p), y.astype(np.uint8)
    h = _handle(name, "f64", (0.8125, 0.0))
    want = L.lmsa_decode(g, y0, pri, cap, 0.8125, 0.0)
    assert want[1][:2].tolist() == [0, 0] and 0 < (want[1] == cap).sum() < B - 2 and len(np.unique(want[1])) > 5
    got = _soft(h, pri, y0, cap)
    _same(got, want, "bsc")
    assert (got[0][1] == 1).all() and not got[2][:2].any()
    # the Python class, one frame per call: a received codeword comes back as it is
    from ldpc_decoders_amd import bsc

    dec = bsc.LMSA(p, _code(name)[1], max_iter=cap, msa_scale=0.8125)
    assert dec.decode(y[1]) is not None and int(dec.dec.last_iters[0]) == 0
    assert np.array_equal(np.asarray(dec.decode(y[5])), want[0][5]) and int(dec.dec.last_iters[0]) == want[1][5]
    xb, ib = dec.decode_batch(y)  # (int64 words, as the reference's channel hands them over)
    assert np.array_equal(xb, want[0]) and np.array_equal(ib, want[1])


# ---------------------------------------------------------------------------------------------- 3. entry points and flags
@pytest.mark.parametrize("prec,dt", PREC)
def test_entry_points_and_flags(prec, dt):
    import torch
    from ldpc_decoders_amd import _lib
    from ldpc_decoders_amd._device import unpack_bits

    name, B, cap = "1200_rho_x5_rand_ldpc_5", 70, 12
    g = _code(name)[0]
    pri = _biawgn(g, 2.0, B, 3).astype(dt)
    h = _handle(name, prec, (0.8125, 0.0))
    want = L.lmsa_decode(g, None, pri, cap, 0.8125, 0.0, dtype=dt)
    assert 0 < (want[1] < cap).sum() < B
    p = torch.from_numpy(pri).cuda()
    x, it = h.decode_device(p, None, cap)
    assert np.array_equal(x.cpu().numpy(), want[0]) and np.array_equal(it.cpu().numpy(), want[1])
    bits, _, it = h.decode_device_bits(p, None, cap)
    assert np.array_equal(unpack_bits(bits.cpu().numpy(), g.n), want[0]) and np.array_equal(it.cpu().numpy(), want[1])
    _same(_soft(h, pri, None, cap), want, "soft")
    x, it = h.decode_host(pri, None, cap)
    assert np.array_equal(x, want[0]) and np.array_equal(it, want[1])
    bits, _, it = h.decode_host_bits(pri, None, cap)
    assert np.array_equal(unpack_bits(bits, g.n), want[0]) and np.array_equal(it, want[1])
    # no early exit: exactly `cap` sweeps for every frame
    full = L.lmsa_decode(g, None, pri, cap, 0.8125, 0.0, dtype=dt, early_exit=False)
    assert (full[1] == cap).all() and not np.array_equal(full[2], want[2])
    _same(_soft(h, pri, None, cap, flags=_lib.FLAG_NO_EARLY_EXIT), full, "no early exit")
    assert h.last_stats() == ("stream", cap)


# ---------------------------------------------------------------------------------------------- 4. frame repacks
def test_repack_invariance(monkeypatch):
    """2.5 dB, 384 frames (six tiles), plain layered min-sum, cap 50: almost every frame leaves within 10 sweeps, five are still live at
    the poll behind sweep 16 (in three tiles), so the eager policy gathers them.  Identical decisions and iteration counts with and
    without, and those of the restatement."""
    name, B, cap = "1200_3_6_rand_ldpc_1", 384, 50
    g = _code(name)[0]
    pri = _biawgn(g, 2.5, B, 11).astype(np.float32)
    want = L.lmsa_decode(g, None, pri[:70], cap, 1.0, 0.0, dtype=np.float32)
    monkeypatch.setenv("LDPC_STREAM_REPACK", "0")
    h0 = _handle(name, "f32")
    x0, i0 = h0.decode_host(pri, None, cap)
    assert h0.last_repacks() == 0
    monkeypatch.setenv("LDPC_STREAM_REPACK", "1")
    monkeypatch.setenv("LDPC_STREAM_REPACK_FILL", "0.97")
    h1 = _handle(name, "f32")
    x1, i1 = h1.decode_host(pri, None, cap)
    print("repacks %d, frames beyond 16 sweeps %d, beyond 32 %d" % (h1.last_repacks(), (i0 > 16).sum(), (i0 > 32).sum()))
    assert h1.last_repacks() >= 1
    assert np.array_equal(x1, x0) and np.array_equal(i1, i0)
    assert np.array_equal(x0[:70], want[0]) and np.array_equal(i0[:70], want[1])


# ---------------------------------------------------------------------------------------------- 5. custom layers
def test_custom_layers():
    from ldpc_decoders_amd import _lib, bpa

    lib = _lib.load()
    name, cap = "512_3_6_rand_ldpc_1", 25
    g, code = _code(name)
    pri = _biawgn(g, 2.0, 70, 21)
    dec = bpa.LMSA(code, max_iter=cap, msa_scale=0.8125)
    greedy = L.greedy_layers(g)
    assert np.array_equal(dec.layers, greedy)
    dflt = _soft(dec.handle, pri, None, cap)
    _same(dflt, L.lmsa_decode(g, None, pri, cap, 0.8125, 0.0), "greedy")
    rev = greedy.max() - greedy
    dec.handle.set_layers(rev)
    assert np.array_equal(dec.layers, rev) and dec.handle.layers()[0] == greedy.max() + 1
    got = _soft(dec.handle, pri, None, cap)
    _same(got, L.lmsa_decode(g, None, pri, cap, 0.8125, 0.0, layers=rev), "reversed")
    assert not np.array_equal(got[2], dflt[2])
    # a refused layering (two checks of layer 0 share a variable; a negative entry; a wrong length) leaves the reversed one in force
    bad = rev.copy()
    bad[:] = 0
    for lay, m in ((bad, g.m), (-rev - 1, g.m), (rev, g.m - 1)):
        lay32 = np.ascontiguousarray(lay, dtype=np.int32)
        assert lib.ldpc_decoder_set_layers(dec.handle.h, lay32.ctypes.data, m) == -1  # LDPC_E_ARG
        assert lib.ldpc_last_error()
    with pytest.raises(ValueError):
        dec.handle.set_layers(bad)
    with pytest.raises(ValueError):
        bpa.LMSA(code, max_iter=cap, layers=bad)
    assert np.array_equal(dec.layers, rev)
    _same(_soft(dec.handle, pri, None, cap), L.lmsa_decode(g, None, pri, cap, 0.8125, 0.0, layers=rev), "after the refusals")
    dec.handle.set_layers(None)  # NULL restores the greedy layering
    _same(_soft(dec.handle, pri, None, cap), dflt, "greedy again")
    # one check per layer, through the constructor
    g2, code2 = _code("12_3_4_ldpc")
    pri2 = _biawgn(g2, 2.0, 70, 22)
    for lay in (np.arange(g2.m), np.arange(g2.m)[::-1] * 3):
        d2 = bpa.LMSA(code2, max_iter=cap, msa_scale=0.8125, layers=lay, precision="f32")
        assert d2.handle.layers()[0] == g2.m and np.array_equal(d2.layers, lay)
        _same(_soft(d2.handle, pri2.astype(np.float32), None, cap), L.lmsa_decode(g2, None, pri2, cap, 0.8125, 0.0, layers=lay, dtype=np.float32), "one per layer")


# ---------------------------------------------------------------------------------------------- 6. Monte-Carlo entry points
@pytest.mark.parametrize("channel,param", [("biawgn", 2.0), ("bsc", 0.06)])
@pytest.mark.parametrize("prec,dt", PREC)
def test_simulate_counters(prec, dt, channel, param):
    """ldpc_simulate == ldpc_channel -> restatement -> count on the same seed; the rows of ldpc_simulate_rounds are single calls."""
    import torch

    name, B, seed, stream, frame0, cap = "1200_3_6_rand_ldpc_1", 130, 77, 2, 1000, 25
    g = _code(name)[0]
    h = _handle(name, prec, (0.8125, 0.0))
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    h.simulate(channel, param, 0, seed, stream, frame0, B, cap, cnt)
    torch.cuda.synchronize()
    assert h.last_stats()[0] == "stream"
    pri, y = h.channel_device(channel, param, 0, seed, stream, frame0, B)
    xr, ir, _ = L.lmsa_decode(g, None if y is None else y.cpu().numpy(), pri.cpu().numpy(), cap, 0.8125, 0.0, dtype=dt)
    assert cnt.cpu().tolist() == [B, int(xr.any(axis=1).sum()), int(xr.sum()), int(ir.sum())]
    assert 0 < (ir < cap).sum()
    rows = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    h.simulate_rounds(channel, param, 0, seed, stream, frame0, B // 2, 2, B // 2, cap, rows)
    single = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    for r in range(2):
        h.simulate(channel, param, 0, seed, stream, frame0 + r * (B // 2), B // 2, cap, single[r])
    torch.cuda.synchronize()
    assert rows.cpu().tolist() == single.cpu().tolist() and rows.sum(dim=0).cpu().tolist() == cnt.cpu().tolist()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_device_usable():
    import torch
    from ldpc_decoders_amd import _lib, bec, codes
    from ldpc_decoders_amd._device import DecoderHandle, code_handle

    lib = _lib.load()
    E_ARG, E_UNSUPPORTED = -1, -4  # include/ldpc_hip.h
    name = "1200_3_6_rand_ldpc_1"
    g, code = _code(name)

    def create(c, alg, prec, backend):
        h = ctypes.c_void_p()
        rc = lib.ldpc_decoder_create(code_handle(c).h, _lib.ALG[alg], _lib.DTYPE[prec], _lib.BACKEND[backend], ctypes.byref(h))
        return rc, (lib.ldpc_last_error() or b"").decode()

    for prec, backend in (("f32", "fused"), ("f64", "fused"), ("f16", "auto"), ("f16", "stream")):
        rc, msg = create(code, "LMSA", prec, backend)
        assert rc == E_UNSUPPORTED and "LMSA" in msg, (prec, backend, rc, msg)
    deg1 = codes.Code(None, np.array([[1, 1, 1, 0], [0, 0, 1, 1], [0, 0, 0, 1]]))
    rc, msg = create(deg1, "LMSA", "f64", "auto")
    assert rc == E_UNSUPPORTED and "degree" in msg
    assert create(deg1, "NMSA", "f64", "stream")[0] == 0  # the flooding decoders take such a code
    pri64 = _biawgn(g, 2.0, 64, 9)
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        h = DecoderHandle(code, "LMSA", prec)
        pri = torch.from_numpy(pri64).to(dt).cuda()
        xh = torch.empty((64, g.n), dtype=torch.uint8, device="cuda")
        it = torch.empty(64, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        grid = _lib.flag_prior_grid(4)
        rc = lib.ldpc_decode(h.h, pri.data_ptr(), None, 64, 10, grid, xh.data_ptr(), it.data_ptr(), st)
        msg = (lib.ldpc_last_error() or b"").decode()
        assert rc == E_UNSUPPORTED and "prior grid" in msg and "LMSA" in msg
        rc = lib.ldpc_simulate(h.h, _lib.CHANNEL["biawgn"], 2.0, 0, 1, 0, 0, 64, 10, grid, 0, cnt.data_ptr(), st)
        assert rc == E_UNSUPPORTED and "prior grid" in (lib.ldpc_last_error() or b"").decode()
        assert lib.ldpc_simulate(h.h, _lib.CHANNEL["bec"], 0.4, 0, 1, 0, 0, 64, 10, 0, 0, cnt.data_ptr(), st) == E_ARG
        for scale, offset in ((0.0, 0.0), (1.5, 0.0), (float("nan"), 0.0), (0.8, -0.25), (0.8, float("inf"))):
            assert lib.ldpc_decoder_set_correction(h.h, ctypes.c_double(scale), ctypes.c_double(offset)) == E_ARG
        assert h.correction() == (1.0, 0.0) and int(cnt.sum()) == 0
        # the decoder is as usable as before
        ndt = np.float32 if prec == "f32" else np.float64
        want = L.lmsa_decode(g, None, pri64[:8].astype(ndt), 10, 1.0, 0.0, dtype=ndt)
        x, i = h.decode_device(pri[:8].contiguous(), None, 10)
        assert np.array_equal(x.cpu().numpy(), want[0]) and np.array_equal(i.cpu().numpy(), want[1])
    # set / get layers on a decoder of another algorithm
    hm = DecoderHandle(code, "NMSA", "f32")
    nl = ctypes.c_int32(0)
    assert lib.ldpc_decoder_set_layers(hm.h, None, 0) == E_ARG and lib.ldpc_decoder_get_layers(hm.h, ctypes.byref(nl), None) == E_ARG
    assert lib.ldpc_abi_version() == 4
    with pytest.raises(NotImplementedError):
        bec.LMSA(0.4, code, max_iter=10)
    x, it = hm.decode_device(torch.from_numpy(pri64).float().cuda(), None, 50)
    torch.cuda.synchronize()
    assert (it.cpu().numpy() > 0).all()


# ---------------------------------------------------------------------------------------------- 8. the point
def test_the_point_of_it():
    """The 48 frames of tests/test_lmsa_cpu.py (1200_3_6_rand_ldpc_1, 2.0 dB, RandomState(1), scale 0.8125, cap 50): the device's layered and
    flooding (streaming kernels) sweep totals are their restatements' totals -- 334 against 584."""
    name, cap = "1200_3_6_rand_ldpc_1", 50
    g = _code(name)[0]
    pri = _biawgn(g, 2.0, 48, 1)
    _, il = _handle(name, "f64", (0.8125, 0.0)).decode_host(pri, None, cap)
    _, ifl = _handle(name, "f64", (0.8125, 0.0), backend="stream", alg="NMSA").decode_host(pri, None, cap)
    wl = L.lmsa_decode(g, None, pri, cap, 0.8125, 0.0)[1]
    wf = N.nmsa_decode(g, None, pri, cap, 0.8125, 0.0)[1]
    print("sweeps: layered %d, flooding %d (%.3f)" % (il.sum(), ifl.sum(), il.sum() / ifl.sum()))
    assert np.array_equal(il, wl) and np.array_equal(ifl, wf)
    assert int(il.sum()) == int(wl.sum()) and int(ifl.sum()) == int(wf.sum()) and wl.sum() <= 0.75 * wf.sum()


# ---------------------------------------------------------------------------------------------- 9. OSD behind it
@pytest.mark.parametrize("prec,dt", PREC)
def test_osd_in_front(prec, dt):
    """bpa.OSD(osd_bp="LMSA"): the frames whose layered soft output is no codeword get the ordered-statistics word of osd_oracle on that
    soft output, the others keep BP's word."""
    from ldpc_decoders_amd import bpa

    name, B, cap = "512_3_6_rand_ldpc_1", 40, 20
    g, code = _code(name)
    H = code.parity_mtx.astype(np.uint8)
    pri = _biawgn(g, 1.5, B, 9).astype(dt)
    x, it, soft = L.lmsa_decode(g, None, pri, cap, 0.8125, 0.0, dtype=dt)
    listed = np.flatnonzero(((OSD.hard(soft).astype(np.int64) @ H.T.astype(np.int64)) % 2).any(axis=1))
    assert 4 <= len(listed) < B
    want_x, want_pick = x.copy(), np.full(B, -1, dtype=np.int64)
    for f in listed:
        want_x[f], want_pick[f], _ = OSD.osd_frame(H, soft[f], pri[f], 1, 64)
    dec = bpa.OSD(code, max_iter=cap, osd_bp="LMSA", osd_order=1, osd_depth=64, msa_scale=0.8125, precision=prec)
    assert dec.bp.handle.alg == "LMSA"
    gx, gi = dec.decode_batch(None, pri)
    assert np.array_equal(gi, it) and np.array_equal(dec.last_pick, want_pick) and np.array_equal(gx, want_x)
    assert not ((gx.astype(np.int64) @ H.T.astype(np.int64)) % 2).any()


# ---------------------------------------------------------------------------------------------- 10. command line
def test_command_line(tmp_path):
    from ldpc_decoders_amd import main

    r = main.main(["biawgn", "1200_3_6_rand_ldpc_1", "LMSA", "--params", "2.5", "--max-iter", "20", "--min-wec", "3", "--max-frames", "4096", "--batch", "1024",
                   "--data_dir", str(tmp_path), "--console"])
    with open(os.path.join(str(tmp_path), "biawgn-1200_3_6_rand_ldpc_1-LMSA-0-3-20-0.8125-0.0.json")) as fp:
        got = json.load(fp)
    assert list(got)[:8] == ["channel", "code", "decoder", "codeword", "min_wec", "max_iter", "msa_scale", "msa_offset"]
    assert list(got)[8:13] == ["tot", "wec", "wer", "bec", "ber"]
    assert (got["decoder"], got["msa_scale"], got["msa_offset"], got["max_iter"]) == ("LMSA", 0.8125, 0.0, 20)
    assert got["tot"]["2.5"] == r[2.5]["tot"] and 1024 <= got["tot"]["2.5"] <= 4096 and got["wer"]["2.5"] < 0.05
    # random codewords on the device and the reference-exact mode run through the same decoder
    r = main.main(["biawgn", "1200_3_6_rand_ldpc_1", "LMSA", "--params", "1.5", "--max-iter", "20", "--min-wec", "5", "--codeword", "-1",
                   "--data_dir", str(tmp_path / "cw"), "--console", "--batch", "512"])
    assert r[1.5]["wec"] >= 5 and r[1.5]["tot"] >= 512
    r = main.main(["bsc", "1200_3_6_rand_ldpc_1", "LMSA", "--params", "0.08", "--max-iter", "20", "--min-wec", "3", "--exact", "--np-seed", "12",
                   "--data_dir", str(tmp_path / "exact"), "--console"])
    assert r[0.08]["wec"] >= 3

"""Fixed-point min-sum on the GPU (LDPC_ALG_QMSA, bpa.QMSA): bit-exact against the CPU restatement (tests/qmsa_oracle.py) on every frame,
identical outputs of the f64 / f32 / f16 decoders on both backends, plain min-sum where no clamp can bind, the quantiser's edges, the
Monte-Carlo entry points, the parameters and refusals, the command line."""
import ctypes
import json
import os

import numpy as np
import pytest

import bp_oracle as O
import qmsa_oracle as Q
from helpers import CODES_DIR, golden_edges

pytestmark = pytest.mark.gpu

# (bits, frac_bits, scale, offset): the default, 5-bit offset min-sum, and a word so short that everything saturates
SETTINGS = [(6, 2, 0.8125, 0), (5, 1, 1.0, 1), (3, 0, 1.0, 0)]
VARIANTS = [("f64", "stream"), ("f64", "fused"), ("f32", "stream"), ("f32", "fused"), ("f16", "stream")]  # (f16: streaming kernels only)
_CODE_CACHE = {}
GOLDEN_CODES = ("1200_3_6_rand_ldpc_1", "7_4_hamming")  # edge lists in tests/golden/codes_edges.npz
# ~12 columns, check 0 of degree 1 (an empty minimum: it sends floor(scale V) - offset), check 1 of degree 2, the others of degree 3 and 4; variable degrees 2 and 3
HAND_H = np.array([[1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                   [0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                   [1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0],
                   [0, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0],
                   [0, 0, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0],
                   [0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 1, 0],
                   [1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1],
                   [0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]])


def _code(name):
    from ldpc_decoders_amd import codes

    if name not in _CODE_CACHE:
        if name == "hand":
            g = O.Edges.from_dense(HAND_H)
        elif name in GOLDEN_CODES:
            g = golden_edges(name)
        else:  # a shipped code file that tests/golden holds no edge list of: the package's own loader (the reference's semantics)
            c = codes.load_parity_mtx(os.path.join(CODES_DIR, name + ".txt"))
            g = O.Edges(c.m, c.n, c.edge_chk, c.edge_var)
        _CODE_CACHE[name] = (g, codes.Code.from_edges(g.m, g.n, g.chk, g.var))
    return _CODE_CACHE[name]


def _handle(name, prec, backend, setting=None, alg="QMSA"):
    from ldpc_decoders_amd._device import DecoderHandle

    h = DecoderHandle(_code(name)[1], alg, prec, backend)
    if setting is not None:
        h.set_fixed_point(*setting)
    return h


def _inputs(name, channel, param, B, seed):
    """-> (y0 uint8 [B, n] or None, priors float32 [B, n]) of the all-zero word: fp32 values, what every precision is handed"""
    g = _code(name)[0]
    rng = np.random.RandomState(seed)
    if channel == "biawgn":
        y = -1 + rng.normal(0, np.sqrt(O.biawgn_noise_var(param)), (B, g.n))
        return None, O.biawgn_priors(y, param).astype(np.float32)
    y = (rng.random_sample((B, g.n)) < param).astype(np.int64)
    return y.astype(np.uint8), O.bsc_priors(y, param).astype(np.float32)


def _decode_soft(h, pri32, y0, max_iter, flags=0):
    """The fp32-valued priors in the decoder's input type -> (xhat, iters, soft as float64)."""
    import torch

    p = torch.from_numpy(np.ascontiguousarray(pri32.astype(np.float64 if h.precision == "f64" else np.float32))).cuda()
    keep = p.clone()
    y = None if y0 is None else torch.from_numpy(np.ascontiguousarray(y0)).cuda()
    x, it, soft = h.decode_soft_device(p, y, max_iter, flags=flags)
    assert torch.equal(p, keep), "the caller's priors were modified"
    return x.cpu().numpy(), it.cpu().numpy(), soft.cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------- 1, 2: the oracle, every precision and backend
CASES = [("1200_3_6_rand_ldpc_1", "biawgn", 1.5), ("1200_rho_x5_rand_ldpc_1", "biawgn", 2.0), ("512_3_6_rand_ldpc_1", "biawgn", 2.0),
         ("7_4_hamming", "bsc", 0.1), ("hand", "biawgn", 2.0)]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "q%d_k%d_%g_%d" % s)
@pytest.mark.parametrize("name,channel,param", CASES)
def test_bit_exact_against_the_oracle_in_every_precision_on_both_backends(name, channel, param, setting):
    """64 frames, max_iter 50: decisions, iteration counts and soft outputs (in levels) of the f64, f32 and f16 decoders on the streaming
    and the LDS backend are those of the CPU restatement -- hence identical to each other.  The hand-made H (a degree-1 and a degree-2
    check) and the 7-bit code run on the streaming kernels; last_stats() shows which backend really ran."""
    g = _code(name)[0]
    B, max_iter = 64, 50
    y0, pri = _inputs(name, channel, param, B, 21)
    bits, frac, scale, offset = setting
    xr, ir, sr, peak = Q.qmsa_decode(g, y0, pri, max_iter, bits, frac, scale, offset, np.float64)
    levels = Q.quantise(pri.astype(np.float64), bits, frac)
    print("%s %s: %d of %d frames at the cap, %d at iteration 0, %.1f %% of the levels saturated, peak |marginal| %d" % (
        name, setting, int((ir == max_iter).sum()), B, int((ir == 0).sum()), 100.0 * (np.abs(levels) == Q.vmax_of(bits)).mean(), peak))
    lds = name not in ("7_4_hamming", "hand")
    ran = set()
    for prec, backend in VARIANTS:
        if backend == "fused" and not lds:
            continue
        h = _handle(name, prec, backend, setting)
        assert h.fixed_point() == (bits, frac, scale, offset)
        x, it, soft = _decode_soft(h, pri, y0, max_iter)
        ran.add(h.last_stats()[0])
        where = (name, setting, prec, backend)
        assert h.last_stats()[0] == backend, where
        assert (it == ir).all(), (where, np.flatnonzero(it != ir)[:8], it[it != ir][:8], ir[it != ir][:8])
        assert (x == xr).all(), (where, np.flatnonzero((x != xr).any(axis=1))[:8])
        assert np.array_equal(soft, sr), (where, np.flatnonzero((soft != sr).any(axis=1))[:8])
    assert ran == ({"stream", "fused"} if lds else {"stream"})
    if name == "7_4_hamming":
        assert (ir == 0).any() and (ir > 0).any()  # the iteration-0 exit of the BSC and frames that sweep


def test_the_integer_statement_on_the_gpu_frames():
    """The all-integer ``//`` statement on two of the frames above: what a packed-integer kernel would be held to is what these kernels give."""
    name, setting = "512_3_6_rand_ldpc_1", (5, 1, 1.0, 1)
    g = _code(name)[0]
    _, pri = _inputs(name, "biawgn", 2.0, 64, 21)
    x, it, soft = _decode_soft(_handle(name, "f32", "fused", setting), pri, None, 50)
    levels = Q.quantise(pri.astype(np.float64), setting[0], setting[1]).astype(np.int64)
    for f in (0, 1):
        xi, ii, si = Q.qmsa_decode_int(g, None, levels[f], 50, setting[0], 64, setting[3])
        assert (xi == x[f]).all() and ii == it[f] and np.array_equal(si, soft[f].astype(np.int64))


# ---------------------------------------------------------------------------------------------- 3: no clamp can bind
def test_without_a_binding_clamp_it_is_min_sum():
    """bits 12 (V = 2047), k 0, scale 1, offset 0, integer priors |p| <= 15, six sweeps of the (3,6) code: |v2c| grows by v_{t+1} <= 15 + 2 v_t,
    i.e. <= 15 (2^7 - 1) = 1 905 < 2 047 after six -- nothing saturates, nothing is rounded, and the outputs are those of MSA in fp64 bit for
    bit, marginals included."""
    name = "1200_3_6_rand_ldpc_1"
    g = _code(name)[0]
    rng = np.random.RandomState(8)
    pri = np.clip(np.rint(rng.normal(2.0, 4.0, (64, g.n))), -15, 15).astype(np.float32)
    xm, im, sm = _decode_soft(_handle(name, "f64", "auto", None, "MSA"), pri, None, 6)
    assert np.abs(sm).max() <= 15 + 3 * 1905 and (im == 6).any()
    for prec, backend in VARIANTS:
        x, it, soft = _decode_soft(_handle(name, prec, backend, (12, 0, 1.0, 0)), pri, None, 6)
        assert (x == xm).all() and (it == im).all() and np.array_equal(soft, sm), (prec, backend)


# ---------------------------------------------------------------------------------------------- 4: quantiser edges
@pytest.mark.parametrize("name", ["1200_3_6_rand_ldpc_1", "hand"])
def test_quantiser_edges(name):
    """Priors at exact half-levels (ties go to even), beyond +-V and +-inf: the soft output after ONE sweep without the early exit is the
    oracle's, in every precision on both backends."""
    from ldpc_decoders_amd import _lib

    g = _code(name)[0]
    setting = (5, 1, 0.8125, 0)  # V = 15, a level is 0.5
    rng = np.random.RandomState(4)
    pri = (rng.randint(-40, 41, (64, g.n)) * 0.25).astype(np.float32)  # multiples of 1/4: every other one is a half-level; beyond +-7.5 saturates
    assert (pri * 2 % 1 == 0.5).any() and (np.abs(pri) > 7.5).any()
    pri[::3, ::5] = np.inf
    pri[1::3, 1::7] = -np.inf
    pri[:, 2] = -0.25  # rounds to level -0: must count as +0
    _, ir, sr, _ = Q.qmsa_decode(g, None, pri, 1, *setting, dtype=np.float64, early=False)
    assert (ir == 1).all() and np.isfinite(sr).all()
    for prec, backend in VARIANTS:
        if backend == "fused" and name == "hand":
            continue
        x, it, soft = _decode_soft(_handle(name, prec, backend, setting), pri, None, 1, flags=_lib.FLAG_NO_EARLY_EXIT)
        assert (it == 1).all() and np.array_equal(soft, sr), (prec, backend, np.flatnonzero((soft != sr).any(axis=1))[:8])
        assert (x == (sr < 0)).all()


# ---------------------------------------------------------------------------------------------- 5: simulate
@pytest.mark.parametrize("channel,param", [("biawgn", 2.0), ("bsc", 0.04)])
@pytest.mark.parametrize("prec,backend", VARIANTS)
def test_simulate_counters(prec, backend, channel, param):
    """ldpc_simulate of a QMSA decoder == ldpc_channel -> ldpc_decode -> count on the same frames (each precision on its own channel output),
    == the restatement on those priors; splitting the batch (1 + 1 233 + the rest) changes no counter."""
    import torch

    name, B, seed, stream, frame0, max_iter = "1200_3_6_rand_ldpc_1", 2048, 77, 2, 1000, 50
    setting = (6, 2, 0.8125, 0)
    g = _code(name)[0]
    h = _handle(name, prec, backend, setting)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    h.simulate(channel, param, 0, seed, stream, frame0, B, max_iter, cnt)
    torch.cuda.synchronize()
    assert h.last_stats()[0] == backend
    got = cnt.cpu().tolist()
    pri, y = h.channel_device(channel, param, 0, seed, stream, frame0, B)
    xh, it = h.decode_device(pri, y, max_iter)
    xh, it = xh.cpu().numpy(), it.cpu().numpy()
    assert got == [B, int(xh.any(axis=1).sum()), int(xh.sum()), int(it.sum())]
    xr, ir, _, _ = Q.qmsa_decode(g, None if y is None else y.cpu().numpy(), pri.cpu().numpy(), max_iter, *setting,
                                 dtype=np.float64 if prec == "f64" else np.float32)
    assert (xh == xr).all() and (it == ir).all()
    assert 0 < got[1] < B or channel == "bsc"
    parts = torch.zeros(4, dtype=torch.int64, device="cuda")
    for f0, nb in ((0, 1), (1, 1233), (1234, B - 1234)):
        h.simulate(channel, param, 0, seed, stream, frame0 + f0, nb, max_iter, parts)
    torch.cuda.synchronize()
    assert parts.cpu().tolist() == got


def test_simulate_random_codewords_and_a_bsc_llr_below_one_level():
    import torch

    name = "1200_3_6_rand_ldpc_1"
    h = _handle(name, "f32", "auto", (6, 2, 0.8125, 0))
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    h.simulate("biawgn", 2.0, -1, 5, 0, 0, 2048, 50, cnt)
    torch.cuda.synchronize()
    c = cnt.cpu().tolist()
    assert c[0] == 2048 and c[1] < 2048 // 4 and c[3] > 0
    # p = 0.49: |LLR| = 0.04 is level 0 at k = 2 -- the priors no longer carry the received word; the counters are still those of the composition
    g = _code(name)[0]
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    h.simulate("bsc", 0.49, 0, 5, 0, 0, 256, 3, cnt)
    pri, y = h.channel_device("bsc", 0.49, 0, 5, 0, 0, 256)
    xh, it = h.decode_device(pri, y, 3)
    xh, it = xh.cpu().numpy(), it.cpu().numpy()
    assert cnt.cpu().tolist() == [256, int(xh.any(axis=1).sum()), int(xh.sum()), int(it.sum())]
    xr, ir, _, _ = Q.qmsa_decode(g, y.cpu().numpy(), pri.cpu().numpy(), 3, 6, 2, 0.8125, 0, np.float32)
    assert (xh == xr).all() and (it == ir).all()


# ---------------------------------------------------------------------------------------------- 6: parameters, refusals
def test_parameters_and_refusals():
    import torch
    from ldpc_decoders_amd import _lib, bec
    from ldpc_decoders_amd._device import DecoderHandle

    lib = _lib.load()
    E_ARG, E_UNSUPPORTED = -1, -4  # include/ldpc_hip.h
    name = "1200_3_6_rand_ldpc_1"
    g, code = _code(name)
    _, pri = _inputs(name, "biawgn", 2.0, 64, 9)

    def last_error():
        return (lib.ldpc_last_error() or b"").decode()

    for prec, backend in VARIANTS:
        h = DecoderHandle(code, "QMSA", prec, backend)
        assert h.fixed_point() == (6, 2, 0.8125, 0)  # the state after create
        # a change between two calls takes effect on the next call; get returns it
        outs = {}
        for setting in ((6, 2, 0.8125, 0), (3, 0, 1.0, 0), (6, 2, 0.8125, 0)):
            h.set_fixed_point(*setting)
            assert h.fixed_point() == setting
            x, it, soft = _decode_soft(h, pri, None, 20)
            xr, ir, sr, _ = Q.qmsa_decode(g, None, pri, 20, *setting)
            assert (x == xr).all() and (it == ir).all() and np.array_equal(soft, sr), (prec, backend, setting)
            outs.setdefault(setting, []).append(soft)
        assert np.array_equal(*outs[(6, 2, 0.8125, 0)]) and not np.array_equal(outs[(6, 2, 0.8125, 0)][0], outs[(3, 0, 1.0, 0)][0])
        # out of range: refused by the library too, state untouched
        for bad in ((1, 2, 0.8125, 0), (13, 2, 0.8125, 0), (6, 9, 0.8125, 0), (6, -9, 0.8125, 0), (6, 2, 0.8, 0), (6, 2, 0.0, 0), (6, 2, 1.02, 0),
                    (6, 2, float("nan"), 0), (6, 2, 0.8125, -1)):
            rc = lib.ldpc_decoder_set_fixed_point(h.h, bad[0], bad[1], ctypes.c_double(bad[2]), bad[3])
            assert rc == E_ARG and "scale" in last_error(), (bad, rc)
        assert h.fixed_point() == (6, 2, 0.8125, 0)
        assert lib.ldpc_decoder_set_correction(h.h, ctypes.c_double(0.8), ctypes.c_double(0.0)) == E_ARG and "NMSA" in last_error()
        # the prior grid would add nothing: refused on every entry point
        p = torch.from_numpy(pri.astype(np.float64 if prec == "f64" else np.float32)).cuda()
        xh = torch.empty((64, g.n), dtype=torch.uint8, device="cuda")
        it = torch.empty(64, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        grid = _lib.flag_prior_grid(4)
        rc = lib.ldpc_decode(h.h, p.data_ptr(), None, 64, 10, grid, xh.data_ptr(), it.data_ptr(), st)
        assert rc == E_UNSUPPORTED and "prior grid" in last_error() and "QMSA" in last_error(), (prec, backend, rc, last_error())
        rc = lib.ldpc_simulate(h.h, _lib.CHANNEL["biawgn"], 2.0, 0, 1, 0, 0, 64, 10, grid, 0, cnt.data_ptr(), st)
        assert rc == E_UNSUPPORTED and "prior grid" in last_error()
        assert int(cnt.sum()) == 0
    hn = DecoderHandle(code, "NMSA", "f32")
    assert lib.ldpc_decoder_set_fixed_point(hn.h, 6, 2, ctypes.c_double(0.8125), 0) == E_ARG and "QMSA" in last_error()
    b, k, o, s = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
    assert lib.ldpc_decoder_get_fixed_point(hn.h, ctypes.byref(b), ctypes.byref(k), ctypes.byref(s), ctypes.byref(o)) == E_ARG
    assert lib.ldpc_abi_version() == 4
    with pytest.raises(NotImplementedError):
        bec.QMSA(0.4, code, max_iter=10)
    # the kernel a QMSA decoder launches is the sibling of the min-sum one, and the device is as usable as before
    hm = DecoderHandle(code, "MSA", "f32")
    hq = DecoderHandle(code, "QMSA", "f32")
    for sim in (False, True):
        assert hq.kernel_name(sim) == hm.kernel_name(sim).replace("<0, ", "<4, ", 1) and hm.fused_info() == hq.fused_info()
    x, it = hm.decode_device(torch.from_numpy(pri).cuda(), None, 50)
    torch.cuda.synchronize()
    assert (it.cpu().numpy() > 0).all()


def test_python_classes():
    """bpa.QMSA / biawgn.QMSA: host buffers, one frame per call and batches, the oracle's decisions."""
    from ldpc_decoders_amd import biawgn, bpa

    name = "512_3_6_rand_ldpc_1"
    g, code = _code(name)
    _, pri = _inputs(name, "biawgn", 2.0, 64, 3)
    xr, ir, _, _ = Q.qmsa_decode(g, None, pri, 30, 5, 1, 1.0, 1)
    for prec in ("f64", "f32"):
        dec = bpa.QMSA(code, max_iter=30, precision=prec, msa_bits=5, msa_frac_bits=1, msa_scale=1, msa_offset=1.0)
        assert dec.handle.fixed_point() == (5, 1, 1.0, 1)
        x, it = dec.decode_batch(None, pri.astype(np.float64))
        assert (x == xr).all() and (it == ir).all()
        one = dec.decode(pri[3] * -0.5 + 0.25, pri[3])  # (a real-valued observation: no iteration-0 word)
        assert (np.asarray(one) == xr[3]).all() and int(dec.last_iters[0]) == int(ir[3])
    wrapped = biawgn.QMSA(2.0, code, max_iter=30)
    assert wrapped.dec.handle.fixed_point() == (6, 2, 0.8125, 0)


# ---------------------------------------------------------------------------------------------- 7: command line
def test_command_line(tmp_path, monkeypatch):
    from ldpc_decoders_amd import codes, main

    monkeypatch.setenv(codes.file_codes_dir_string, CODES_DIR)
    r = main.main(["biawgn", "1200_3_6_rand_ldpc_1", "QMSA", "--msa-bits", "5", "--msa-frac-bits", "1", "--msa-scale", "1", "--msa-offset", "1",
                   "--params", "2.0", "--max-iter", "50", "--min-wec", "30", "--batch", "16384", "--data_dir", str(tmp_path), "--console", "--seed", "11"])
    with open(os.path.join(str(tmp_path), "biawgn-1200_3_6_rand_ldpc_1-QMSA-0-30-50-5-1-1.0-1.0.json")) as fp:
        got = json.load(fp)
    # the reference's keys: the id keys (src/main.py:14) with this decoder's four behind max_iter, then tot wec wer bec ber (src/main.py:29)
    assert list(got) == ["channel", "code", "decoder", "codeword", "min_wec", "max_iter", "msa_bits", "msa_frac_bits", "msa_scale", "msa_offset",
                         "tot", "wec", "wer", "bec", "ber"]
    assert (got["decoder"], got["msa_bits"], got["msa_frac_bits"], got["msa_scale"], got["msa_offset"]) == ("QMSA", 5, 1, 1.0, 1.0)
    print("5-bit offset min-sum at 2.0 dB: WER %s over %s frames" % (got["wer"]["2.0"], got["tot"]["2.0"]))
    # (CPU sample of this point: 14 word errors in 1 024 frames; plain min-sum 160)
    assert got["wec"]["2.0"] >= 30 and got["tot"]["2.0"] >= 16384 and 0 < got["wer"]["2.0"] < 0.08 and r[2.0]["wec"] == got["wec"]["2.0"]
    # the reference-exact mode (host noise, sequential rule, run_point_exact; decoder on the GPU): one small point
    r = main.main(["biawgn", "1200_3_6_rand_ldpc_1", "QMSA", "--params", "1.0", "--max-iter", "50", "--min-wec", "3", "--exact", "--np-seed", "1234",
                   "--data_dir", str(tmp_path / "exact"), "--console"])
    assert r[1.0]["wec"] >= 3 and r[1.0]["tot"] >= 3
    with pytest.raises(SystemExit, match="--prior-grid"):
        main.main(["biawgn", "1200_3_6_rand_ldpc_1", "QMSA", "--params", "2.0", "--prior-grid", "4", "--data_dir", str(tmp_path / "grid"), "--console"])

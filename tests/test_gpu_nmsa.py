"""Corrected (normalised / offset) min-sum on the GPU (LDPC_ALG_NMSA, bpa.NMSA): identity with min-sum at (1, 0), bit parity with the CPU
restatement (tests/nmsa_oracle.py) on every frame, same backend / shape / plan as min-sum for every shipped code, the Monte-Carlo entry
points, what the correction is worth, the fp16 storage mode, the refusals and the command line."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

import bp_oracle as O
import nmsa_oracle as N
from helpers import CODES_DIR, golden_edges

pytestmark = pytest.mark.gpu

CODES = ["1200_3_6_rand_ldpc_1", "1200_rho_x5_rand_ldpc_5", "margulis", "7_4_hamming"]
CORRECTIONS = [(0.8125, 0.0), (0.75, 0.0), (1.0, 0.5), (0.875, 0.125)]
ALL_NAMES = sorted(os.path.splitext(os.path.basename(f))[0] for f in glob.glob(os.path.join(CODES_DIR, "*.txt")))
_CODE_CACHE = {}


def _code(name):
    from ldpc_decoders_amd.codes import Code

    if name not in _CODE_CACHE:
        g = golden_edges(name)
        _CODE_CACHE[name] = (g, Code.from_edges(g.m, g.n, g.chk, g.var))
    return _CODE_CACHE[name]


def _handle(name, alg, prec, backend="auto", corr=None):
    from ldpc_decoders_amd._device import DecoderHandle

    h = DecoderHandle(_code(name)[1], alg, prec, backend)
    if corr is not None:
        h.set_correction(*corr)
    return h


def _inputs(name, channel, param, B, seed):
    """-> (y0 uint8 [B, n] or None, priors float64 [B, n]) of the all-zero word"""
    g = _code(name)[0]
    rng = np.random.RandomState(seed)
    if channel == "biawgn":
        y = -1 + rng.normal(0, np.sqrt(O.biawgn_noise_var(param)), (B, g.n))
        return None, O.biawgn_priors(y, param)
    y = (rng.random_sample((B, g.n)) < param).astype(np.int64)
    return y.astype(np.uint8), O.bsc_priors(y, param)


def _decode_soft(h, pri, y0, max_iter, dt):
    import torch

    p = torch.from_numpy(np.ascontiguousarray(pri.astype(dt))).cuda()
    y = None if y0 is None else torch.from_numpy(np.ascontiguousarray(y0)).cuda()
    x, it, soft = h.decode_soft_device(p, y, max_iter)
    return x.cpu().numpy(), it.cpu().numpy(), soft.cpu().numpy()


# ---------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("backend", ["stream", "auto"])
@pytest.mark.parametrize("prec,dt", [("f64", np.float64), ("f32", np.float32)])
@pytest.mark.parametrize("name", CODES)
def test_identity_correction_is_min_sum(name, prec, dt, backend):
    """scale 1, offset 0 (the state after create): decisions, iteration counts and soft outputs of MSA, 2 048 frames (4 096 of the 7-bit
    code) at an SNR where some converge within the cap and some do not."""
    B = 4096 if name == "7_4_hamming" else 2048
    y0, pri = _inputs(name, "biawgn", 1.5 if name != "7_4_hamming" else 2.0, B, 3)
    hm, hn = _handle(name, "MSA", prec, backend), _handle(name, "NMSA", prec, backend)
    assert hn.correction() == (1.0, 0.0)
    xm, im, sm = _decode_soft(hm, pri, y0, 25, dt)
    xn, inn, sn = _decode_soft(hn, pri, y0, 25, dt)
    assert hm.last_stats()[0] == hn.last_stats()[0]
    conv = int((im < 25).sum())
    print("%s %s %s: %d of %d frames left before the cap" % (name, prec, backend, conv, B))
    assert 0 < conv and (name == "7_4_hamming" or conv < B)
    assert (xm == xn).all() and (im == inn).all() and np.array_equal(sm, sn)
    # the Python classes, host buffers
    from ldpc_decoders_amd import bpa

    code = _code(name)[1]
    a = bpa.MSA(code, max_iter=25, precision=prec, backend=backend).decode_batch(None, pri[:256])
    b = bpa.NMSA(code, max_iter=25, precision=prec, backend=backend, msa_scale=1.0, msa_offset=0.0).decode_batch(None, pri[:256])
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[0] == xm[:256]).all()


# ---------------------------------------------------------------------------------------------- parity with the restatement
@pytest.mark.parametrize("prec,dt", [("f64", np.float64), ("f32", np.float32)])
@pytest.mark.parametrize("name", CODES)
def test_parity_with_the_cpu_restatement(name, prec, dt):
    """Every frame: decisions and iteration counts bit-identical, soft outputs equal by value (rtol 0; -0.0 == 0.0) -- both backends, four
    corrections, BI-AWGN at 1.5 and 2.0 dB and the BSC at p = 0.05 with the iteration-0 rule.  No allow-list: the rule is compare /
    multiply / subtract only."""
    g = _code(name)[0]
    B = {"7_4_hamming": 1024, "margulis": 96}.get(name, 192)
    max_iter = 25
    handles = {bk: _handle(name, "NMSA", prec, bk) for bk in ("stream", "auto")}
    for ci, (channel, param) in enumerate((("biawgn", 1.5), ("biawgn", 2.0), ("bsc", 0.05))):
        y0, pri = _inputs(name, channel, param, B, 40 + ci)
        pri = pri.astype(dt)
        for scale, offset in CORRECTIONS:
            xr, ir, sr = N.nmsa_decode(g, y0, pri, max_iter, scale, offset, dt)
            for bk, h in handles.items():
                h.set_correction(scale, offset)
                x, it, soft = _decode_soft(h, pri, y0, max_iter, dt)
                where = (name, prec, bk, channel, param, scale, offset)
                assert (it == ir).all(), (where, np.flatnonzero(it != ir)[:8])
                assert (x == xr).all(), (where, np.flatnonzero((x != xr).any(axis=1))[:8])
                assert soft.dtype == sr.dtype and np.array_equal(soft, sr), (where, np.flatnonzero((soft != sr).any(axis=1))[:8])
    assert handles["stream"].last_stats()[0] == "stream" and (name == "7_4_hamming" or handles["auto"].last_stats()[0] == "fused")


# ---------------------------------------------------------------------------------------------- backend, shape, plan
@pytest.mark.parametrize("name", ALL_NAMES)
def test_same_backend_shape_and_plan_as_min_sum(name, monkeypatch, tmp_path):
    """27 shipped code files x fp32 / fp64: an NMSA decoder runs where the MSA decoder runs -- same backend, same kernel shape (only the
    algorithm argument of the kernel name differs), the same stored layout plan (nothing annealed at construction)."""
    import torch
    from ldpc_decoders_amd import codes
    from ldpc_decoders_amd._device import DecoderHandle

    assert len(ALL_NAMES) == 27
    monkeypatch.setenv("LDPC_FUSED_PLAN_SAVE", "none")
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "empty"))
    monkeypatch.setenv("LDPC_FUSED_PLAN_MOVES", "1000")  # a plan that is not in the store would show up with hundreds of conflict cycles
    code = codes.load_parity_mtx(os.path.join(CODES_DIR, name + ".txt"))
    limit = 60 if name.startswith("512_") or "rho" in name else 40  # (tests/test_gpu_plan_store.py)
    rng = np.random.RandomState(1)
    pri64 = O.biawgn_priors(-1 + rng.normal(0, np.sqrt(O.biawgn_noise_var(2.0)), (64, code.n)), 2.0)
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        hm, hn = DecoderHandle(code, "MSA", prec), DecoderHandle(code, "NMSA", prec)
        fm, fn = hm.fused_info(), hn.fused_info()
        assert fm == fn and fn["waves_per_frame"] > 0, (name, prec, fm, fn)
        assert fn["conflict_cycles_planned"] <= limit < fn["conflict_cycles_identity"], (name, prec, fn)
        for sim in (False, True):
            km, kn = hm.kernel_name(sim), hn.kernel_name(sim)
            assert km and "<0, " in km and kn == km.replace("<0, ", "<3, ", 1), (km, kn)
        pri = torch.from_numpy(pri64).to(dt).cuda()
        hm.decode_device(pri, None, 10), hn.decode_device(pri, None, 10)
        assert hm.last_stats()[0] == hn.last_stats()[0] == "fused"


# ---------------------------------------------------------------------------------------------- Monte-Carlo entry points
@pytest.mark.parametrize("backend", ["auto", "stream"])
@pytest.mark.parametrize("prec,dt", [("f32", np.float32), ("f64", np.float64)])
def test_simulate_counters(prec, dt, backend):
    """ldpc_simulate / ldpc_simulate_rounds of an NMSA decoder == ldpc_channel -> ldpc_decode -> ldpc_count_errors on the same seed == the
    restatement on those priors; two half-rounds add up to the round; a change of the correction between two calls takes effect."""
    import torch
    from ldpc_decoders_amd import _lib

    name, B, snr, seed, stream, frame0, max_iter = "1200_3_6_rand_ldpc_1", 4096, 2.0, 77, 2, 1000, 50
    g = _code(name)[0]
    h = _handle(name, "NMSA", prec, backend, (0.8125, 0.0))
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    h.simulate("biawgn", snr, 0, seed, stream, frame0, B, max_iter, cnt)
    torch.cuda.synchronize()
    assert h.last_stats()[0] == ("fused" if backend == "auto" else "stream")
    got = cnt.cpu().tolist()
    # (a) the composition
    pri, _ = h.channel_device("biawgn", snr, 0, seed, stream, frame0, B)
    xh, it = h.decode_device(pri, None, max_iter)
    ref = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().ldpc_count_errors(xh.data_ptr(), None, 0, it.data_ptr(), B, g.n, 0, ref.data_ptr(), st))
    torch.cuda.synchronize()
    assert got == ref.cpu().tolist()
    # (b) the restatement on those priors
    xr, ir, _ = N.nmsa_decode(g, None, pri.cpu().numpy(), max_iter, 0.8125, 0.0, dt)
    assert (xh.cpu().numpy() == xr).all() and (it.cpu().numpy() == ir).all()
    assert got == [B, int(xr.any(axis=1).sum()), int(xr.sum()), int(ir.sum())]
    # sharding invariance, through ldpc_simulate_rounds (two rounds of half the frames)
    rows = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    h.simulate_rounds("biawgn", snr, 0, seed, stream, frame0, B // 2, 2, B // 2, max_iter, rows)
    torch.cuda.synchronize()
    assert rows.sum(dim=0).cpu().tolist() == got
    # a change of the correction takes effect from the next call: (1, 0) is min-sum
    h.set_correction(1.0, 0.0)
    c1 = torch.zeros(4, dtype=torch.int64, device="cuda")
    h.simulate("biawgn", snr, 0, seed, stream, frame0, B, max_iter, c1)
    cm = torch.zeros(4, dtype=torch.int64, device="cuda")
    _handle(name, "MSA", prec, backend).simulate("biawgn", snr, 0, seed, stream, frame0, B, max_iter, cm)
    torch.cuda.synchronize()
    assert c1.cpu().tolist() == cm.cpu().tolist() and c1.cpu().tolist() != got
    h.set_correction(0.8125, 0.0)
    c2 = torch.zeros(4, dtype=torch.int64, device="cuda")
    h.simulate("biawgn", snr, 0, seed, stream, frame0, B, max_iter, c2)
    torch.cuda.synchronize()
    assert c2.cpu().tolist() == got


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_the_point_of_it(prec):
    """65 536 frames, 2.0 dB, 50 sweeps, device noise, config 2: the corrected rule has fewer than a quarter of min-sum's word errors AND
    executes fewer sweeps.  (CPU sample of the same operating point: 8 against 160 word errors in 1 024 frames, 11.2 against 19.9 sweeps.)"""
    import torch

    name, B = "1200_3_6_rand_ldpc_1", 65536
    out = {}
    for alg, corr in (("MSA", None), ("NMSA", (0.8125, 0.0))):
        h = _handle(name, alg, prec, "auto", corr)
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        h.simulate("biawgn", 2.0, 0, 2024, 0, 0, B, 50, cnt)
        torch.cuda.synchronize()
        out[alg] = cnt.cpu().tolist()
        assert h.last_stats()[0] == "fused" and out[alg][0] == B
    print("%s: tot, wec, bec, iter_sum  MSA %s  NMSA(0.8125) %s" % (prec, out["MSA"], out["NMSA"]))
    assert out["NMSA"][1] * 4 < out["MSA"][1]
    assert out["NMSA"][3] < out["MSA"][3]


# ---------------------------------------------------------------------------------------------- fp16 storage
@pytest.mark.parametrize("name,B", [("1200_3_6_rand_ldpc_1", 300), ("1200_rho_x5_rand_ldpc_5", 130)])
def test_fp16_storage_within_its_stated_tolerance(name, B):
    """DESIGN section 5's bound for the mode, 1e-2 (1 + |fp32 value|), on the marginals after 1, 2, 3 sweeps against the fp32 NMSA decoder
    on the streaming kernels (the correction is applied in fp32, before the message is rounded to half)."""
    import torch
    from ldpc_decoders_amd import _lib

    _, pri = _inputs(name, "biawgn", 2.0, B, 5)
    pri = torch.from_numpy(pri.astype(np.float32)).cuda()
    h16, h32 = _handle(name, "NMSA", "f16", "auto", (0.8125, 0.0)), _handle(name, "NMSA", "f32", "stream", (0.8125, 0.0))
    for sweeps in (1, 2, 3):
        x16, i16, m16 = h16.decode_soft_device(pri, None, sweeps, flags=_lib.FLAG_NO_EARLY_EXIT)
        x32, i32, m32 = h32.decode_soft_device(pri, None, sweeps, flags=_lib.FLAG_NO_EARLY_EXIT)
        assert h16.last_stats()[0] == "stream" and (i16 == sweeps).all() and (i32 == sweeps).all()
        m16, m32 = m16.cpu().numpy().astype(np.float64), m32.cpu().numpy().astype(np.float64)
        err = np.abs(m16 - m32) / (1 + np.abs(m32))
        print("%s sweep %d: max error %.2e of the bound 1e-2" % (name, sweeps, err.max()))
        assert np.isfinite(m32).all() and err.max() <= 1e-2
    # and the mode is not min-sum in disguise: the corrected marginals differ from the plain ones
    _, _, plain = _handle(name, "MSA", "f16").decode_soft_device(pri, None, 3, flags=_lib.FLAG_NO_EARLY_EXIT)
    assert np.abs(plain.cpu().numpy() - m16).max() > 0.1


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_device_usable():
    """Every refusal happens on the host before any launch, carries a message, and a min-sum decode afterwards succeeds."""
    import torch
    from ldpc_decoders_amd import _lib, bec
    from ldpc_decoders_amd._device import DecoderHandle

    lib = _lib.load()
    E_ARG, E_UNSUPPORTED = -1, -4  # include/ldpc_hip.h
    name = "1200_3_6_rand_ldpc_1"
    g, code = _code(name)
    _, pri64 = _inputs(name, "biawgn", 2.0, 64, 9)

    def last_error():
        return (lib.ldpc_last_error() or b"").decode()

    hm = DecoderHandle(code, "MSA", "f32")
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        for backend in ("auto", "stream"):
            h = DecoderHandle(code, "NMSA", prec, backend)
            pri = torch.from_numpy(pri64).to(dt).cuda()
            xh = torch.empty((64, g.n), dtype=torch.uint8, device="cuda")
            it = torch.empty(64, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            grid = _lib.flag_prior_grid(4)
            rc = lib.ldpc_decode(h.h, pri.data_ptr(), None, 64, 10, grid, xh.data_ptr(), it.data_ptr(), st)
            msg = last_error()
            assert rc == E_UNSUPPORTED and "prior grid" in msg and "NMSA" in msg, (prec, backend, rc, msg)
            rc = lib.ldpc_simulate(h.h, _lib.CHANNEL["biawgn"], 2.0, 0, 1, 0, 0, 64, 10, grid, 0, cnt.data_ptr(), st)
            assert rc == E_UNSUPPORTED and "prior grid" in last_error()
            # the erasure channel pairs with the erasure decoder only, as for MSA
            rc = lib.ldpc_simulate(h.h, _lib.CHANNEL["bec"], 0.4, 0, 1, 0, 0, 64, 10, 0, 0, cnt.data_ptr(), st)
            rc_m = lib.ldpc_simulate(hm.h, _lib.CHANNEL["bec"], 0.4, 0, 1, 0, 0, 64, 10, 0, 0, cnt.data_ptr(), st)
            assert rc == rc_m == E_ARG and "erasure" in last_error()
            for scale, offset in ((0.0, 0.0), (-1.0, 0.0), (1.5, 0.0), (float("nan"), 0.0), (0.8, -0.25), (0.8, float("inf")), (0.8, float("nan"))):
                rc = lib.ldpc_decoder_set_correction(h.h, ctypes.c_double(scale), ctypes.c_double(offset))
                assert rc == E_ARG and "scale" in last_error(), (scale, offset, rc)
                with pytest.raises(ValueError):
                    h.set_correction(scale, offset)
            assert h.correction() == (1.0, 0.0)  # untouched by the refused calls
            assert int(cnt.sum()) == 0
    # the header's codes, and a setter / getter on a decoder of another algorithm
    with open(os.path.join(os.path.dirname(CODES_DIR), "..", "..", "include", "ldpc_hip.h")) as fp:
        assert "LDPC_E_ARG = -1" in fp.read()
    assert lib.ldpc_decoder_set_correction(hm.h, ctypes.c_double(0.8), ctypes.c_double(0.0)) == E_ARG and "NMSA" in last_error()
    s, o = ctypes.c_double(0), ctypes.c_double(0)
    assert lib.ldpc_decoder_get_correction(hm.h, ctypes.byref(s), ctypes.byref(o)) == E_ARG
    assert lib.ldpc_abi_version() == 4
    with pytest.raises(NotImplementedError):
        bec.NMSA(0.4, code, max_iter=10)
    # the device is as usable as before
    pri = torch.from_numpy(pri64).float().cuda()
    x, it = hm.decode_device(pri, None, 50)
    torch.cuda.synchronize()
    assert (it.cpu().numpy() > 0).all() and x.shape == (64, g.n)


# ---------------------------------------------------------------------------------------------- command line
def test_command_line(tmp_path, monkeypatch):
    from ldpc_decoders_amd import codes, main

    monkeypatch.setenv(codes.file_codes_dir_string, CODES_DIR)
    common = ["--params", "2.0", "--max-iter", "50", "--min-wec", "50", "--data_dir", str(tmp_path), "--console", "--seed", "11", "--batch", "8192"]
    main.main(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA"] + common + ["--msa-scale", "0.8125"])
    main.main(["biawgn", "1200_3_6_rand_ldpc_1", "MSA"] + common)
    with open(os.path.join(str(tmp_path), "biawgn-1200_3_6_rand_ldpc_1-NMSA-0-50-50-0.8125-0.0.json")) as fp:
        got = json.load(fp)
    with open(os.path.join(str(tmp_path), "biawgn-1200_3_6_rand_ldpc_1-MSA-0-50-50.json")) as fp:
        ref = json.load(fp)
    assert [k for k in got if k not in ("msa_scale", "msa_offset")] == list(ref)
    assert list(got)[:8] == ["channel", "code", "decoder", "codeword", "min_wec", "max_iter", "msa_scale", "msa_offset"]
    assert (got["decoder"], got["msa_scale"], got["msa_offset"]) == ("NMSA", 0.8125, 0.0)
    print("WER at 2.0 dB: NMSA %s (%s frames), MSA %s (%s frames)" % (got["wer"]["2.0"], got["tot"]["2.0"], ref["wer"]["2.0"], ref["tot"]["2.0"]))
    assert got["wec"]["2.0"] >= 50 and 0 < got["wer"]["2.0"] < ref["wer"]["2.0"]
    # random codewords on the device, and the reference-exact mode (host noise, sequential rule, decoder on the GPU)
    r = main.main(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA", "--params", "1.5", "--max-iter", "50", "--min-wec", "20", "--codeword", "-1",
                   "--data_dir", str(tmp_path / "cw"), "--console", "--batch", "2048"])
    assert r[1.5]["wec"] >= 20 and r[1.5]["tot"] >= 2048
    r = main.main(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA", "--params", "1.0", "--max-iter", "50", "--min-wec", "5", "--exact", "--np-seed", "1234",
                   "--data_dir", str(tmp_path / "exact"), "--console"])
    assert r[1.0]["wec"] >= 5 and r[1.0]["tot"] >= 5
    with pytest.raises(SystemExit, match="--prior-grid"):
        main.main(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA", "--params", "2.0", "--prior-grid", "4", "--data_dir", str(tmp_path / "grid"), "--console"])

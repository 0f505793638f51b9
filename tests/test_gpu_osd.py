"""Ordered-statistics post-processing (csrc/ldpc_osd.hip): bit-exact against the numpy statement of osd_oracle.py, its properties on a
large batch, word errors against plain BP on the same frames, batching, refusals and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import osd_oracle as OSD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, STREAM = 0x0D5EED1200, 2
SCALE = 0.8125


def _code(name):
    from ldpc_decoders_amd import codes

    return codes.get_code(name)


def _handles(code, precision):
    from ldpc_decoders_amd._device import DecoderHandle, OsdHandle

    bp = DecoderHandle(code, "NMSA", precision)
    bp.set_correction(SCALE, 0.0)
    return bp, OsdHandle(bp)


def _syndrome_dev(code, x):
    """x: CUDA uint8 [B, n] -> CUDA int [B] = number of unsatisfied checks."""
    import torch

    chk = torch.from_numpy(code.edge_chk.astype(np.int64)).cuda()
    var = torch.from_numpy(code.edge_var.astype(np.int64)).cuda()
    s = torch.zeros((x.shape[0], code.m), dtype=torch.int32, device=x.device)
    s.index_add_(1, chk, x[:, var].int())
    return (s & 1).sum(dim=1)


def _unpack_dev(bits, n):
    import torch

    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits[:, :, None] >> sh) & 1).reshape(bits.shape[0], -1)[:, :n].to(torch.uint8)


CASES = [("512_3_6_rand_ldpc_1", 2.0, 20), ("1200_3_6_rand_ldpc_1", 1.5, 50), ("1200_rho_x5_rand_ldpc_10", 1.5, 50), ("12_3_4_ldpc", 1.5, 0)]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name,snr,sweeps", CASES)
def test_bit_exact_against_the_numpy_statement(name, snr, sweeps, precision):
    """512 frames of device BI-AWGN noise on encoder words through NMSA (post = its soft output; the n = 12 code: post = prior), plus
    synthetic rows: all post = 0 (alone, and with one negative entry so that the frame is listed), BSC priors after one sweep (massive
    ties), a few +inf, a NaN.  Word, pick and cost (== on the doubles) for every listed frame of the n = 512 case, up to 16 evenly spaced
    listed frames of the others and every synthetic row; pass-through frames in full."""
    import torch

    code = _code(name)
    n, H = code.n, code.parity_mtx.astype(np.uint8)
    bp, osd = _handles(code, precision)
    B = 512
    sent = code.encoder().handle().encode_random(SEED, STREAM, 0, B)
    pri, _ = bp.channel_sent_device("biawgn", snr, sent, SEED, STREAM, 0)
    post = bp.decode_soft_device(pri, None, sweeps)[2] if sweeps else pri.clone()
    # synthetic rows
    bsc_pri, _ = bp.channel_device("bsc", 0.06, 0, SEED, STREAM, 5000, 6)
    bsc_post = bp.decode_soft_device(bsc_pri, None, 1, flags=1)[2]  # exactly one sweep: a handful of distinct magnitudes
    zero = torch.zeros_like(pri[:2])
    zero[1, n // 3] = -1.0  # one negative entry: no codeword, every other key ties at 0
    failed = (_syndrome_dev(code, (post < 0).to(torch.uint8)) != 0).nonzero().flatten()[:3]  # three frames BP left without a codeword
    odd_post, odd_pri = post[failed].clone(), pri[failed].clone()
    odd_post[0, [1, n // 2, n - 1]] = float("inf")
    odd_pri[1, [0, n - 2]] = float("inf")
    odd_pri[1, 3] = -float("inf")
    odd_post[2, n // 4] = float("nan")
    odd_pri[2, n // 5] = float("nan")
    post_all = torch.cat([post, zero, bsc_post, odd_post]).contiguous()
    pri_all = torch.cat([pri, pri[:2], bsc_pri, odd_pri]).contiguous()
    po, pr = post_all.cpu().numpy(), pri_all.cpu().numpy()
    h = OSD.hard(po)
    listed = np.flatnonzero(((h.astype(np.int64) @ H.T.astype(np.int64)) % 2).any(axis=1))
    passed = np.setdiff1d(np.arange(len(po)), listed)
    print("%s %s: %d of %d channel frames listed, %d synthetic rows listed" % (name, precision, (listed < B).sum(), B, (listed >= B).sum()))
    assert (listed < B).sum() >= 8, "the case must exercise the solver"
    real = listed[listed < B]
    check = real if n == 512 else real[np.linspace(0, len(real) - 1, min(16, len(real))).astype(int)]
    check = np.concatenate([check, listed[listed >= B]])
    elim = {f: OSD.eliminate(H, po[f]) for f in check}
    for order, depth in ((0, 0), (1, 64), (1, 10 ** 6)):
        bits, pick, cost = osd.solve(post_all, pri_all, order, depth)
        x, pk, co = _unpack_dev(bits, n).cpu().numpy(), pick.cpu().numpy(), cost.cpu().numpy()
        assert (x[passed] == h[passed]).all() and (pk[passed] == -1).all() and (co[passed] == -1.0).all()
        assert int(_syndrome_dev(code, _unpack_dev(bits, n)).max()) == 0
        for f in check:
            want_x, want_t, want_c = OSD.osd_frame(H, po[f], pr[f], order, depth, elim=elim[f])
            assert pk[f] == want_t and co[f] == want_c and (x[f] == want_x).all(), (name, precision, order, depth, int(f), pk[f], want_t, co[f], want_c)


def test_properties_on_a_large_batch():
    import torch

    code = _code("512_3_6_rand_ldpc_1")
    n, B = code.n, 4096
    bp, osd = _handles(code, "f32")
    pri, _ = bp.channel_device("biawgn", 2.0, 0, SEED, STREAM, 0, B)
    xbp, _, post = bp.decode_soft_device(pri, None, 20)
    hard = (post < 0).to(torch.uint8)
    ok = _syndrome_dev(code, hard) == 0
    b0, p0, c0 = osd.solve(post, pri, 0, 64)
    b1, p1, c1 = osd.solve(post, pri, 1, 64)
    bz, pz, cz = osd.solve(post, pri, 1, 0)
    assert int((~ok).sum()) >= 100
    for bits, pick in ((b0, p0), (b1, p1)):
        x = _unpack_dev(bits, n)
        assert int(_syndrome_dev(code, x).max()) == 0
        assert torch.equal(pick == -1, ok) and torch.equal(x[ok], hard[ok])
    assert torch.equal(hard[ok], xbp[ok])  # what BP called a codeword is what the post-processor leaves alone
    assert bool((p0[~ok] == 0).all())
    assert int(p1[~ok].min()) >= 0 and int(p1.max()) <= min(64, n - code.encoder().rank)
    assert bool((c1 <= c0).all()) and bool((c1[~ok] >= 0).all())
    assert int((c1 < c0).sum()) > 0  # order 1 does find cheaper words
    assert torch.equal(bz, b0) and torch.equal(pz, p0) and torch.equal(cz, c0)


def _count(lib, xhat, sent, iters, n, bins, counters):
    import torch

    st = torch.cuda.current_stream().cuda_stream
    if sent is None:
        rc = lib.ldpc_count_errors(xhat.data_ptr(), None, 0, iters.data_ptr(), xhat.shape[0], n, bins, counters.data_ptr(), st)
    else:
        rc = lib.ldpc_count_errors_words(xhat.data_ptr(), sent.data_ptr(), iters.data_ptr(), xhat.shape[0], n, bins, counters.data_ptr(), st)
    assert rc == 0


@pytest.mark.parametrize("codeword", [0, -1])
def test_word_errors_never_go_up_and_do_go_down(codeword):
    import torch
    from ldpc_decoders_amd import _lib

    code = _code("512_3_6_rand_ldpc_1")
    n, B, bins, frame0 = code.n, 8192, 21, 1000
    bp, osd = _handles(code, "f32")
    osd.order, osd.depth = 1, 64
    c_bp, c_osd, c_hand = (torch.zeros(4 + bins, dtype=torch.int64, device="cuda") for _ in range(3))
    bp.simulate("biawgn", 2.0, codeword, SEED, STREAM, frame0, B, 20, c_bp, hist_bins=bins)
    osd.simulate("biawgn", 2.0, codeword, SEED, STREAM, frame0, B, 20, c_osd, hist_bins=bins)
    if codeword == 0:
        pri, sent = bp.channel_device("biawgn", 2.0, 0, SEED, STREAM, frame0, B)[0], None
    else:
        sent = code.encoder().handle().encode_random(SEED, STREAM, frame0, B)
        pri = bp.channel_sent_device("biawgn", 2.0, sent, SEED, STREAM, frame0)[0]
    xhat, iters, pick = osd.decode_device(pri, None, 20)
    _count(_lib.load(), xhat, sent, iters, n, bins, c_hand)
    a, b, c = c_bp.cpu().numpy(), c_osd.cpu().numpy(), c_hand.cpu().numpy()
    print("codeword %d: BP %s, OSD %s" % (codeword, a[:4], b[:4]))
    assert (b == c).all()
    assert a[_lib.CNT_TOT] == b[_lib.CNT_TOT] == B and a[_lib.CNT_ITER_SUM] == b[_lib.CNT_ITER_SUM] and (a[4:] == b[4:]).all()
    assert b[_lib.CNT_WEC] < a[_lib.CNT_WEC]
    # frame by frame: a frame BP got right is not touched
    xbp, ibp = bp.decode_device(pri, None, 20)
    good = (xbp == (0 if sent is None else sent)).all(dim=1)
    assert torch.equal(xhat[good], xbp[good]) and bool((pick[good] == -1).all()) and torch.equal(iters, ibp)
    assert int(_syndrome_dev(code, xhat).max()) == 0


def test_batch_split_does_not_change_any_frame():
    import torch

    code = _code("1200_rho_x5_rand_ldpc_10")
    bp, osd = _handles(code, "f32")
    osd.order, osd.depth = 1, 64
    pri, _ = bp.channel_device("biawgn", 1.5, 0, SEED, STREAM, 500, 3000)
    whole = osd.decode_device(pri, None, 50)
    parts = [osd.decode_device(pri[a:b].contiguous(), None, 50) for a, b in ((0, 1), (1, 1234), (1234, 3000))]
    for k in range(3):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts]))
    assert int((whole[2] >= 0).sum()) >= 100


def test_refusals_launch_nothing():
    import torch
    from ldpc_decoders_amd import _lib
    from ldpc_decoders_amd._device import DecoderHandle

    lib = _lib.load()
    code, other = _code("512_3_6_rand_ldpc_1"), _code("512_3_6_rand_ldpc_2")
    bp, osd = _handles(code, "f32")
    B, n = 64, code.n
    pri, _ = bp.channel_device("biawgn", 1.0, 0, SEED, STREAM, 0, B)
    y = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
    xhat = torch.full((B, n), 7, dtype=torch.uint8, device="cuda")
    iters = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    pick = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    bad = [(DecoderHandle(code, "NMSA", "f16"), 0, 64), (DecoderHandle(code, "BEC", "f32"), 0, 64), (bp, 2, 64), (bp, 1, -1),
           (DecoderHandle(other, "NMSA", "f32"), 0, 64)]
    for dec, order, depth in bad:
        rc = lib.ldpc_osd_decode(osd.h, dec.h, pri.data_ptr(), y.data_ptr(), B, 20, 0, order, depth, xhat.data_ptr(), iters.data_ptr(),
                                 pick.data_ptr(), st)
        assert rc < 0 and len(lib.ldpc_last_error()) > 10, (dec.alg, dec.precision, order, depth)
        rc = lib.ldpc_osd_simulate(osd.h, dec.h, _lib.CHANNEL["biawgn"], 2.0, 0, SEED, STREAM, 0, B, 20, 0, order, depth, 0, counters.data_ptr(), st)
        assert rc < 0 and len(lib.ldpc_last_error()) > 10
        with pytest.raises(_lib.LdpcHipError):
            osd.decode_device(pri, None, 20, order=order, depth=depth, bp=dec)
    assert lib.ldpc_osd_decode(osd.h, DecoderHandle(code, "NMSA", "f16").h, pri.data_ptr(), None, B, 20, 0, 0, 0, xhat.data_ptr(), iters.data_ptr(),
                               pick.data_ptr(), st) == -4  # LDPC_E_UNSUPPORTED
    post = pri.clone()
    bits = torch.full((B, (n + 31) // 32), 7, dtype=torch.int32, device="cuda")
    for order, depth in ((2, 0), (-1, 0), (1, -5)):
        assert lib.ldpc_osd_solve(osd.h, 0, post.data_ptr(), pri.data_ptr(), B, order, depth, bits.data_ptr(), pick.data_ptr(), None, st) < 0
    assert lib.ldpc_osd_solve(osd.h, 2, post.data_ptr(), pri.data_ptr(), B, 0, 0, bits.data_ptr(), pick.data_ptr(), None, st) < 0  # fp16 values
    assert lib.ldpc_osd_simulate(osd.h, bp.h, _lib.CHANNEL["bec"], 0.4, 0, SEED, STREAM, 0, B, 20, 0, 0, 0, 0, counters.data_ptr(), st) < 0
    assert lib.ldpc_osd_simulate(osd.h, bp.h, _lib.CHANNEL["biawgn"], 2.0, 2, SEED, STREAM, 0, B, 20, 0, 0, 0, 0, counters.data_ptr(), st) < 0
    torch.cuda.synchronize()
    assert bool((xhat == 7).all()) and bool((iters == -7).all()) and bool((pick == -7).all()) and bool((bits == 7).all())
    assert int(counters.sum()) == 0
    # codeword 1 where a check has odd degree
    odd = _code("6_2_3_ldpc")
    assert (np.bincount(odd.edge_chk) % 2 == 1).any()
    _, osdr = _handles(odd, "f32")
    cr = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.LdpcHipError, match="odd degree"):
        osdr.simulate("biawgn", 2.0, 1, SEED, STREAM, 0, 64, 20, cr)
    with pytest.raises(ValueError):
        osd.simulate("bec", 0.4, 0, SEED, STREAM, 0, 64, 20, counters)


def _run_main(args, out_dir):
    cmd = [sys.executable, "-m", "ldpc_decoders_amd.main"] + args + ["--data_dir", str(out_dir), "--console"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]


def test_cli_writes_the_reference_files(tmp_path):
    flags = ["--params", "2", "--min-wec", "50", "--max-iter", "20"]
    _run_main(["biawgn", "512_3_6_rand_ldpc_1", "OSD"] + flags, tmp_path / "osd")
    name = "biawgn-512_3_6_rand_ldpc_1-OSD-0-50-20-0.8125-0.0-0-64.json"
    assert os.listdir(str(tmp_path / "osd")) == [name]
    osd = json.load(open(os.path.join(str(tmp_path / "osd"), name)))
    assert list(osd)[:10] == ["channel", "code", "decoder", "codeword", "min_wec", "max_iter", "msa_scale", "msa_offset", "osd_order", "osd_depth"]
    assert list(osd)[10:] == ["tot", "wec", "wer", "bec", "ber"] and osd["wec"]["2.0"] >= 50
    assert (osd["decoder"], osd["osd_order"], osd["osd_depth"]) == ("OSD", 0, 64)
    _run_main(["biawgn", "512_3_6_rand_ldpc_1", "NMSA"] + flags, tmp_path / "nmsa")
    bp = json.load(open(os.path.join(str(tmp_path / "nmsa"), "biawgn-512_3_6_rand_ldpc_1-NMSA-0-50-20-0.8125-0.0.json")))
    p0, t0 = osd["wer"]["2.0"], osd["tot"]["2.0"]
    p1, t1 = bp["wer"]["2.0"], bp["tot"]["2.0"]
    sd = np.sqrt(p0 * (1 - p0) / t0 + p1 * (1 - p1) / t1)
    print("CLI: OSD wer %g over %d frames, NMSA wer %g over %d frames" % (p0, t0, p1, t1))
    assert p0 <= p1 + 5 * sd, (p0, t0, p1, t1)


# ---- over the BSC: ldpc_osd_decode with y0, ldpc_osd_simulate with LDPC_CH_BSC, k_osd_unswept ------------------------------------------

def _bsc_frames(code, bp, B, frame0):
    """B frames of device BSC noise at p = 0.05 on encoder words; frames 3, 300, 700 and B - 1 carry the noiseless word, so they leave at
    the iteration-0 check of y0.  -> (priors, y0)"""
    import torch

    sent = code.encoder().handle().encode_random(SEED, STREAM, frame0, B)
    pri, y0 = bp.channel_sent_device("bsc", 0.05, sent, SEED, STREAM, frame0)
    llr = pri.abs().max()
    assert bool((pri.abs() == llr).all())
    clean = torch.tensor([3, 300, 700, B - 1], device=pri.device)
    y0[clean] = sent[clean]
    pri[clean] = torch.where(sent[clean] == 1, -llr, llr)
    return pri, y0


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_bsc_decode_is_bp_then_the_statement(precision):
    """ldpc_osd_decode with y0: BP's iters; a frame that left at the iteration-0 check keeps y0 (its soft output is its priors, not the
    zeros BP leaves there); every other frame is osd_frame on BP's marginals."""
    import torch

    code = _code("512_3_6_rand_ldpc_1")
    n, H = code.n, code.parity_mtx.astype(np.uint8)
    bp, osd = _handles(code, precision)
    pri, y0 = _bsc_frames(code, bp, 1024, 0)
    xhat, iters, pick = osd.decode_device(pri, y0, 20, order=1, depth=64)
    _, ibp, marg = bp.decode_soft_device(pri, y0, 20)
    assert torch.equal(iters, ibp)
    left = ibp == 0
    assert int(left.sum()) >= 4 and bool((pick[left] == -1).all()) and torch.equal(xhat[left], y0[left])
    post = torch.where(left[:, None], pri, marg)
    po, pr, x, pk = post.cpu().numpy(), pri.cpu().numpy(), xhat.cpu().numpy(), pick.cpu().numpy()
    h = OSD.hard(po)
    listed = np.flatnonzero(((h.astype(np.int64) @ H.T.astype(np.int64)) % 2).any(axis=1))
    passed = np.setdiff1d(np.arange(len(po)), listed)
    print("bsc %s: %d listed, %d left at the iteration-0 check" % (precision, len(listed), int(left.sum())))
    assert len(listed) >= 8
    assert (x[passed] == h[passed]).all() and (pk[passed] == -1).all() and (pk[listed] >= 0).all()
    for f in listed[np.linspace(0, len(listed) - 1, min(64, len(listed))).astype(int)]:
        want_x, want_t, _ = OSD.osd_frame(H, po[f], pr[f], 1, 64)
        assert pk[f] == want_t and (x[f] == want_x).all(), (precision, int(f), pk[f], want_t)
    assert int(_syndrome_dev(code, xhat).max()) == 0


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_bsc_simulate_counts_what_decode_returns(precision):
    import torch
    from ldpc_decoders_amd import _lib

    code = _code("512_3_6_rand_ldpc_1")
    n, B, bins, frame0 = code.n, 4096, 21, 1000
    bp, osd = _handles(code, precision)
    osd.order, osd.depth = 1, 64
    c_bp, c_osd, c_hand = (torch.zeros(4 + bins, dtype=torch.int64, device="cuda") for _ in range(3))
    bp.simulate("bsc", 0.05, 0, SEED, STREAM, frame0, B, 20, c_bp, hist_bins=bins)
    osd.simulate("bsc", 0.05, 0, SEED, STREAM, frame0, B, 20, c_osd, hist_bins=bins)
    pri, y0 = bp.channel_device("bsc", 0.05, 0, SEED, STREAM, frame0, B)
    xhat, iters, pick = osd.decode_device(pri, y0, 20)
    _count(_lib.load(), xhat, None, iters, n, bins, c_hand)
    a, b, c = c_bp.cpu().numpy(), c_osd.cpu().numpy(), c_hand.cpu().numpy()
    print("bsc %s: BP %s, OSD %s" % (precision, a[:4], b[:4]))
    assert (b == c).all()
    assert a[_lib.CNT_TOT] == b[_lib.CNT_TOT] == B and a[_lib.CNT_ITER_SUM] == b[_lib.CNT_ITER_SUM] and (a[4:] == b[4:]).all()
    assert int((pick >= 0).sum()) >= 8 and b[_lib.CNT_WEC] <= a[_lib.CNT_WEC]

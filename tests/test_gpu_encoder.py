"""GF(2) encoder on the i8 matrix cores (csrc/ldpc_encode.hip) and `--codeword -1` for codes without a code book."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _irregular_10000():
    from ldpc_decoders_amd import codes

    return codes.rand_irregular_ldpc(10000, codes.LAMBDA_RHO_X5_HALF_RATE, 6, np.random.RandomState(11))


def _philox_info_bits(seed, stream, frame0, B, k):
    """The oracle's statement of the random information bits: shared with test_gpu_encoder_edges.py, so it lives in encoder_codes.py."""
    from encoder_codes import philox_info_bits

    return philox_info_bits(seed, stream, frame0, B, k)


@pytest.mark.parametrize("name,B", [("7_4_hamming", 100), ("12_3_4_ldpc", 1), ("1200_3_6_ldpc", 1), ("1200_3_6_ldpc", 1000),
                                    ("512_3_6_rand_ldpc_1", 777), ("margulis", 300), ("irregular_10000", 130)])
def test_encode_device_equals_host(name, B):
    import torch

    from ldpc_decoders_amd import codes

    code = _irregular_10000() if name == "irregular_10000" else codes.get_code(name)
    enc = code.encoder()
    u = np.random.RandomState(B).randint(0, 2, (B, enc.k)).astype(np.uint8)
    got = enc.encode_device(torch.from_numpy(u).cuda()).cpu().numpy()
    want = enc.encode(u)
    assert (got == want).all()
    assert code.syndrome(got).sum() == 0


@pytest.mark.parametrize("name", ["1200_3_6_ldpc", "irregular_10000"])
def test_random_words(name):
    from ldpc_decoders_amd import codes

    code = _irregular_10000() if name == "irregular_10000" else codes.get_code(name)
    enc = code.encoder()
    seed, stream, frame0, B = 0x1234567890AB, 3, (1 << 33) + 5, 192
    sent = enc.random_words(seed, stream, frame0, B).cpu().numpy()
    u = _philox_info_bits(seed, stream, frame0, B, enc.k)
    assert (sent[:, enc.info_positions] == u).all()
    assert (sent == enc.encode(u)).all() and code.syndrome(sent).sum() == 0
    # a frame's word depends on its global index only, not on the batching
    a = enc.random_words(seed, stream, frame0, B // 2).cpu().numpy()
    b = enc.random_words(seed, stream, frame0 + B // 2, B - B // 2).cpu().numpy()
    assert (np.concatenate([a, b]) == sent).all()
    big = enc.random_words(seed, stream, 0, 4096).cpu().numpy()[:, enc.info_positions]
    N = big.size
    assert abs(big.mean() - 0.5) < 5 * 0.5 / np.sqrt(N)


@pytest.mark.parametrize("channel,param", [("biawgn", 2.0), ("bsc", 0.05), ("bec", 0.4)])
def test_channel_sent_noise_identities(channel, param):
    import bp_oracle as O
    from ldpc_decoders_amd import codes
    from ldpc_decoders_amd._device import DecoderHandle

    code = codes.get_code("1200_3_6_ldpc")
    h = DecoderHandle(code, "BEC" if channel == "bec" else "MSA", "f64", "auto")
    seed, stream, frame0, B = 77, 2, 4000, 512
    sent = code.encoder().random_words(seed, stream + 100, frame0, B)
    pri, y = h.channel_sent_device(channel, param, sent, seed, stream, frame0)
    p0, y0 = h.channel_device(channel, param, 0, seed, stream, frame0, B)
    s = sent.cpu().numpy()
    if channel == "biawgn":
        var = O.biawgn_noise_var(param)
        assert np.allclose(pri.cpu().numpy(), p0.cpu().numpy() - 4.0 * s / var, rtol=1e-12, atol=1e-12)
    elif channel == "bsc":
        assert ((y.cpu().numpy() ^ y0.cpu().numpy()) == s).all()
        assert (pri.cpu().numpy() == p0.cpu().numpy() * (1 - 2 * s.astype(np.int64))).all()
    else:
        yy, y00 = y.cpu().numpy(), y0.cpu().numpy()
        assert ((yy == 2) == (y00 == 2)).all() and (yy[yy != 2] == s[yy != 2]).all()
    # an all-zero word gives exactly ldpc_channel(codeword = 0)
    zero = sent.new_zeros(sent.shape)
    pz, yz = h.channel_sent_device(channel, param, zero, seed, stream, frame0)
    if pz is not None:
        assert (pz.cpu().numpy() == p0.cpu().numpy()).all()
    if yz is not None:
        assert (yz.cpu().numpy() == y0.cpu().numpy()).all()


@pytest.mark.parametrize("channel,param,alg,prec", [("bsc", 0.035, "MSA", "f64"), ("biawgn", 2.0, "SPA", "f32"), ("bec", 0.4, "BEC", "f32")])
def test_simulate_random_codewords_whole_path(channel, param, alg, prec):
    import torch

    import bp_oracle as O
    import c_oracle as C
    from ldpc_decoders_amd import codes
    from ldpc_decoders_amd._device import DecoderHandle

    code = codes.get_code("1200_3_6_ldpc")
    assert getattr(code, "cb", None) is None  # no code book: the encoder path
    h = DecoderHandle(code, alg, prec, "auto")
    seed, stream, frame0, B, it = 5, 1, 640, 2048, 50
    cnt = torch.zeros(4 + 51, dtype=torch.int64, device="cuda")
    h.simulate(channel, param, -1, seed, stream, frame0, B, it, cnt, hist_bins=51)
    sent = code.encoder().random_words(seed, stream, frame0, B)
    pri, y = h.channel_sent_device(channel, param, sent, seed, stream, frame0)
    xhat, iters = h.decode_device(pri, y, it)
    s, xh, its = sent.cpu().numpy(), xhat.cpu().numpy(), iters.cpu().numpy()
    err = (xh != s).sum(axis=1)
    c = cnt.cpu().numpy()
    assert c[0] == B and c[1] == (err > 0).sum() and c[2] == err.sum() and c[3] == its.sum()
    assert (c[4:] == np.bincount(np.minimum(its, 50), minlength=51)).all()
    assert 0 < c[1] < B
    # decisions of a sample of frames equal the plain-C fp64 oracle's on the same priors
    g = O.Edges(code.m, code.n, code.edge_chk, code.edge_var)
    rows = np.arange(0, B, B // 64)[:64]
    if channel == "bec":
        want_x, want_it = C.bec_decode(g, y.cpu().numpy()[rows], it)
    else:
        p = pri.cpu().numpy()[rows].astype(np.float64)
        h64 = DecoderHandle(code, alg, "f64", "auto")
        x64, i64 = h64.decode_device(pri[rows].double().contiguous(), None if y is None else y[rows].contiguous(), it)
        want_x, want_it = C.bp_decode(g, alg, None if y is None else y.cpu().numpy()[rows].astype(np.float64), p, it)
        xh, its = x64.cpu().numpy(), i64.cpu().numpy()
        rows = np.arange(len(rows))
    assert (xh[rows] == want_x).all() and (its[rows] == want_it).all()


def _run_main(args, env=None):
    cmd = [sys.executable, "-m", "ldpc_decoders_amd.main"] + args
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def test_cli_random_codeword_on_a_code_without_code_book(tmp_path):
    import json

    res = {}
    for cw in ("-1", "0"):
        _run_main(["biawgn", "1200_3_6_ldpc", "MSA", "--codeword", cw, "--precision", "f64", "--params", "2.5", "--min-wec", "200",
                   "--batch", "8192", "--data_dir", str(tmp_path / cw), "--console"])
        res[cw] = json.load(open(os.path.join(str(tmp_path / cw), "biawgn-1200_3_6_ldpc-MSA-%s-200-10.json" % cw)))
    a, b = res["-1"], res["0"]
    assert a["codeword"] == -1 and a["wec"]["2.5"] >= 200
    wa, wb = a["wer"]["2.5"], b["wer"]["2.5"]
    sd = np.sqrt(wa * (1 - wa) / a["tot"]["2.5"] + wb * (1 - wb) / b["tot"]["2.5"])
    assert abs(wa - wb) <= 4 * sd


def test_two_ranks_equal_one_rank_random_codewords(tmp_path):
    import json

    args = ["bsc", "1200_3_6_ldpc", "MSA", "--codeword", "-1", "--params", "0.04", "--min-wec", "100", "--batch", "4096", "--max-iter", "20",
            "--console"]
    env1 = dict(os.environ, LDPC_DIST_BACKEND="gloo", LDPC_DIST_FORCE_GROUP="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                MASTER_ADDR="127.0.0.1", MASTER_PORT="29811", OMP_NUM_THREADS="4")
    _run_main(args + ["--batch", "8192", "--data_dir", str(tmp_path / "one")], env=env1)
    env2 = dict(os.environ, LDPC_DIST_BACKEND="gloo", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29812", "-m", "ldpc_decoders_amd.main"] + args + ["--data_dir", str(tmp_path / "two")]
    out = subprocess.run(cmd, cwd=ROOT, env=env2, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    f = "bsc-1200_3_6_ldpc-MSA--1-100-20.json"
    one, two = json.load(open(os.path.join(str(tmp_path / "one"), f))), json.load(open(os.path.join(str(tmp_path / "two"), f)))
    for key in ("tot", "wec", "bec"):
        assert one[key] == two[key], key
    assert one["wec"]["0.04"] >= 100

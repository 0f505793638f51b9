"""Bit-sliced Gallager-B (csrc/ldpc_hard.hip): bit-exact against the numpy statement of galb_oracle.py on both backends, LDS-resident
against streaming kernels, position independence, the simulate composition, the direction against min-sum, refusals and the CLI."""
import json
import os

import numpy as np
import pytest

import galb_oracle as G
from helpers import CODES_DIR

pytestmark = pytest.mark.gpu
SEED, STREAM = 0x6A11B5EED, 3
E_ARG, E_UNSUPPORTED = -1, -4  # include/ldpc_hip.h


def _code(name):
    from ldpc_decoders_amd import codes

    return codes.get_code(name)


def _handle(code, backend, t=0):
    from ldpc_decoders_amd._device import HardHandle

    return HardHandle(code, backend, threshold=t)


def _bsc(code, p, B, frame0=0, codeword=0):
    """B frames of device BSC noise on the all-`codeword` word -> CUDA uint8 [B, n]"""
    import torch

    from ldpc_decoders_amd import _lib

    y = torch.empty((B, code.n), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().ldpc_channel(_lib.CHANNEL["bsc"], 0, float(p), codeword, SEED, STREAM, frame0, B, code.n, None, y.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    return y


def _unpack(bits, n):
    from ldpc_decoders_amd._device import unpack_bits

    return unpack_bits(bits.cpu().numpy(), n)


def _syndrome_dev(code, x):
    """x: CUDA uint8 [B, n] -> CUDA int [B] = number of unsatisfied checks."""
    import torch

    chk = torch.from_numpy(code.edge_chk.astype(np.int64)).cuda()
    var = torch.from_numpy(code.edge_var.astype(np.int64)).cuda()
    s = torch.zeros((x.shape[0], code.m), dtype=torch.int32, device=x.device)
    s.index_add_(1, chk, x[:, var].int())
    return (s & 1).sum(dim=1)


CASES = [("12_3_4_ldpc", 0.08, 2048 + 33), ("7_4_hamming", 0.08, 300), ("512_3_6_rand_ldpc_1", 0.03, 300), ("1200_3_6_rand_ldpc_1", 0.03, 300),
         ("1200_rho_x5_rand_ldpc_10", 0.004, 300), ("margulis", 0.03, 65)]
EXERCISED = ("512_3_6_rand_ldpc_1", "1200_3_6_rand_ldpc_1", "1200_rho_x5_rand_ldpc_10")


@pytest.mark.parametrize("name,p,B", CASES)
def test_bit_exact_against_the_numpy_statement(name, p, B):
    """Decisions -- as bytes and as packed words -- and iters of every frame, t in {0, 1, 255}, max_iter in {1, 20}, with and without
    NO_EARLY_EXIT, streaming and LDS-resident kernels; four all-zero rows are planted.  B = 2048 + 33 on the n = 12 code is more than
    one supertile and a ragged last slab; 7_4_hamming has degrees 1-3, the irregular code 0-8."""
    code = _code(name)
    n = code.n
    y = _bsc(code, p, B)
    y[[0, B // 3, B // 2, B - 1]] = 0
    yh = y.cpu().numpy()
    H = code.parity_mtx.astype(np.int64)
    handles = {bk: _handle(code, bk) for bk in ("stream", "fused")}
    for t in (0, 1, 255):
        for h in handles.values():
            h.set_threshold(t)
            assert h.threshold() == t
        for max_iter in (1, 20):
            for flags in (0, G.NO_EARLY_EXIT):
                want_x, want_it = G.galb_decode(code, yh, t=t, max_iter=max_iter, flags=flags)
                if t == 0 and max_iter == 20 and flags == 0:
                    ok = ~((want_x.astype(np.int64) @ H.T) & 1).any(axis=1)
                    counts = (int((want_it == 0).sum()), int((ok & (want_it >= 2)).sum()), int((~ok).sum()))
                    print("%s: left at iteration 0 / converged after >= 2 sweeps / no codeword: %s" % (name, counts))
                    if name in EXERCISED:  # the test exercises the decoder: every kind of exit occurs
                        assert counts[0] >= 4 and counts[1] >= 8 and counts[2] >= 8, counts
                for bk, h in handles.items():
                    x, it = h.decode_device(y, max_iter, flags)
                    assert h.last_backend() == bk
                    what = (name, bk, t, max_iter, flags)
                    assert (it.cpu().numpy() == want_it).all(), what
                    assert (x.cpu().numpy() == want_x).all(), what
                    bits, it2 = h.decode_device_bits(y, max_iter, flags)
                    assert (it2.cpu().numpy() == want_it).all(), what
                    assert (_unpack(bits, n) == want_x).all(), what
                    if n % 32:  # padding bits of the last word are 0
                        assert not (bits[:, -1].cpu().numpy().view(np.uint32) >> (n % 32)).any(), what


def test_lds_resident_equals_streaming(monkeypatch):
    code = _code("1200_3_6_rand_ldpc_1")
    y = _bsc(code, 0.03, 4096)
    lds, stream = _handle(code, "fused"), _handle(code, "stream")
    auto = _handle(code, "auto")
    monkeypatch.setenv("LDPC_HARD_TABLES", "lds")  # the measured variant of profiles/r13_galb.md: 16-bit graph tables in the LDS (read at create)
    tab = _handle(code, "fused")
    monkeypatch.delenv("LDPC_HARD_TABLES")
    d, id_ = tab.decode_device_bits(y, 20)
    assert tab.info()["slabs_per_cu"] < lds.info()["slabs_per_cu"]
    a, ia = lds.decode_device_bits(y, 20)
    b, ib = stream.decode_device_bits(y, 20)
    c, ic = auto.decode_device_bits(y, 20)
    assert lds.last_backend() == "fused" and stream.last_backend() == "stream" and auto.last_backend() in ("fused", "stream")
    assert (a == b).all() and (ia == ib).all() and (a == c).all() and (ia == ic).all() and (a == d).all() and (ia == id_).all()
    assert 0 < int((ia == 20).sum()) < 4096 and int(ia.min()) >= 1
    info = lds.info()
    assert info["frames_per_slab"] == 32 and info["lds_bytes_per_slab"] == 4 * (2 * code.n + code.E + code.m + 4) and info["slabs_per_cu"] >= 1
    assert stream.info()["slabs_per_cu"] == 0


def test_lds_resident_above_64_kib_per_workgroup():
    """A generated n = 4800 (3,6) code: 105 KiB per slab, one workgroup per CU, more LDS than a workgroup gets without asking; a ragged
    last slab."""
    from ldpc_decoders_amd import codes, hard

    code = codes.rand_reg_ldpc(4800, 3, 6, np.random.RandomState(17))
    assert 64 * 1024 < hard.hard_lds_bytes(code.m, code.n, code.E) <= hard.LDS_BYTES
    y = _bsc(code, 0.03, 256 + 7)
    lds, stream = _handle(code, "fused"), _handle(code, "stream")
    assert lds.info()["slabs_per_cu"] == 1
    a, ia = lds.decode_device(y, 20)
    b, ib = stream.decode_device(y, 20)
    assert lds.last_backend() == "fused" and (a == b).all() and (ia == ib).all()
    pick = np.array([0, 100, 262])
    want_x, want_it = G.galb_decode(code, y[pick].cpu().numpy(), max_iter=20)
    assert (a.cpu().numpy()[pick] == want_x).all() and (ia.cpu().numpy()[pick] == want_it).all()


@pytest.mark.parametrize("backend", ["stream", "fused"])
def test_a_frame_does_not_see_its_batch(backend):
    import torch

    code = _code("512_3_6_rand_ldpc_1")
    y = _bsc(code, 0.03, 300)
    h = _handle(code, backend)
    x, it = h.decode_device(y, 20)
    perm = torch.from_numpy(np.random.RandomState(5).permutation(300)).cuda()
    xp, itp = h.decode_device(y[perm].contiguous(), 20)
    assert (xp == x[perm]).all() and (itp == it[perm]).all()
    xs, its = h.decode_device(y[:100].contiguous(), 20)
    assert (xs == x[:100]).all() and (its == it[:100]).all()
    assert len(set(it.cpu().tolist())) > 3


@pytest.mark.parametrize("backend", ["stream", "fused"])
@pytest.mark.parametrize("channel,param,codeword", [("bsc", 0.03, 0), ("bsc", 0.03, 1), ("biawgn", 6.0, 0)])
def test_simulate_is_channel_decode_count(backend, channel, param, codeword):
    import torch

    from ldpc_decoders_amd import _lib

    lib, code = _lib.load(), _code("512_3_6_rand_ldpc_1")
    n, B, frame0, bins, max_iter = code.n, 4096 + 100, 777, 21, 20
    h = _handle(code, backend)
    st = torch.cuda.current_stream().cuda_stream
    got = torch.zeros(4 + bins, dtype=torch.int64, device="cuda")
    h.simulate(channel, param, codeword, SEED, STREAM, frame0, B, max_iter, got, hist_bins=bins)
    # by hand
    pri = torch.empty((B, n), dtype=torch.float32, device="cuda") if channel == "biawgn" else None
    y = torch.empty((B, n), dtype=torch.uint8, device="cuda") if channel == "bsc" else None
    _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE["f32"], float(param), codeword, SEED, STREAM, frame0, B, n,
                                None if pri is None else pri.data_ptr(), None if y is None else y.data_ptr(), st))
    if y is None:
        y = (pri < 0).to(torch.uint8)
    bits, it = h.decode_device_bits(y, max_iter)
    want = torch.zeros_like(got)
    _lib.check(lib.ldpc_count_errors_bits(bits.data_ptr(), None, None, codeword, it.data_ptr(), B, n, bins, want.data_ptr(), st))
    assert (got == want).all() and int(got[0]) == B and 0 < int(got[1]) < B and int(got[4:].sum()) == B
    # two halves at frame0, frame0 + B / 2
    halves = torch.zeros_like(got)
    h.simulate(channel, param, codeword, SEED, STREAM, frame0, B // 2, max_iter, halves, hist_bins=bins)
    h.simulate(channel, param, codeword, SEED, STREAM, frame0 + B // 2, B - B // 2, max_iter, halves, hist_bins=bins)
    assert (halves == got).all()


@pytest.mark.parametrize("channel,param", [("bsc", 0.03), ("biawgn", 6.0)])
def test_simulate_random_codewords(channel, param):
    import torch

    from ldpc_decoders_amd import _lib

    lib, code = _lib.load(), _code("512_3_6_rand_ldpc_1")
    n, B, frame0, bins, max_iter = code.n, 1000, 31, 21, 20
    h = _handle(code, "auto")
    st = torch.cuda.current_stream().cuda_stream
    got = torch.zeros(4 + bins, dtype=torch.int64, device="cuda")
    h.simulate(channel, param, -1, SEED, STREAM, frame0, B, max_iter, got, hist_bins=bins)
    sent = code.encoder().handle().encode_random(SEED, STREAM, frame0, B)
    assert int(sent.sum()) > 0 and not int(_syndrome_dev(code, sent).sum())
    pri = torch.empty((B, n), dtype=torch.float32, device="cuda") if channel == "biawgn" else None
    y = torch.empty((B, n), dtype=torch.uint8, device="cuda") if channel == "bsc" else None
    _lib.check(lib.ldpc_channel_sent(_lib.CHANNEL[channel], _lib.DTYPE["f32"], float(param), sent.data_ptr(), SEED, STREAM, frame0, B, n,
                                     None if pri is None else pri.data_ptr(), None if y is None else y.data_ptr(), st))
    if y is None:
        y = (pri < 0).to(torch.uint8)
    x, it = h.decode_device(y, max_iter)
    want = torch.zeros_like(got)
    _lib.check(lib.ldpc_count_errors_words(x.data_ptr(), sent.data_ptr(), it.data_ptr(), B, n, bins, want.data_ptr(), st))
    assert (got == want).all() and int(got[0]) == B and 0 < int(got[1]) < B


def test_against_the_soft_decoder():
    """The same 8192 BSC frames through GALB and fp64 min-sum: a GALB frame that left before the cap carries a codeword (syndrome
    recomputed on the device, whether or not it is the sent word), and hard decisions cannot beat the soft decoder's word errors."""
    from ldpc_decoders_amd._device import DecoderHandle

    code = _code("1200_3_6_rand_ldpc_1")
    B, max_iter = 8192, 20
    msa = DecoderHandle(code, "MSA", "f64")
    pri, y = msa.channel_device("bsc", 0.03, 0, SEED, STREAM, 0, B)
    x, it = _handle(code, "auto").decode_device(y, max_iter)
    syn = _syndrome_dev(code, x)
    early = it < max_iter
    assert int(early.sum()) > B // 2 and not int(syn[early].sum())
    wec = int((x.sum(dim=1) > 0).sum())
    xm, _ = msa.decode_device(pri, y, max_iter)
    wec_msa = int((xm.sum(dim=1) > 0).sum())
    print("word errors of 8192 frames at p = 0.03: GALB %d, fp64 MSA %d" % (wec, wec_msa))
    assert wec >= wec_msa


def test_refusals():
    import torch

    from ldpc_decoders_amd import _lib, codes, hard
    from ldpc_decoders_amd._device import HardHandle

    code = _code("12_3_4_ldpc")
    h = _handle(code, "auto")
    y = _bsc(code, 0.1, 8)
    for bad_iter in (0, -3):
        with pytest.raises(_lib.LdpcHipError, match="error %d.*max_iter" % E_ARG):
            h.decode_device(y, bad_iter)
    for bad_t in (256, -1):
        with pytest.raises(_lib.LdpcHipError, match="error %d.*0 <= t <= 255" % E_ARG):
            h.set_threshold(bad_t)
    assert h.threshold() == 0
    with pytest.raises(ValueError):
        hard.GALB(code, max_iter=0)
    with pytest.raises(ValueError):
        hard.GALB(code, max_iter=5, gal_threshold=256)
    for bad_y in (y[:, :11].contiguous(), y.int(), y.cpu(), y.t(), y[0]):
        with pytest.raises(ValueError):
            h.decode_device(bad_y, 5)
        with pytest.raises(ValueError):
            h.decode_device_bits(bad_y, 5)
    dec = hard.GALB(code, max_iter=5)
    with pytest.raises(ValueError):
        dec.decode_batch(np.zeros((3, 11), dtype=np.uint8))
    with pytest.raises(ValueError):
        dec.decode_batch(np.full((3, 12), 2, dtype=np.uint8))
    with pytest.raises(ValueError):
        dec.decode_batch(np.zeros((3, 12)))
    with pytest.raises(ValueError):
        h.simulate("bec", 0.1, 0, SEED, STREAM, 0, 64, 5, torch.zeros(4, dtype=torch.int64, device="cuda"))
    odd = _handle(codes.rand_reg_ldpc(40, 3, 5, np.random.RandomState(3)), "auto")  # checks of degree 5: the all-ones word is no codeword
    with pytest.raises(_lib.LdpcHipError, match="odd degree"):
        odd.simulate("bsc", 0.1, 1, SEED, STREAM, 0, 64, 5, torch.zeros(4, dtype=torch.int64, device="cuda"))
    # a code whose slab does not fit one CU: FUSED is refused, AUTO streams
    big = codes.rand_reg_ldpc(64800, 3, 6, np.random.RandomState(13))
    assert hard.hard_lds_bytes(big.m, big.n, big.E) > hard.LDS_BYTES
    with pytest.raises(_lib.LdpcHipError, match="error %d.*LDPC_BACKEND_FUSED" % E_UNSUPPORTED):
        HardHandle(big, "fused")
    hb = HardHandle(big, "auto")
    yb = _bsc(big, 0.03, 64)
    xb, itb = hb.decode_device(yb, 20)
    assert hb.last_backend() == "stream" and hb.info()["slabs_per_cu"] == 0
    pick = np.arange(0, 64, 8)
    want_x, want_it = G.galb_decode(big, yb[pick].cpu().numpy(), max_iter=20)
    assert (xb.cpu().numpy()[pick] == want_x).all() and (itb.cpu().numpy()[pick] == want_it).all()


def test_host_wrappers_decode_what_the_handle_decodes():
    from ldpc_decoders_amd import biawgn, bsc

    code = _code("512_3_6_rand_ldpc_1")
    y = _bsc(code, 0.03, 40)
    yh = y.cpu().numpy()
    want_x, want_it = G.galb_decode(code, yh, t=2, max_iter=20)
    dec = bsc.GALB(0.03, code, max_iter=20, gal_threshold=2)
    x, it = dec.decode_batch(yh.astype(np.int64))
    assert (x == want_x).all() and (it == want_it).all()
    xd, itd = dec.decode_batch(y)
    assert (xd.cpu().numpy() == want_x).all() and (itd.cpu().numpy() == want_it).all()
    assert (dec.decode(yh[7]) == want_x[7]).all()
    # biawgn: bit 1 <=> LLR < 0 <=> observation > 0 (the channel sends 0 as -1)
    obs = (2.0 * yh - 1.0) * 0.7
    soft = biawgn.GALB(6.0, code, max_iter=20, gal_threshold=2)
    xs, its = soft.decode_batch(obs)
    assert (xs == want_x).all() and (its == want_it).all()


def test_cli_device_and_exact(tmp_path, monkeypatch):
    from ldpc_decoders_amd import bsc, codes, main
    from ldpc_decoders_amd.montecarlo import run_point_exact

    monkeypatch.setenv(codes.file_codes_dir_string, CODES_DIR)
    base = "bsc 512_3_6_rand_ldpc_1 GALB --params 0.02 --max-iter 20 --min-wec 20".split()
    file_name = "bsc-512_3_6_rand_ldpc_1-GALB-0-20-20-0.json"
    dev_dir, exact_dir = tmp_path / "dev", tmp_path / "exact"
    main.main(base + ["--batch", "4096", "--data_dir", str(dev_dir), "--console"])
    with open(os.path.join(str(dev_dir), file_name)) as fp:
        res = json.load(fp)
    assert res["decoder"] == "GALB" and res["max_iter"] == 20 and res["gal_threshold"] == 0
    tot, wec, bec = res["tot"]["0.02"], res["wec"]["0.02"], res["bec"]["0.02"]
    assert tot % 4096 == 0 and 20 <= wec < tot and wec <= bec <= wec * 512 and res["wer"]["0.02"] == pytest.approx(wec / tot)
    # --exact: numpy noise, the reference's sequential rule; the same loop around the numpy statement gives the same counters
    main.main(base + ["--exact", "--np-seed", "1", "--data_dir", str(exact_dir), "--console"])
    with open(os.path.join(str(exact_dir), file_name)) as fp:
        res = json.load(fp)
    code = codes.get_code("512_3_6_rand_ldpc_1")

    class Oracle:
        def decode_batch(self, y):
            return G.galb_decode(code, y, t=0, max_iter=20)

    np.random.seed(1)
    want = run_point_exact(bsc.Channel(0.02), Oracle(), np.zeros(code.n, dtype=np.int64), 20, chunk=32)
    assert (res["tot"]["0.02"], res["wec"]["0.02"], res["bec"]["0.02"]) == (want["tot"], want["wec"], want["bec"])
    assert want["wec"] == 20

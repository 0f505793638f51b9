"""ML decoding over the BEC for every code (csrc/ldpc_bec_ml.hip): bit-exact against the numpy statement of test_bec_ml_cpu.py, the
reference's rule on the toy codes (k_ml's tie sets), never worse than BP frame by frame, keyed by global frame index, and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_bec_ml_cpu import ml_keyed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, STREAM = 0x1234ABCD5678, 3


def _code(name):
    from ldpc_decoders_amd import codes

    return codes.get_code(name)


def _handles(code):
    from ldpc_decoders_amd._device import BecMlHandle, DecoderHandle

    return DecoderHandle(code, "BEC", "f32"), BecMlHandle(code)


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


@pytest.mark.parametrize("name", ["1200_3_6_rand_ldpc_1", "1200_rho_x5_rand_ldpc_1", "512_3_6_rand_ldpc_1"])
def test_bit_exact_against_the_numpy_statement(name):
    import torch
    from ldpc_decoders_amd._device import unpack_bits

    code = _code(name)
    bp, ml = _handles(code)
    enc = code.encoder().handle()
    B, frame0 = 2048, 77
    for eps in (0.0, 0.40, 0.45, 0.48, 0.6, 1.0):
        sent = enc.encode_random(SEED, STREAM, frame0, B)
        _, y = bp.channel_sent_device("bec", eps, sent, SEED, STREAM, frame0)
        bits, era, _ = bp.decode_device_bits(None, y, 0)
        out, nul = ml.solve_bits(bits, era, SEED, STREAM, frame0)
        xh, nul2 = ml.decode_device(y, SEED, STREAM, frame0)
        torch.cuda.synchronize()
        assert torch.equal(xh, _unpack_dev(out, code.n)) and torch.equal(nul, nul2)
        assert torch.equal(xh, sent) or eps > 0.3  # below every threshold nothing is lost
        assert int(_syndrome_dev(code, xh).max()) == 0
        peeled = unpack_bits(bits.cpu().numpy(), code.n, era.cpu().numpy())
        listed = np.flatnonzero((peeled == 2).any(axis=1))
        done = np.setdiff1d(np.arange(B), listed)
        x_np, n_np = xh.cpu().numpy(), nul.cpu().numpy()
        # frames that peeling finished: the peeled word, nullity 0
        assert (x_np[done] == peeled[done]).all() and (n_np[done] == 0).all()
        for f in listed[:: max(1, len(listed) // 12)][:12]:
            want, d = ml_keyed(code, peeled[f], SEED, STREAM, frame0 + int(f))
            assert d == n_np[f] and (want == x_np[f]).all(), (name, eps, f)
        if eps == 1.0:
            assert (n_np == code.encoder().k).all()


@pytest.mark.parametrize("name", ["7_4_hamming", "12_3_4_ldpc", "6_2_3_ldpc", "4_2_test"])
def test_reference_rule_on_the_toy_codes(name):
    import torch
    from ldpc_decoders_amd._device import BecMlHandle, MlHandle

    code = _code(name)
    cb = code.cb.astype(np.uint8)
    rng = np.random.RandomState(21)
    B = 4096
    sent = cb[rng.randint(len(cb), size=B)]
    y = np.where(rng.random_sample(sent.shape) < rng.choice([0.2, 0.5, 0.8], size=(B, 1)), 2, sent).astype(np.uint8)
    yd = torch.from_numpy(y).cuda()
    p = 0.5
    ref = MlHandle(cb, "bec", "f64").decode_device(yd, (np.log(p), np.log(1 - p)), want_mask=True)
    xh, nul = BecMlHandle(code).decode_device(yd, SEED, STREAM, 0)
    ties = ref["ties"].cpu().numpy()
    mask = ref["tie_mask"].cpu().numpy().view(np.uint32)
    tie_bits = ((mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, -1)[:, :len(cb)]
    x_np, n_np = xh.cpu().numpy(), nul.cpu().numpy()
    idx = np.array([np.flatnonzero((cb == x).all(axis=1))[0] for x in x_np])
    assert (tie_bits[np.arange(B), idx] == 1).all()
    assert (2 ** n_np.astype(np.int64) == ties).all()
    one = ties == 1
    assert (x_np[one] == ref["xhat"].cpu().numpy()[one]).all()
    # uniform over one tie set: the same symbols in 4000 frames, each keyed by its own frame index
    y0 = y[np.argmax(ties)]
    rep = torch.from_numpy(np.repeat(y0[None, :], 4000, axis=0)).cuda()
    xr, nr = BecMlHandle(code).decode_device(rep, SEED, STREAM, 10 ** 6)
    k = int(2 ** nr[0].item())
    if k > 1:
        words, counts = np.unique(xr.cpu().numpy(), axis=0, return_counts=True)
        assert len(words) == k
        e = 4000 / k
        chi2 = ((counts - e) ** 2 / e).sum()
        assert chi2 < 3 * (k - 1) + 30, (counts, chi2)


def test_never_worse_than_bp_frame_by_frame():
    import torch
    from ldpc_decoders_amd import _lib

    code = _code("1200_3_6_rand_ldpc_1")
    bp, ml = _handles(code)
    B, eps = 65536, 0.45
    _, y = bp.channel_device("bec", eps, 0, SEED, STREAM, 0, B)
    bits, era, _ = bp.decode_device_bits(None, y, 0)
    out, nul = ml.solve_bits(bits, era, SEED, STREAM, 0)
    assert int(((out & ~era) != 0).sum()) == 0  # every ML error bit lies in BP's residual (sent word: all zero)
    done = (era == 0).all(dim=1)
    assert torch.equal(out[done], bits[done])
    x = _unpack_dev(out, code.n)
    assert int(_syndrome_dev(code, x).max()) == 0
    assert bool(((x == y) | (y == 2)).all())
    assert int(nul.min()) >= 0
    c_ml = torch.zeros(4, dtype=torch.int64, device="cuda")
    c_bp = torch.zeros(4, dtype=torch.int64, device="cuda")
    ml.simulate("bec", eps, 0, SEED, STREAM, 0, B, 0, c_ml)
    bp.simulate("bec", eps, 0, SEED, STREAM, 0, B, 0, c_bp)
    a, b = c_ml.cpu().numpy(), c_bp.cpu().numpy()
    assert a[_lib.CNT_TOT] == b[_lib.CNT_TOT] == B and a[_lib.CNT_ITER_SUM] == 0
    assert a[_lib.CNT_WEC] <= b[_lib.CNT_WEC] and a[_lib.CNT_BEC] <= b[_lib.CNT_BEC]
    assert a[_lib.CNT_WEC] == int((x != 0).any(dim=1).sum()) and a[_lib.CNT_BEC] == int(x.sum())


def test_batch_split_does_not_change_any_frame():
    import torch

    code = _code("1200_rho_x5_rand_ldpc_1")
    bp, ml = _handles(code)
    _, y = bp.channel_device("bec", 0.47, 0, SEED, STREAM, 500, 3000)
    whole, nw = ml.decode_device(y, SEED, STREAM, 500)
    parts = [ml.decode_device(y[a:b].contiguous(), SEED, STREAM, 500 + a) for a, b in ((0, 1), (1, 1234), (1234, 3000))]
    assert torch.equal(whole, torch.cat([p[0] for p in parts])) and torch.equal(nw, torch.cat([p[1] for p in parts]))


def test_random_codewords_and_codeword_one():
    import torch

    code = _code("512_3_6_rand_ldpc_1")
    bp, ml = _handles(code)
    sent = code.encoder().handle().encode_random(SEED, STREAM, 0, 4096)
    _, y = bp.channel_sent_device("bec", 0.45, sent, SEED, STREAM, 0)
    xh, _ = ml.decode_device(y, SEED, STREAM, 0)
    assert int(_syndrome_dev(code, xh).max()) == 0 and bool(((xh == y) | (y == 2)).all())
    c1 = torch.zeros(4, dtype=torch.int64, device="cuda")
    ml.simulate("bec", 0.45, 1, SEED, STREAM, 0, 8192, 0, c1)  # every check of this code has degree 6: all-ones is a codeword
    c0 = torch.zeros(4, dtype=torch.int64, device="cuda")
    ml.simulate("bec", 0.45, 0, SEED, STREAM, 0, 8192, 0, c0)
    a, b = c0.cpu().numpy(), c1.cpu().numpy()  # same erasure patterns; the free bits land on the other solutions: equal in law
    assert a[0] == b[0] == 8192 and abs(int(a[1]) - int(b[1])) <= 5 * np.sqrt(a[1] + b[1]) + 5


def _run_main(args, out_dir):
    cmd = [sys.executable, "-m", "ldpc_decoders_amd.main"] + args + ["--data_dir", str(out_dir), "--console"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]


def test_cli_writes_the_reference_files(tmp_path):
    _run_main(["bec", "1200_3_6_rand_ldpc_1", "ML", "--params", "0.45", "--min-wec", "50", "--batch", "16384"], tmp_path / "ml")
    ml = json.load(open(os.path.join(str(tmp_path / "ml"), "bec-1200_3_6_rand_ldpc_1-ML-0-50.json")))
    assert list(ml)[:5] == ["channel", "code", "decoder", "codeword", "min_wec"]
    assert {"tot", "wec", "wer", "bec", "ber"} <= set(ml) and ml["wec"]["0.45"] >= 50
    _run_main(["bec", "1200_3_6_rand_ldpc_1", "SPA", "--params", "0.45", "--min-wec", "50", "--max-iter", "0", "--batch", "16384"],
              tmp_path / "spa")
    spa = json.load(open(os.path.join(str(tmp_path / "spa"), "bec-1200_3_6_rand_ldpc_1-SPA-0-50-0.json")))
    assert spa["wer"]["0.45"] >= ml["wer"]["0.45"]
    _run_main(["bec", "1200_3_6_rand_ldpc_1", "ML", "--codeword", "-1", "--params", "0.45", "--min-wec", "50", "--batch", "16384"],
              tmp_path / "rand")
    rnd = json.load(open(os.path.join(str(tmp_path / "rand"), "bec-1200_3_6_rand_ldpc_1-ML--1-50.json")))
    p0, t0 = ml["wer"]["0.45"], ml["tot"]["0.45"]
    p1, t1 = rnd["wer"]["0.45"], rnd["tot"]["0.45"]
    sd = np.sqrt(p0 * (1 - p0) / t0 + p1 * (1 - p1) / t1)
    assert abs(p0 - p1) <= 5 * sd + 1e-3, (p0, t0, p1, t1)

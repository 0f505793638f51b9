"""One call across the 2^17-frame chunk of the elimination ML decoder, the ordered-statistics post-processor and Gallager-B: B = 2^17 + 37
frames of 12_3_4_ldpc against the same frames in two calls split at frame 70 000 (both parts below one chunk, ``frame0`` advanced), every
frame equal; and the numpy statements on frames 2^17 - 8 ... 2^17 + 36.  A pointer offset or a Philox key of the second chunk that
forgets the chunk's first frame fails here.  test_edge_codes_cpu.py asserts what the batches hold."""
import numpy as np
import pytest

import edge_codes as EC
import galb_oracle as G
import osd_oracle as OSD
from test_bec_ml_cpu import ml_keyed

pytestmark = pytest.mark.gpu
SEED, STREAM = 0xC4055ED, 7
FRAME0 = (1 << 33) + 999
B, SPLIT, WINDOW = EC.CROSS_B, EC.CROSS_SPLIT, EC.CROSS_WINDOW
PARTS = ((0, SPLIT), (SPLIT, B))
SCALE = 0.8125


def _code():
    from ldpc_decoders_amd import codes

    return codes.get_code("12_3_4_ldpc")


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unpack_dev(bits, n):
    import torch

    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits[:, :, None] >> sh) & 1).reshape(bits.shape[0], -1)[:, :n].to(torch.uint8)


def _whole_equals_parts(call, tensors):
    """call(frame offset, the tensors' rows [a, b)) -> tuple of tensors with one row per frame: one call on all of them against the two
    parts.  -> the whole call's outputs"""
    import torch

    whole = call(0, *tensors)
    parts = [call(a, *[None if t is None else t[a:b].contiguous() for t in tensors]) for a, b in PARTS]
    torch.cuda.synchronize()
    for k in range(len(whole)):
        got = torch.cat([p[k] for p in parts])
        assert whole[k].shape[0] == B and torch.equal(whole[k], got), (k, int((whole[k] != got).reshape(B, -1).any(dim=1).sum()))
    return whole


def _counters_add_up(simulate, size=4):
    import torch
    from ldpc_decoders_amd import _lib

    one, two = (torch.zeros(size, dtype=torch.int64, device="cuda") for _ in range(2))
    simulate(FRAME0, B, one)
    for a, b in PARTS:
        simulate(FRAME0 + a, b - a, two)
    one, two = one.cpu().numpy(), two.cpu().numpy()
    assert one[_lib.CNT_TOT] == B and (one == two).all(), (one, two)
    return one


def test_bec_ml_across_the_chunk():
    import torch
    from ldpc_decoders_amd._device import BecMlHandle, DecoderHandle, unpack_bits

    code = _code()
    bp, ml = DecoderHandle(code, "BEC", "f32"), BecMlHandle(code)
    sent, y = EC.cross_bec(code, EC.SEED + 6)
    yd = _dev(y)
    xh, nul = _whole_equals_parts(lambda a, t: ml.decode_device(t, SEED, STREAM, FRAME0 + a), [yd])
    peel = [bp.decode_device_bits(None, yd[a:b].contiguous(), 0) for a, b in PARTS]
    bits, era = (torch.cat([p[k] for p in peel]) for k in (0, 1))
    out, nul2 = _whole_equals_parts(lambda a, bi, er: ml.solve_bits(bi, er, SEED, STREAM, FRAME0 + a), [bits, era])
    assert torch.equal(_unpack_dev(out, code.n), xh) and torch.equal(nul, nul2)
    peeled = unpack_bits(bits.cpu().numpy(), code.n, era.cpu().numpy())
    assert (peeled[WINDOW] == EC.peel_batch(code, y[WINDOW])).all()
    x, d = xh.cpu().numpy(), nul.cpu().numpy()
    free = 0
    for f in range(WINDOW.start, WINDOW.stop):
        want, dd = ml_keyed(code, peeled[f], SEED, STREAM, FRAME0 + f)
        assert dd == d[f] and (want == x[f]).all(), f
        free += int(dd > 0 and f >= EC.CHUNK)
    assert free >= 8  # frames of the second chunk whose word the key decides
    assert code.syndrome(x).sum() == 0 and ((x == y) | (y == 2)).all() and d.min() >= 0
    cnt = _counters_add_up(lambda f0, nb, c: ml.simulate("bec", 0.5, 0, SEED, STREAM, f0, nb, 0, c))
    assert cnt[1] > 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_osd_across_the_chunk(precision):
    import torch
    from ldpc_decoders_amd._device import DecoderHandle, OsdHandle

    code = _code()
    n, H = code.n, code.parity_mtx.astype(np.uint8)
    dtype = np.float64 if precision == "f64" else np.float32
    bp = DecoderHandle(code, "NMSA", precision)
    bp.set_correction(SCALE, 0.0)
    osd = OsdHandle(bp, order=1, depth=64)
    frames = range(WINDOW.start, WINDOW.stop)
    # solve
    post, prior = EC.cross_llr(code, EC.SEED + 7, dtype)
    bits, pick, cost = _whole_equals_parts(lambda a, po, pr: osd.solve(po, pr, 1, 64), [_dev(post), _dev(prior)])
    x, pk, co = _unpack_dev(bits, n).cpu().numpy(), pick.cpu().numpy(), cost.cpu().numpy()
    for f in frames:
        want_x, want_t, want_c = OSD.osd_frame(H, post[f], prior[f], 1, 64)
        assert pk[f] == want_t and co[f] == want_c and (x[f] == want_x).all(), f
    assert (pk[EC.CHUNK:] >= 0).sum() >= 8 and (pk[EC.CHUNK:] == -1).sum() >= 8
    # decode: BP in front, without and with the iteration-0 check of y0
    noisy = EC.cross_llr(code, EC.SEED + 9, dtype, snr_db=-1.0)[1]  # BP leaves frames of these without a codeword
    y0, bsc_pri = EC.cross_bsc(code, EC.SEED + 8, dtype)
    for pri, y in ((noisy, None), (bsc_pri, y0)):
        pd, yd = _dev(pri), None if y is None else _dev(y)
        xh, iters, pick = _whole_equals_parts(lambda a, p, yy: osd.decode_device(p, yy, 5), [pd, yd])
        w = slice(WINDOW.start, WINDOW.stop)
        _, it_bp, marg = bp.decode_soft_device(pd[w].contiguous(), None if yd is None else yd[w].contiguous(), 5)
        assert torch.equal(iters[w], it_bp)
        it_np, x, pk = it_bp.cpu().numpy(), xh.cpu().numpy(), pick.cpu().numpy()
        soft = np.where(it_np[:, None] == 0, pri[w], marg.cpu().numpy())
        for i, f in enumerate(frames):
            want_x, want_t, _ = OSD.osd_frame(H, soft[i], pri[f], 1, 64)
            assert pk[f] == want_t and (x[f] == want_x).all(), (f, y is None)
        assert code.syndrome(x).sum() == 0 and (pk[EC.CHUNK:] >= 0).sum() >= 4
        if y is not None:
            left = it_np == 0
            assert left[8:].sum() >= 4 and (pk[w][left] == -1).all() and (x[w][left] == y[w][left]).all()
    for channel, param in (("biawgn", -1.0), ("bsc", 0.15)):
        cnt = _counters_add_up(lambda f0, nb, c: osd.simulate(channel, param, 0, SEED, STREAM, f0, nb, 5, c, hist_bins=6), 4 + 6)
        assert cnt[4:].sum() == B


@pytest.mark.parametrize("backend", ["stream", "fused"])
def test_gallager_b_across_the_chunk(backend):
    from ldpc_decoders_amd._device import HardHandle

    code = _code()
    h = HardHandle(code, backend)
    y0, _ = EC.cross_bsc(code, EC.SEED + 8, np.float32)
    xh, iters = _whole_equals_parts(lambda a, t: h.decode_device(t, 20), [_dev(y0)])
    assert h.last_backend() == backend
    want_x, want_it = G.galb_decode(code, y0[WINDOW], max_iter=20)
    assert (xh.cpu().numpy()[WINDOW] == want_x).all() and (iters.cpu().numpy()[WINDOW] == want_it).all()
    assert (want_it[8:] > 0).sum() >= 8
    cnt = _counters_add_up(lambda f0, nb, c: h.simulate("bsc", 0.15, 0, SEED, STREAM, f0, nb, 20, c, hist_bins=21), 4 + 21)
    assert cnt[4:].sum() == B and cnt[1] > 0

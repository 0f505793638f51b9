"""The GF(2) elimination kernels (csrc/ldpc_bec_ml.hip, csrc/ldpc_osd.hip) on the synthetic codes of edge_codes.py: n, |R| and m at the
word (32), lane / row-block (64) and power-of-two edges, rank-deficient graphs with a duplicated row, a variable in no check and
degree-1 variables, inconsistent systems (nullity -1), both passes of k_bec_ml_solve in one call, codes on each side of the 160 KiB create
rules.  Every frame is compared with the numpy statements (test_bec_ml_cpu.ml_keyed, osd_oracle.osd_frame): ``==`` on words, nullities,
picks and the fp64 costs.  test_edge_codes_cpu.py asserts what the batches hold."""
import ctypes
import time

import numpy as np
import pytest

import edge_codes as EC
import osd_oracle as OSD
from test_bec_ml_cpu import ml_keyed

pytestmark = pytest.mark.gpu
SEED, STREAM = 0x5EED0ED6E5, 5
FRAME0 = (1 << 33) + 12345  # above 2^32: the high word of the Philox frame counter matters
IDS = ["%dx%d" % s[:2] for s in EC.SHAPES]
LDPC_E_ARG = -1


def _timed(what, make):
    t = time.time()
    out = make()
    print("create %s: %.3f s" % (what, time.time() - t))
    return out


def _bec_handles(code, tag):
    from ldpc_decoders_amd._device import BecMlHandle, DecoderHandle

    ml = _timed("BecMlHandle %s" % tag, lambda: BecMlHandle(code))
    return DecoderHandle(code, "BEC", "f32", backend="stream"), ml


def _unpack_dev(bits, n):
    import torch

    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits[:, :, None] >> sh) & 1).reshape(bits.shape[0], -1)[:, :n].to(torch.uint8)


def _bec_run(code, bp, ml, y, frame0):
    """decode_device and peel + solve_bits on one batch -> (words [B, n], nullities [B], the device's peeled words with 2 = residual)"""
    import torch
    from ldpc_decoders_amd._device import unpack_bits

    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint8)).cuda()
    xh, nul = ml.decode_device(yd, SEED, STREAM, frame0)
    bits, era, _ = bp.decode_device_bits(None, yd, 0)
    out, nul2 = ml.solve_bits(bits, era, SEED, STREAM, frame0)
    torch.cuda.synchronize()
    assert torch.equal(xh, _unpack_dev(out, code.n)) and torch.equal(nul, nul2)
    return xh.cpu().numpy(), nul.cpu().numpy(), unpack_bits(bits.cpu().numpy(), code.n, era.cpu().numpy())


def _bec_against_statement(code, y, x, nul, peeled, frame0, frames):
    """Every frame of ``frames``: word and nullity of the keyed statement; under nullity -1 the unerased symbols are returned as they came."""
    bad = []
    for f in frames:
        want, d = ml_keyed(code, peeled[f], SEED, STREAM, frame0 + int(f))
        assert d == nul[f], (int(f), d, int(nul[f]))
        if d >= 0:
            assert (want == x[f]).all(), (int(f), d)
        else:
            bad.append(int(f))
            assert x[f].max() <= 1 and (x[f][y[f] != 2] == y[f][y[f] != 2]).all(), int(f)
    return bad


@pytest.mark.parametrize("m,n,redundant", EC.SHAPES, ids=IDS)
def test_bec_ml_every_frame_against_the_statement(m, n, redundant):
    code = EC.shape_code(m, n, redundant)
    bp, ml = _bec_handles(code, "%d x %d" % (m, n))
    sent, y = EC.bec_batch(code, EC.SEED + 1)
    P = EC.peel_batch(code, y)
    x, nul, peeled = _bec_run(code, bp, ml, y, FRAME0)
    assert (peeled == P).all()  # step 1 of the contract: the stopping-set exit
    listed = (P == 2).any(axis=1)
    assert (x[~listed] == P[~listed]).all() and (nul[~listed] == 0).all()
    assert not _bec_against_statement(code, y, x, nul, peeled, FRAME0, range(len(y)))
    assert code.syndrome(x).sum() == 0 and ((x == y) | (y == 2)).all()
    a, i = EC.BEC_PLANTED["all"], EC.BEC_PLANTED["isolated"]
    assert nul[a] == n - code.encoder().rank and nul[i] == 1 and nul[EC.BEC_PLANTED["none"]] == 0 == nul[EC.BEC_PLANTED["degree_one"]]
    # inconsistent systems: 16 listed frames with one unerased bit next to the residual set flipped
    y_bad, P_bad, flipped = EC.inconsistent_batch(code, y, P)
    xb, nb, pb = _bec_run(code, bp, ml, y_bad, FRAME0)
    assert (pb == P_bad).all()
    same = np.setdiff1d(np.arange(len(y)), flipped)
    assert (xb[same] == x[same]).all() and (nb[same] == nul[same]).all()
    assert _bec_against_statement(code, y_bad, xb, nb, pb, FRAME0, flipped) == flipped.tolist()
    assert (np.flatnonzero(nb == -1) == flipped).all()
    print("%d x %d: %d listed, %d passed through, 16 inconsistent, nullities up to %d" % (m, n, listed.sum(), (~listed).sum(), nul.max()))


def test_bec_ml_both_passes_in_one_call():
    """The m = 897 code: the all-erased frames need 34 764 B and go to the overflow list, every other listed frame is solved by the 32 KiB
    pass, in the same call.  On the m = 896 code the all-erased frame takes 32 460 B and the first pass keeps it."""
    n, fits, over, _ = EC.OVERFLOW
    code = EC.overflow_code(over)
    bp, ml = _bec_handles(code, "%d x %d" % (over, n))
    sent, y = EC.overflow_batch(code, EC.SEED + 3)
    P = EC.peel_batch(code, y)
    x, nul, peeled = _bec_run(code, bp, ml, y, FRAME0)
    assert (peeled == P).all()
    assert not _bec_against_statement(code, y, x, nul, peeled, FRAME0, range(len(y)))
    need = np.array([EC.lds_bytes_of(code, p) for p in P])
    second = np.flatnonzero(need > EC.SMALL_SLAB)
    assert len(second) >= 8 and len(np.unique(x[second], axis=0)) > 1  # the same erasures, other free bits
    code = EC.overflow_code(fits)
    bp, ml = _bec_handles(code, "%d x %d" % (fits, n))
    y = np.full((3, n), 2, dtype=np.uint8)
    x, nul, peeled = _bec_run(code, bp, ml, y, FRAME0)
    assert (peeled == 2).all() and (nul == n - code.encoder().rank).all()
    assert not _bec_against_statement(code, y, x, nul, peeled, FRAME0, range(3))


def test_bec_ml_create_rule_at_its_limit():
    """n = 2048 with m = 576 (151 308 B: the first decode that uses nearly all of a CU's LDS) is decoded; m = 577 (167 948 B) is refused by
    the constructor before the library is asked, and by ldpc_bec_ml_create with LDPC_E_ARG."""
    from ldpc_decoders_amd import _lib, bec_ml
    from ldpc_decoders_amd._device import code_handle

    n, ok, refused = EC.LIMIT_BEC
    code = EC.limit_code(ok, n)
    bp, ml = _bec_handles(code, "%d x %d" % (ok, n))
    sent, y = EC.limit_bec_batch(code, EC.SEED + 4)
    x, nul, peeled = _bec_run(code, bp, ml, y, FRAME0)
    assert (peeled == EC.peel_batch(code, y)).all() and (peeled[0] == 2).all()
    assert not _bec_against_statement(code, y, x, nul, peeled, FRAME0, range(len(y)))
    assert code.syndrome(x).sum() == 0 and nul[0] == n - code.encoder().rank
    bad = EC.limit_code(refused, n)
    with pytest.raises(ValueError, match="167948"):
        bec_ml.BecEliminationML(0.4, bad)
    h = ctypes.c_void_p()
    lib = _lib.load()
    assert lib.ldpc_bec_ml_create(code_handle(bad).h, ctypes.byref(h)) == LDPC_E_ARG and not h
    assert b"167948" in lib.ldpc_last_error()


# ---- ordered-statistics post-processing -------------------------------------------------------------------------------------------------

DEPTHS = [(0, 0), (1, 1), (1, 63), (1, 64), (1, 127), (1, 128), (1, 10 ** 6)]


def _osd_handles(code, precision, tag):
    from ldpc_decoders_amd._device import DecoderHandle, OsdHandle

    bp = DecoderHandle(code, "NMSA", precision, backend="stream")  # never runs here; "stream": no LDS plan is searched for a throw-away code
    return bp, _timed("OsdHandle %s %s" % (tag, precision), lambda: OsdHandle(bp))


def _osd_against_statement(code, osd, post, prior, cases):
    """solve at every (order, depth) of ``cases`` against osd_frame on every listed frame; pass-through frames in full.
    -> {(order, depth): picks}"""
    import torch

    n, H = code.n, code.parity_mtx.astype(np.uint8)
    pd, qd = torch.from_numpy(post).cuda(), torch.from_numpy(prior).cuda()
    h = OSD.hard(post)
    listed = EC.osd_listed(code, post)
    passed = np.setdiff1d(np.arange(len(post)), listed)
    elim = {f: OSD.eliminate(H, post[f]) for f in listed}
    picks = {}
    for order, depth in cases:
        bits, pick, cost = osd.solve(pd, qd, order, depth)
        x, pk, co = _unpack_dev(bits, n).cpu().numpy(), pick.cpu().numpy(), cost.cpu().numpy()
        assert (x[passed] == h[passed]).all() and (pk[passed] == -1).all() and (co[passed] == -1.0).all()
        assert code.syndrome(x).sum() == 0
        for f in listed:
            want_x, want_t, want_c = OSD.osd_frame(H, post[f], prior[f], order, depth, elim=elim[f])
            assert pk[f] == want_t and co[f] == want_c and (x[f] == want_x).all(), (order, depth, int(f), int(pk[f]), want_t, co[f], want_c)
        picks[(order, depth)] = pk[listed]
    return picks


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("m,n,redundant", EC.SHAPES, ids=IDS)
def test_osd_every_frame_against_the_statement(m, n, redundant, precision):
    code = EC.shape_code(m, n, redundant)
    bp, osd = _osd_handles(code, precision, "%d x %d" % (m, n))
    post, prior = EC.osd_batch(code, EC.SEED + 2, np.float64 if precision == "f64" else np.float32)
    picks = _osd_against_statement(code, osd, post, prior, DEPTHS)
    nf = n - code.encoder().rank
    deep = picks[(1, 10 ** 6)]
    assert int(deep.max()) <= nf and (picks[(0, 0)] == 0).all()
    print("%d x %d %s: %d listed, |F| = %d, %d frames picked the last candidate at depth >= |F|, %d some flip, largest pick %d"
          % (m, n, precision, len(deep), nf, (deep == nf).sum(), (deep > 0).sum(), deep.max()))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_osd_create_rule_at_its_limit(precision):
    """n = 1536 with m = 576 (152 512 B) is solved; m = 577 (164 800 B) is refused by bpa.OSD before the library is asked, and by
    ldpc_osd_create with LDPC_E_ARG."""
    from ldpc_decoders_amd import _lib, bpa
    from ldpc_decoders_amd._device import code_handle

    n, ok, refused = EC.LIMIT_OSD
    code = EC.limit_code(ok, n)
    bp, osd = _osd_handles(code, precision, "%d x %d" % (ok, n))
    post, prior = EC.limit_osd_batch(code, EC.SEED + 5, np.float64 if precision == "f64" else np.float32)
    picks = _osd_against_statement(code, osd, post, prior, [(1, 64)])
    assert len(picks[(1, 64)]) == 8
    bad = EC.limit_code(refused, n)
    with pytest.raises(ValueError, match="164800"):
        bpa.OSD(bad, max_iter=5)
    h = ctypes.c_void_p()
    lib = _lib.load()
    assert lib.ldpc_osd_create(code_handle(bad).h, ctypes.byref(h)) == LDPC_E_ARG and not h
    assert b"164800" in lib.ldpc_last_error()

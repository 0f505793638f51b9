"""Several frames per wave for quasi-cyclic codes of lifting size up to 32 (csrc/ldpc_qc.hip k_qc_pack, ldpc_qcpack_*): decisions -- bytes and
packed words -- iteration counts and soft outputs equal to the integer statement of lqmsa_oracle.py with the block rows as layers, with
``==``, and equal to what the same handle returns at one frame per workgroup.  The codes, noise draws, bisection and comparisons are those
of test_gpu_qc.py (its helpers and its caches are used, so a reference is computed once): every number of slots from 2 to 64, idle lanes,
irregular block rows, the loop form, a code whose slots the LDS limits, fp32 and fp64 priors, parameters, caps, the flag, block-row orders,
batch sizes around the slot count, slots that refill with mixed exit times, received codewords in a row over the BSC, the refusals, the
simulate composition, the class and the command line."""
import json
import os

import numpy as np
import pytest

import bp_oracle as O
import lqmsa_oracle as LQ
import test_gpu_qc as Q

pytestmark = pytest.mark.gpu
SEED, STREAM = Q.SEED, Q.STREAM
E_ARG = Q.E_ARG
DENSE = [1, 2, 7, 16, 21, 22, 31, 32]  # frames per wave 64, 32, 9 (one idle lane), 4, 3 (one idle lane), 2 (20 idle lanes), 2, 2
ALL_KEYS = [("dense", z) for z in DENSE] + ["irregular 13", "loop 8", "loop 16", "4x8", "lds"]


def _code(key):
    """-> (oracle edge list, codes.Code, base, Z); the seeds of test_gpu_qc, whose cache holds the codes of this file too"""
    from ldpc_decoders_amd import layered, qc

    if not isinstance(key, tuple) and key != "4x8" and key not in Q._CODES:
        if key == "irregular 13":
            c = qc.rand_qc_ldpc(Q.IRREGULAR, 13, np.random.RandomState(11))
            assert (c.qc[0] >= 0).sum(axis=1).tolist() == [2, 3, 7, 8, 8] and {0, 1} <= set(np.unique(c.col_degrees()))
        elif key in ("loop 8", "loop 16"):
            c = qc.rand_qc_ldpc(Q.LOOP, int(key.split()[1]), np.random.RandomState(12), girth6=False)
            assert (c.qc[0] >= 0).sum(axis=1).tolist() == [9, 16, 17, 33]
        else:  # the LDS holds three frames of it where the lanes take four
            assert key == "lds"
            c = qc.rand_qc_ldpc(qc.regular_mask(250, 500, 3), 16, np.random.RandomState(15))
            assert c.n == 8000 and layered.lqmsa_lds_bytes(c.m, c.n, c.E, 6) == 48016
        Q._CODES[key] = (O.Edges(c.m, c.n, c.edge_chk, c.edge_var), c, c.qc[0], c.qc[1])
    return Q._code(key)


def _rule(key):
    from ldpc_decoders_amd import layered, qc

    _, c, base, Z = _code(key)
    return qc.qc_pack(Z, layered.lqmsa_lds_bytes(c.m, c.n, c.E, int((base >= 0).sum(axis=1).max())))


def _shape(key):
    """(frames, cap) of the key's batch"""
    return (12, 20) if key == "lds" else (32, 50)


def _batch(key, B=None, cap=None):
    _code(key)
    b, c = _shape(key)
    return Q._batch(key, B or b, cap or c)


def _handle(key, P=0, params=None, order=None):
    _code(key)
    h = Q._handle(key, params, order)
    h.set_pack(P)
    return h


def _equal(got, ref, where):
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and np.array_equal(a, b), where


# ---------------------------------------------------------------------------------------------- 1. every code at the rule's pick
def test_the_rule_picks_what_the_list_says():
    assert [_rule(("dense", z)) for z in DENSE] == [64, 32, 9, 4, 3, 2, 2, 2]
    assert [_rule(k) for k in ALL_KEYS[len(DENSE):]] == [4, 8, 4, 2, 3]


@pytest.mark.parametrize("key", ALL_KEYS, ids=str)
def test_equals_the_integer_statement(key):
    """The rule's pick, default parameters, natural order; fp64 and fp32 priors; the +-inf frame and the all-zero frame; the same handle at
    one frame per workgroup returns the same tensors.  info() under packing."""
    from ldpc_decoders_amd import layered, qc

    g, c, base, Z = _code(key)
    B, cap = _shape(key)
    pri, snr = _batch(key)
    h = _handle(key)
    P = _rule(key)
    assert 2 <= P <= 64 // Z and h.pack() == (P, P)
    need = layered.lqmsa_lds_bytes(c.m, c.n, c.E, int((base >= 0).sum(axis=1).max()))
    info = h.info()
    per_cu = min(layered.LDS_BYTES // (P * qc.qc_pack_stride(need, Z)), 32)
    assert info["lds_bytes_per_frame"] == need and info["waves_per_frame"] == 1 and info["frames_per_cu"] == P * per_cu
    assert info["workgroups"] % per_cu == 0 and info["workgroups"] >= per_cu
    for dt in (np.float64, np.float32):
        p = pri.astype(dt)
        want = Q._want(key, "parity", None, p, cap)
        left = (want[1] < cap).sum()  # (_batch asserted a third to two thirds of the B - 2 noisy frames, on the fp64 priors)
        assert want[1][B - 1] == 1 and (key in Q.TINY or B / 3 - 2 <= left <= 2 * B / 3 + 2), (key, snr, left)
        got = Q._run(h, p, None, cap)
        Q._same(got, want, (key, dt.__name__, "P = %d" % P))
    h.set_pack(1)
    assert h.pack() == (1, P) and h.info()["frames_per_cu"] == Q._handle(key).info()["frames_per_cu"]
    _equal(Q._run(h, p, None, cap), got, (key, "one frame per workgroup"))


@pytest.mark.parametrize("key,packs", [(("dense", 7), range(1, 10)), (("dense", 16), (2, 3))], ids=str)
def test_every_number_of_slots(key, packs):
    pri = _batch(key)[0].astype(np.float32)
    want = Q._want(key, "parity", None, pri, 50)
    h = _handle(key, 1)
    for P in packs:
        h.set_pack(P)
        assert h.pack()[0] == P and (P == 1 or h.info()["frames_per_cu"] % P == 0)
        Q._same(Q._run(h, pri, None, 50), want, (key, "P = %d" % P))


# ---------------------------------------------------------------------------------------------- 2. set, get, refusals
def test_set_get_and_refusals():
    from ldpc_decoders_amd import _lib
    from ldpc_decoders_amd._device import QcHandle

    lib = _lib.load()
    for key, good, bad in ((("dense", 7), 4, (10, 64, -1, -7)), (("dense", 22), 2, (3, 4)), ("lds", 2, (4, 5)), (("dense", 65), 1, (2, 3))):
        c, Z = (_code(key) if key != ("dense", 65) else Q._code(key))[1::2]
        h = QcHandle(c, Z)
        assert h.pack() == (1, _rule(key) if Z <= 32 else 1)  # the state after create
        h.set_pack(good)
        for P in bad:
            assert lib.ldpc_qcpack_set(h.h, P) == E_ARG
            msg = lib.ldpc_last_error().decode()
            assert "Z = %d" % Z in msg and "bytes" in msg and "ldpc_qcpack_set" in msg, msg
            assert h.pack()[0] == good
            with pytest.raises(_lib.LdpcHipError, match="error %d.*ldpc_qcpack_set" % E_ARG):
                h.set_pack(P)
        h.set_pack(0)
        assert h.pack() == (h.pack()[1],) * 2
        assert QcHandle(c, Z, pack=0).pack() == h.pack() and QcHandle(c, Z, pack=good).pack()[0] == good
    # the handle is usable after the refusals, at the value that stayed
    key = ("dense", 7)
    pri = _batch(key)[0].astype(np.float32)
    h = _handle(key, 4)
    assert lib.ldpc_qcpack_set(h.h, 10) == E_ARG and h.pack() == (4, 9)
    Q._same(Q._run(h, pri, None, 50), Q._want(key, "parity", None, pri, 50), (key, "after a refusal"))
    assert lib.ldpc_qcpack_set(None, 1) == E_ARG and lib.ldpc_qcpack_get(h.h, None, None) == E_ARG


# ---------------------------------------------------------------------------------------------- 3. parameters, caps, the flag
@pytest.mark.parametrize("key", [("dense", 16), "irregular 13", "loop 8"], ids=str)
def test_parameters_caps_and_flags(key):
    """Five parameter sets at cap 50; max_iter 1 and 2; LDPC_FLAG_NO_EARLY_EXIT; max_iter <= 0 runs to the frame's own exit."""
    pri = _batch(key)[0].astype(np.float32)
    h = _handle(key)
    for params in Q.PARAMS:
        h.set_fixed_point(*params)
        Q._same(Q._run(h, pri, None, 50), Q._want(key, "params", None, pri, 50, params), (key, params))
    h.set_fixed_point(*Q.DEFAULT)
    for cap in (1, 2):
        Q._same(Q._run(h, pri, None, cap), Q._want(key, "caps", None, pri, cap), (key, cap))
    want = Q._want(key, "free", None, pri, 7, early=False)
    assert (want[1] == 7).all()
    Q._same(Q._run(h, pri, None, 7, Q.NO_EARLY_EXIT), want, (key, "no early exit"))
    easy = pri[np.flatnonzero(Q._want(key, "params", None, pri, 50)[1] < 50)[:8]]  # frames that leave on their own
    want = Q._want(key, "unbounded", None, easy, 0)
    assert len(easy) == 8 and want[1].max() < 50
    Q._same(Q._run(h, easy, None, 0), want, (key, "max_iter 0"))
    Q._same(Q._run(h, easy, None, -3), want, (key, "max_iter -3"))


# ---------------------------------------------------------------------------------------------- 4. the order of the block rows
@pytest.mark.parametrize("key", [("dense", 21), "irregular 13"], ids=str)
def test_block_row_order(key):
    mb = _code(key)[2].shape[0]
    pri = _batch(key)[0].astype(np.float32)
    h = _handle(key)
    perm = np.random.RandomState(3).permutation(mb)
    assert not np.array_equal(perm, np.arange(mb))
    for name, order in (("reversed", np.arange(mb)[::-1].copy()), ("random", perm)):
        h.set_order(order)
        want = Q._want(key, "order", None, pri, 50, order=order)
        Q._same(Q._run(h, pri, None, 50), want, (key, name))
    natural = Q._want(key, "parity", None, pri, 50)
    assert not np.array_equal(want[1], natural[1]) or not np.array_equal(want[2], natural[2])
    h.set_order(None)
    Q._same(Q._run(h, pri, None, 50), natural, (key, "natural again"))


# ---------------------------------------------------------------------------------------------- 5. batch sizes, refilling slots
@pytest.mark.parametrize("key", [("dense", 7), "4x8"], ids=str)
def test_any_batch_size_and_position(key, monkeypatch):
    P = _rule(key)
    pri = _batch(key, 64)[0].astype(np.float32)
    want = Q._want(key, "parity 64", None, pri, 50)
    h = _handle(key)
    ext = np.concatenate([pri, pri[:1]])
    for B in sorted({1, P - 1, P, P + 1, 63, 64, 65}):
        idx = np.arange(B) % 64
        Q._same(Q._run(h, ext[:B], None, 50), tuple(a[idx] for a in want[:3]), (key, B))
    # two workgroups: every slot refills several times with mixed exit times; a frame gives the same result in any slot at any time
    monkeypatch.setenv("LDPC_QC_PACK_GRID", "2")
    small = _handle(key)
    B = 6 * P + 17
    idx = np.random.RandomState(5).randint(0, 64, size=B)
    assert 0 < (want[1][idx] < 50).sum() < B
    Q._same(Q._run(small, pri[idx], None, 50), tuple(a[idx] for a in want[:3]), (key, "B = %d on two workgroups" % B))


@pytest.mark.parametrize("key,p", [(("dense", 16), 0.07), (("dense", 7), 0.07), ("irregular 13", 0.04), ("loop 8", 0.01)], ids=str)
def test_bsc_received_codewords_in_a_row(key, p, monkeypatch):
    """One workgroup hands the frames out in index order: 3 P received codewords at the head (every slot draws again and again before its
    first sweep) and 2 P more from index 40 (slots that just wrote a decoded frame draw several that leave at once), the rest flipped
    with p.  Frames with 0 sweeps keep y0 and have soft output 0."""
    P = _rule(key)
    g = _code(key)[0]
    B, cap = 64, 50
    y = (np.random.RandomState(9).random_sample((B, g.n)) < p).astype(np.uint8)
    y[:min(3 * P, 40)] = 0
    y[40:40 + min(2 * P, B - 40)] = 0
    monkeypatch.setenv("LDPC_QC_PACK_GRID", "1")
    h = _handle(key)
    for dt in (np.float64, np.float32):
        pri = O.bsc_priors(y.astype(np.int64), p).astype(dt)
        want = Q._want(key, "bsc rows", y, pri, cap)
        kinds = ((want[1] == 0).sum(), (want[1] == cap).sum(), ((want[1] > 0) & (want[1] < cap)).sum())
        assert kinds[0] >= min(3 * P, 40) + min(2 * P, B - 40) and kinds[1] > 0 and kinds[2] > 0, kinds
        got = Q._run(h, pri, y, cap)
        Q._same(got, want, (key, "bsc", dt.__name__, kinds))
        assert not got[3][want[1] == 0].any() and np.array_equal(got[0][want[1] == 0], y[want[1] == 0])
    Q._same(Q._run(h, pri, y, 3, Q.NO_EARLY_EXIT), Q._want(key, "bsc rows free", y, pri, 3, early=False), (key, "bsc, no early exit"))
    want = Q._want(key, "bsc rows no y0", None, pri, cap)
    assert want[1][0] == 1
    Q._same(Q._run(h, pri, None, cap), want, (key, "bsc priors without y0"))


# ---------------------------------------------------------------------------------------------- 6. simulate, the class, the command line
@pytest.mark.parametrize("channel,param", [("biawgn", 2.5), ("bsc", 0.07)])
def test_simulate_equals_channel_decode_count(channel, param):
    """Packed counters == the counters at one frame per workgroup == the oracle's on the priors ldpc_channel writes."""
    import torch

    from ldpc_decoders_amd import _lib

    key, B, cap, frame0, bins = ("dense", 16), 128, 20, 1000, 21
    g = _code(key)[0]
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    pri = torch.empty((B, g.n), dtype=torch.float32, device="cuda")
    y = torch.empty((B, g.n), dtype=torch.uint8, device="cuda") if channel == "bsc" else None
    _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE["f32"], float(param), 0, SEED, STREAM, frame0, B, g.n, pri.data_ptr(),
                                None if y is None else y.data_ptr(), st))
    x, it, _, _ = LQ.lqmsa_decode(g, None if y is None else y.cpu().numpy(), pri.cpu().numpy(), cap, layers=Q._layers(key))
    wrong = x.any(axis=1)
    assert 0 < wrong.sum() < B
    got = {}
    for P in (0, 1):
        h = _handle(key, P)
        cnt = torch.zeros(_lib.CNT_HIST0 + bins, dtype=torch.int64, device="cuda")
        h.simulate(channel, param, 0, SEED, STREAM, frame0, B, cap, cnt, hist_bins=bins)
        got[P] = cnt.cpu().numpy()
    assert np.array_equal(got[0], got[1])
    c = got[0]
    assert c[_lib.CNT_TOT] == B and c[_lib.CNT_WEC] == wrong.sum() and c[_lib.CNT_BEC] == x.sum() and c[_lib.CNT_ITER_SUM] == it.sum()
    assert np.array_equal(c[_lib.CNT_HIST0:], np.bincount(it, minlength=bins))


def test_simulate_random_codewords():
    """codeword = -1 through the packed handle: encoder words, ldpc_channel_sent, decode, ldpc_count_errors_words."""
    import torch

    from ldpc_decoders_amd import _lib

    key, B, cap, frame0 = ("dense", 16), 128, 20, 64
    g, c = _code(key)[:2]
    got = {}
    for P in (0, 1):
        h = _handle(key, P)
        cnt = torch.zeros(_lib.CNT_HIST0, dtype=torch.int64, device="cuda")
        h.simulate("biawgn", 2.5, -1, SEED, STREAM, frame0, B, cap, cnt)
        got[P] = cnt.cpu().numpy()
    assert np.array_equal(got[0], got[1])
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    sent = c.encoder().handle(h.device).encode_random(SEED, STREAM, frame0, B)
    pri = torch.empty((B, g.n), dtype=torch.float32, device="cuda")
    _lib.check(lib.ldpc_channel_sent(_lib.CHANNEL["biawgn"], _lib.DTYPE["f32"], 2.5, sent.data_ptr(), SEED, STREAM, frame0, B, g.n, pri.data_ptr(), None, st))
    x, it, _, _ = LQ.lqmsa_decode(g, None, pri.cpu().numpy(), cap, layers=Q._layers(key))
    s = sent.cpu().numpy()
    assert s.any() and 0 < (x != s).any(axis=1).sum() < B
    assert tuple(got[0][[_lib.CNT_TOT, _lib.CNT_WEC, _lib.CNT_BEC, _lib.CNT_ITER_SUM]]) == (B, (x != s).any(axis=1).sum(), (x != s).sum(), it.sum())


def test_the_class_packs_by_the_rule():
    from ldpc_decoders_amd import qc

    key = "4x8"
    c = _code(key)[1]
    pri = _batch(key)[0].astype(np.float32)
    want = Q._want(key, "parity", None, pri, 50)
    dec = qc.QCMSA(c, max_iter=50)
    assert dec.qc_pack == 0 and dec.handle.pack() == (_rule(key),) * 2 == (2, 2)
    x, it = dec.decode_batch(None, pri)
    assert np.array_equal(x, want[0]) and np.array_equal(it, want[1])
    one = qc.QCMSA(c, max_iter=50, qc_pack=1)
    assert one.handle.pack() == (1, 2)
    x1, it1 = one.decode_batch(None, pri)
    assert np.array_equal(x1, x) and np.array_equal(it1, it)
    with pytest.raises(ValueError, match="Z = 27"):
        qc.QCMSA(c, max_iter=50, qc_pack=3)


def test_cli(tmp_path, monkeypatch):
    """``--qc-pack 1`` and the default (the rule) write the same file name with the same counters."""
    from ldpc_decoders_amd import codes, main, qc

    code_dir = tmp_path / "codes"
    monkeypatch.setenv(codes.file_codes_dir_string, str(code_dir))
    qc.gen_rand_qc(qc.setup_parser().parse_args("1 4 8 27 --seed 5 --dir".split() + [str(code_dir)]))
    argv = "biawgn 216_qc_4x8_z27_1 QCMSA --params 3.0 --max-iter 20 --batch 4096 --max-frames 4096".split()
    res = {}
    for name, extra in (("rule", []), ("one", ["--qc-pack", "1"])):
        out = tmp_path / name
        main.main(argv + extra + ["--data_dir", str(out), "--console"])
        with open(os.path.join(str(out), "biawgn-216_qc_4x8_z27_1-QCMSA-0-100-20-6-2-0.8125-0.0-27.json")) as fp:
            res[name] = json.load(fp)
    assert "qc_pack" not in res["rule"] and res["rule"]["tot"]["3.0"] == 4096 and 4 <= res["rule"]["wec"]["3.0"] < 2048
    for k in ("tot", "wec", "bec"):
        assert res["rule"][k] == res["one"][k], k

"""Layered fixed-point min-sum without a GPU: properties of the integer statement (lqmsa_oracle.py), what ties it to LMSA and to QMSA, the
registry row, the command line, the Python checks, the LDS rule and the ABI."""
import os

import numpy as np
import pytest

import bp_oracle as O
import lmsa_oracle as L
import lqmsa_oracle as LQ
import qmsa_oracle as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _code(name):
    from ldpc_decoders_amd import codes

    if name not in _CACHE:
        c = codes.get_code(name)
        _CACHE[name] = (O.Edges(c.m, c.n, c.edge_chk, c.edge_var), c)
    return _CACHE[name]


def _biawgn(g, snr, B, seed, dt=np.float64):
    rng = np.random.RandomState(seed)
    return O.biawgn_priors(-1 + rng.normal(0, np.sqrt(O.biawgn_noise_var(snr)), (B, g.n)), snr).astype(dt)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_a_hand_worked_example():
    """Two checks on four variables, {0, 1, 2} and {1, 2, 3}: two layers.  bits 6 (V = 31), frac 0, scale 0.75 (scale64 = 48), offset 0,
    levels (5, -3, 2, -7).  Sweep 1, check 0: v = (5, -3, 2) -> c2v = (-(96 >> 6), +(96 >> 6), -(144 >> 6)) = (-1, 1, -2), marg = (4, -2, 0,
    -7); check 1: v = (-2, 0, -7) -> c2v = (0, +1, 0), marg = (4, -2, 1, -7).  Sweep 2, check 0: v = (5, -3, 3) -> (-2, 2, -2), marg =
    (3, -1, 1, -7); check 1: v = (-1, 0, -7) -> (0, (48 >> 6) = 0, 0), marg = (3, -1, 0, -7)."""
    g = O.Edges(2, 4, np.array([0, 0, 0, 1, 1, 1]), np.array([0, 1, 2, 1, 2, 3]))
    assert L.greedy_layers(g).tolist() == [0, 1]
    pri = np.array([[5.0, -3.0, 2.0, -7.0]])
    for one in (False, True):
        x, it, soft, peak = LQ.lqmsa_decode(g, None, pri, 1, bits=6, frac_bits=0, scale=0.75, offset=0, one_by_one=one)
        assert soft.dtype == np.int16 and soft.tolist() == [[4, -2, 1, -7]] and x.tolist() == [[0, 1, 0, 1]] and it.tolist() == [1] and peak == 7
        x, it, soft, peak = LQ.lqmsa_decode(g, None, pri, 2, bits=6, frac_bits=0, scale=0.75, offset=0, one_by_one=one)
        assert soft.tolist() == [[3, -1, 0, -7]] and x.tolist() == [[0, 1, 0, 1]] and it.tolist() == [2] and peak == 7
    # the other order of the two layers: check 1 first.  v = (-3, 2, -7) -> c2v = (-1, +2, -1), marg = (5, -4, 4, -8); check 0: v = (5, -4, 4)
    # -> (-(192 >> 6), +3, -3), marg = (2, -1, 1, -8)
    _, _, soft, _ = LQ.lqmsa_decode(g, None, pri, 1, bits=6, frac_bits=0, scale=0.75, offset=0, layers=[1, 0])
    assert soft.tolist() == [[2, -1, 1, -8]]
    # an offset clamps at 0, a saturated input counts as V: bits 3 (V = 3), levels (3, -3, 2, -3); check 0: a = (3, 3, 2), scale 1, offset 2
    _, _, soft, peak = LQ.lqmsa_decode(g, None, pri, 1, bits=3, frac_bits=0, scale=1.0, offset=2)
    assert soft.tolist() == [[3, -3, 2, -3]] and peak == 3  # check 0: c2v = (0, 0, -(3 - 2)), marg_2 = 1; check 1: v = (-3, 1, -3) -> (0, +(3 - 2), 0)


@pytest.mark.parametrize("name", ["12_3_4_ldpc", "512_3_6_rand_ldpc_1", "1200_rho_x5_rand_ldpc_1"])
def test_one_by_one_equals_the_grouped_schedule(name):
    g = _code(name)[0]
    pri = _biawgn(g, 2.0, 12, 3)
    y0 = (np.random.RandomState(4).random_sample((12, g.n)) < 0.05).astype(np.uint8)
    y0[0] = 0
    for kw in (dict(), dict(bits=3, frac_bits=0, scale=1.0, offset=1), dict(early_exit=False), dict(layers=L.greedy_layers(g)[::-1].copy() if name == "12_3_4_ldpc" else None)):
        for y in (None, y0):
            a = LQ.lqmsa_decode(g, y, pri, 6, **kw)
            b = LQ.lqmsa_decode(g, y, pri, 6, one_by_one=True, **kw)
            assert _same(a, b), (name, kw)
    x, it, soft, _ = LQ.lqmsa_decode(g, y0, pri, 6)
    assert it[0] == 0 and not soft[0].any() and not x[0].any()  # a received codeword leaves at iteration 0


@pytest.mark.parametrize("offset", [0, 1])
def test_scale_one_is_lmsa_on_the_levels(offset):
    """With scale 1 and an integer offset the rule is LMSA's on integers, as long as no |v_j| exceeds V (the clip min(|v_j|, V) is then
    the identity): decisions, iteration counts and soft outputs equal lmsa_oracle.lmsa_decode in fp64 on the levels.  bits 8, frac 0
    clips the priors at +-127; the levels are scaled down so that the messages stay inside."""
    g = _code("512_3_6_rand_ldpc_1")[0]
    pri = _biawgn(g, 2.5, 48, 11)
    level = Q.quantise(pri * 0.75, 8, 0)  # integer priors; quantising them again changes nothing
    assert np.abs(level).max() <= 40
    x, it, soft, peak = LQ.lqmsa_decode(g, None, level, 50, bits=8, frac_bits=0, scale=1.0, offset=offset)
    assert peak <= Q.vmax_of(8), peak
    xr, itr, softr = L.lmsa_decode(g, None, level, 50, 1.0, float(offset), dtype=np.float64)
    assert np.array_equal(x, xr) and np.array_equal(it, itr) and np.array_equal(soft.astype(np.float64), softr)
    assert 0 < (it < 50).sum() and len(np.unique(it)) > 3


def test_what_the_schedule_is_worth():
    """48 BI-AWGN frames of 1200_3_6_rand_ldpc_1 at 2.0 dB (RandomState 2024), cap 50, bits 6, frac 2, scale 0.8125, offset 0:
    LQMSA 7.27 sweeps per frame, QMSA (flooding) 12.81, one word error each.  The device is held to the oracle exactly, so the value of
    the layered schedule is pinned here."""
    g = _code("1200_3_6_rand_ldpc_1")[0]
    pri = _biawgn(g, 2.0, 48, 2024)
    x, it, _, _ = LQ.lqmsa_decode(g, None, pri, 50)
    xq, itq, _, _ = Q.qmsa_decode(g, None, pri, 50, bits=6, frac_bits=2, scale=0.8125, offset=0)
    print("mean sweeps: LQMSA %.2f, QMSA %.2f; word errors %d, %d" % (it.mean(), itq.mean(), x.any(axis=1).sum(), xq.any(axis=1).sum()))
    assert it.mean() < itq.mean()
    assert x.any(axis=1).sum() <= xq.any(axis=1).sum() + 1


def test_registry_row_parser_and_channel_classes(tmp_path):
    from ldpc_decoders_amd import bec, biawgn, bsc, layered, main, models, registry, utils

    assert models.layered_fixed_point_decoder_names == ["LQMSA"] and utils.layered_fixed_point_decoder_names is models.layered_fixed_point_decoder_names
    row = registry.BY_NAME["LQMSA"]
    assert registry.ROWS[-2] is row and registry.ROWS[-1].name == "GALB" and row.group == "layered_fixed_point" and row.integer_layered
    assert row.bec_refusal is None and row.prior_grid is None and row.backing is layered.LQMSA
    assert not (row.device_words or row.tie_dominated or row.f16 or row.osd_front or row.pops_layers or row.refuses_fused or row.hard)
    assert [r.name for r in registry.ROWS if r.integer_layered] == ["LQMSA"]
    assert "LQMSA" in models.all_decoder_names and "LQMSA" not in registry.osd_fronts()
    args = main.build_parser().parse_args("biawgn 512_3_6_rand_ldpc_1 LQMSA --msa-bits 5 --msa-frac-bits 1 --msa-scale 0.75 --msa-offset 1 --max-iter 20".split())
    assert (args.decoder, args.msa_bits, args.msa_frac_bits, args.msa_scale, args.msa_offset) == ("LQMSA", 5, 1, 0.75, 1.0)
    keys = ["max_iter", "msa_bits", "msa_frac_bits", "msa_scale", "msa_offset"]
    assert bsc.LQMSA.id_keys == biawgn.LQMSA.id_keys == bec.LQMSA.id_keys == layered.LQMSA.id_keys == keys
    assert bsc.LQMSA.__module__.endswith(".bsc") and biawgn.LQMSA.__module__.endswith(".biawgn") and bec.LQMSA.__module__.endswith(".bec")
    assert issubclass(biawgn.LQMSA, biawgn.LLR) and issubclass(bsc.LQMSA, bsc.LLR)
    with pytest.raises(NotImplementedError) as e:
        bec.LQMSA(0.1, None, max_iter=1)
    assert "does not exist over the bec" in str(e.value) and "SPA / MSA" in str(e.value)
    # the result file: <channel>-<code>-<decoder>-<codeword>-<min_wec>-<max_iter>-<bits>-<frac>-<scale>-<offset>.json
    id_keys = ["channel", "code", "decoder", "codeword", "min_wec"] + biawgn.LQMSA.id_keys
    saver = utils.Saver(str(tmp_path), [(k, vars(args)[k]) for k in id_keys])
    assert os.path.basename(saver.file_path) == "biawgn-512_3_6_rand_ldpc_1-LQMSA-0-100-20-5-1-0.75-1.0.json"
    helps = main.build_parser().format_help()
    assert helps.count("LQMSA") >= 4


@pytest.mark.parametrize("argline,needle", [
    ("biawgn 512_3_6_rand_ldpc_1 LQMSA --precision f16", "--precision f16"),
    ("biawgn 512_3_6_rand_ldpc_1 LQMSA --prior-grid 4", "--prior-grid"),
    ("bsc 512_3_6_rand_ldpc_1 LQMSA --backend stream", "--backend stream"),
])
def test_the_driver_refuses_before_a_decoder_exists(argline, needle, tmp_path, monkeypatch):
    from ldpc_decoders_amd import layered, main

    def no_decoder(*a, **k):
        raise AssertionError("a decoder was built")

    monkeypatch.setattr(layered.LQMSA, "__init__", no_decoder)
    args = main.build_parser().parse_args(argline.split() + ["--data_dir", str(tmp_path), "--console"])
    with pytest.raises(SystemExit) as e:
        main.test(args)
    assert needle in str(e.value)


@pytest.mark.parametrize("backend", ["auto", "fused"])
def test_the_driver_accepts_auto_and_fused_and_drops_layers(backend, tmp_path, monkeypatch):
    """--backend auto / fused reach the constructor; --layers (ADMMA's network shape) does not."""
    from ldpc_decoders_amd import layered, main

    seen = {}

    def stop(self, parity_mtx, **k):
        seen.update(k)
        raise KeyboardInterrupt

    monkeypatch.setattr(layered.LQMSA, "__init__", stop)
    args = main.build_parser().parse_args(("biawgn 512_3_6_rand_ldpc_1 LQMSA --params 2.5 --backend %s" % backend).split() + ["--data_dir", str(tmp_path), "--console"])
    with pytest.raises(KeyboardInterrupt):
        main.test(args)
    assert "layers" not in seen and seen["backend"] == backend and seen["msa_bits"] == 6 and seen["precision"] == "f32"


def test_parameters_are_checked_in_python(monkeypatch):
    from ldpc_decoders_amd import _lib, layered

    assert layered.check_params(6, 2, 0.8125, 0) == (6, 2, 0.8125, 0) and layered.check_params(2, -8, 1 / 64, 7) == (2, -8, 1 / 64, 7)
    assert layered.check_params(8, 8, 1.0, 3.0) == (8, 8, 1.0, 3)
    for bad in ((9, 2, 0.8125, 0), (1, 2, 0.8125, 0), (6, 9, 0.8125, 0), (6, -9, 0.8125, 0), (6, 2, 0.8, 0), (6, 2, 0.0, 0), (6, 2, 1.015625, 0),
                (6, 2, 0.8125, -1), (6, 2, 0.8125, 0.5), (6.5, 2, 0.8125, 0), (6, 2, float("nan"), 0)):
        with pytest.raises(ValueError):
            layered.check_params(*bad)

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    code = _code("512_3_6_rand_ldpc_1")[1]
    for kw in (dict(msa_bits=9), dict(msa_scale=0.8), dict(msa_offset=-1), dict(precision="f16"), dict(backend="stream"),
               dict(layers=np.zeros(code.m, dtype=np.int64)), dict(layers=np.arange(code.m - 1))):
        with pytest.raises(ValueError):
            layered.LQMSA(code, max_iter=5, **kw)
    # the LDS rule and the degree rule, on synthetic codes (weight-6 rows): 2 n + 8 m + 16 on either side of 160 KiB
    import edge_codes as EC

    m_ok = (layered.LDS_BYTES - 16 - 2 * 4096) // 8
    assert layered.lqmsa_lds_bytes(m_ok, 4096, 6 * m_ok, 6) == layered.LDS_BYTES and layered.lqmsa_lds_bytes(m_ok + 1, 4096, 6 * m_ok + 6, 6) > layered.LDS_BYTES
    with pytest.raises(ValueError) as e:
        layered.LQMSA(EC.limit_code(m_ok + 1, 4096), max_iter=5)
    assert "LMSA" in str(e.value)
    with pytest.raises(AssertionError):  # the accepted side passes every Python check and reaches the library
        layered.LQMSA(EC.limit_code(m_ok, 4096), max_iter=5)
    with pytest.raises(ValueError):  # a check of degree 1
        layered.LQMSA(np.array([[1, 1, 0], [0, 0, 1]]), max_iter=5)
    with pytest.raises(ValueError) as e:  # (3, 6) at n = 64 800
        layered.check_code(type("C", (), dict(m=32400, n=64800, E=194400, edge_chk=np.repeat(np.arange(32400), 6), edge_var=np.arange(194400) % 64800))())
    assert "LMSA" in str(e.value)


def test_the_size_rule():
    from ldpc_decoders_amd import layered

    assert [layered.lqmsa_row_bytes(d) for d in (2, 6, 8, 9, 12, 13, 33, 64)] == [8, 8, 8, 12, 12, 16, 36, 64]
    assert layered.lqmsa_lds_bytes(600, 1200, 3600, 6) == 2400 + 4800 + 16
    assert layered.lqmsa_lds_bytes(9, 31, 60, 7) == 64 + 72 + 16  # 62 bytes of marginals rounded up to 64
    assert [layered.lqmsa_waves(f) for f in (1, 2, 3, 4, 7, 8, 15, 16, 22, 31, 32, 400)] == [8, 8, 8, 8, 8, 4, 4, 2, 2, 2, 1, 1]
    # rate-1/2 irregular n = 10 000 (BASELINE config 4): m = 5000 checks of degree <= 8 fit; (3, 6) at n = 64 800 does not
    assert layered.lqmsa_lds_bytes(5000, 10000, 40000, 8) <= layered.LDS_BYTES
    assert layered.lqmsa_lds_bytes(5000, 10000, 60000, 20) <= layered.LDS_BYTES
    assert layered.lqmsa_lds_bytes(32400, 64800, 194400, 6) > layered.LDS_BYTES
    # the header states the same formula
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "ldpc_lqmsa.hpp")) as fp:
        text = fp.read()
    assert "(2 * (int64_t)n + 7) / 8 * 8 + (int64_t)m * lqmsa_row_bytes(dc_max) + 16" in text and "dc_max <= 8 ? 8 : (dc_max + 3) / 4 * 4" in text


def test_every_shipped_code_fits_the_lds_rule():
    from ldpc_decoders_amd import codes, layered

    names = [n for n in codes.get_code_names() if os.path.exists(os.path.join(ROOT, "ldpc_decoders_amd", "data", "codes", n + ".txt"))]
    assert len(names) == 27 and "margulis" in names
    for name in names:
        c = codes.get_code(name)
        layered.check_code(c)
        assert layered.lqmsa_lds_bytes(c.m, c.n, c.E, int(c.row_degrees().max())) <= layered.LDS_BYTES, name
        assert c.col_degrees().max() <= layered.MAX_DV and c.n <= 65536


def test_the_abi_declares_and_binds_the_family():
    import re

    from ldpc_decoders_amd import _lib

    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as fp:
        text = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    declared = set(re.findall(r"\b(ldpc_lqmsa_[a-z0-9_]+)\s*\(", text))
    assert declared == {"ldpc_lqmsa_create", "ldpc_lqmsa_destroy", "ldpc_lqmsa_set_fixed_point", "ldpc_lqmsa_get_fixed_point", "ldpc_lqmsa_set_layers",
                        "ldpc_lqmsa_get_layers", "ldpc_lqmsa_decode", "ldpc_lqmsa_simulate", "ldpc_lqmsa_info"}
    assert declared <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["ldpc_lqmsa_decode"][1]) == 12 and len(_lib.SIGNATURES["ldpc_lqmsa_simulate"][1]) == 13
    assert "LQMSA" not in _lib.ALG  # a handle family of its own, not an algorithm of ldpc_decoder_create

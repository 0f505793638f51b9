"""Fixed-point min-sum (LDPC_ALG_QMSA), everything that needs no GPU: the CPU restatement (tests/qmsa_oracle.py) in float64, in float32 and
as an all-integer statement on the reference's golden min-sum inputs, the commutation of the clamp / floor / offset map with the minimum,
what the bits are worth, the registry / parser / result-file surface, the parameter checks, and the built library's kernel set (every
min-sum kernel has its fixed-point sibling, the variable pass has none)."""
import os
import re
import sys

import numpy as np
import pytest

import bp_oracle as O
import nmsa_oracle as N
import qmsa_oracle as Q
from helpers import case_id, decode_cases, golden_edges, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSA_CASES = decode_cases("biawgn_MSA_*") + decode_cases("bsc_MSA_*")
# (bits, frac_bits, scale, offset): the default, 5-bit offset min-sum, and a word so short that everything saturates
SETTINGS = [(6, 2, 0.8125, 0), (5, 1, 1.0, 1), (3, 0, 1.0, 0)]


def _case_inputs(c):
    if c["channel"] == "biawgn":
        return None, O.biawgn_priors(c["y"].astype(np.float64), c["param"])
    y = c["y"].astype(np.int64)
    return y, O.bsc_priors(y, c["param"])


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("bits,frac,scale,offset", SETTINGS)
@pytest.mark.parametrize("path", MSA_CASES, ids=case_id)
def test_float64_float32_and_the_integer_statement_agree(path, bits, frac, scale, offset):
    """Every value is a small integer: the rule computed in float64, in float32 and with ``//`` on integers is one and the same function of
    the (fp32-representable) priors -- decisions, iteration counts and marginals.  A few frames of each golden min-sum input."""
    c = load_case(path)
    assert MSA_CASES and c["decoder"] == "MSA"
    g = golden_edges(c["code"])
    y0, pri = _case_inputs(c)
    F = min(len(pri), 3 if g.n > 100 else 16)
    pri = pri[:F].astype(np.float32)  # what an fp32 decoder is handed; float64 holds the same values
    y0 = None if y0 is None else y0[:F]
    x64, i64, s64, _ = Q.qmsa_decode(g, y0, pri, c["max_iter"], bits, frac, scale, offset, np.float64)
    x32, i32, s32, _ = Q.qmsa_decode(g, y0, pri, c["max_iter"], bits, frac, scale, offset, np.float32)
    assert s32.dtype == np.float32 and (x64 == x32).all() and (i64 == i32).all() and np.array_equal(s64, s32.astype(np.float64))
    levels = Q.quantise(pri.astype(np.float64), bits, frac)
    assert (np.abs(levels) <= Q.vmax_of(bits)).all() and (levels == np.rint(levels)).all()
    for f in range(F):
        xi, ii, si = Q.qmsa_decode_int(g, None if y0 is None else y0[f], levels[f].astype(np.int64), c["max_iter"], bits, int(round(64 * scale)), offset)
        assert (xi == x64[f]).all() and ii == i64[f] and np.array_equal(si, s64[f].astype(np.int64)), (f, ii, i64[f])


def test_quantiser_edges():
    """Half-levels go to the even neighbour, values beyond the range and +-inf saturate, -0 comes out as +0; the input is not modified."""
    p = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.25, -0.25, 0.75, 100.0, -100.0, np.inf, -np.inf, 15.5, 16.5, -0.0], dtype=np.float32)
    keep = p.copy()
    q = Q.quantise(p, 5, 0)  # V = 15
    assert np.array_equal(q, np.array([0, 2, 2, 0, -2, -2, 0, 0, 1, 15, -15, 15, -15, 15, 15, 0], dtype=np.float32))
    assert not np.signbit(q[[0, 3, 6, 7, 15]]).any() and np.array_equal(p, keep, equal_nan=True)
    assert np.array_equal(Q.quantise(p, 5, 1)[:9], np.array([1, 3, 5, -1, -3, -5, 0, 0, 2], dtype=np.float32))  # 0.25 * 2 = 0.5 -> 0, 0.75 * 2 = 1.5 -> 2
    assert np.array_equal(Q.quantise(np.array([5.0, 6.0, 7.0, -6.0]), 6, -2), np.array([1.0, 2.0, 2.0, -2.0]))  # a level of 4: 1.25, 1.5, 1.75


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bits,scale,offset", [(6, 0.8125, 0), (5, 1.0, 1), (4, 0.75, 0), (3, 1.0, 0), (12, 1.0, 0), (8, 0.015625, 0), (6, 0.5, 3)])
def test_fixing_inputs_before_the_minimum_equals_fixing_outputs_after_it(dtype, bits, scale, offset):
    """x -> max(floor(scale min(x, V)) - offset, 0) is monotone non-decreasing, so it commutes with min exactly: the kernels may apply it to
    the d inputs of their minimum network or to its outputs.  Random integer rows with ties, zeros and +inf (padding positions, empty
    minima) -- and clamping the inputs to V first changes nothing."""
    V = Q.vmax_of(bits)
    rng = np.random.RandomState(5)
    rows = np.floor(rng.exponential(V / 2.0 + 1.0, (20000, 6))).astype(dtype)  # a good part beyond V
    rows[rng.random_sample(rows.shape) < 0.15] = 0.0
    rows[rng.random_sample(rows.shape) < 0.10] = np.inf
    tie = rng.random_sample(rows.shape[0]) < 0.3
    rows[tie, 1] = rows[tie, 4]
    rows[::101] = np.inf
    for j in range(6):
        others = np.delete(rows, j, axis=1)
        after = Q.fix(others.min(axis=1), scale, offset, V)
        before = Q.fix(others, scale, offset, V).min(axis=1)
        clamped = Q.fix(np.minimum(others, dtype(V)).min(axis=1), scale, offset, V)
        assert after.dtype == dtype and np.array_equal(after, before) and np.array_equal(after, clamped)
        assert (after == np.floor(after)).all() and after.max() <= V
        empty = np.isinf(others).all(axis=1)
        assert empty.any() and (after[empty] == max(int(np.floor(scale * V)) - offset, 0)).all()  # an empty minimum: floor(scale V) - offset
    ints = np.arange(0, V + 1)
    assert np.array_equal(Q.fix(ints.astype(dtype), scale, offset, V), np.maximum((int(round(64 * scale)) * ints) // 64 - offset, 0).astype(dtype))


@pytest.fixture(scope="module")
def table_frames():
    """The issue's frames: 1200_3_6_rand_ldpc_1, BI-AWGN at 2.0 dB, all-zero word, np.random.RandomState(11); the first 256 of the 1 024."""
    g = golden_edges("1200_3_6_rand_ldpc_1")
    var = 10 ** -0.2
    y = -1 + np.random.RandomState(11).normal(0, np.sqrt(var), (1024, g.n))[:256]
    return g, -2 * y / var


def test_what_the_bits_are_worth_at_2_dB(table_frames):
    """On all 1 024 frames: float plain min-sum 160 word errors, q = 8 (k = 4, 0.8125) 8, q = 6 (k = 2, 0.8125) 10, q = 5 (k = 1, 0.8125)
    25, q = 4 (k = 0, 0.75) 544.  The first 256 of those frames here; the orderings hold with room."""
    g, pri = table_frames
    xp, _, _ = N.nmsa_decode(g, None, pri, 50, 1.0, 0.0)  # (1, 0): the reference's plain min-sum, float64
    wec = {"plain": int(xp.any(axis=1).sum())}
    for name, (bits, frac, scale) in dict(q8=(8, 4, 0.8125), q6=(6, 2, 0.8125), q5=(5, 1, 0.8125), q4=(4, 0, 0.75)).items():
        x, it, _, peak = Q.qmsa_decode(g, None, pri, 50, bits, frac, scale, 0, np.float32)
        wec[name] = int(x.any(axis=1).sum())
        assert peak <= Q.vmax_of(bits) * (1 + 3)  # |marginal| <= V (1 + dv)
    print("word errors of 256:", wec)
    assert wec["plain"] > 0 and wec["q6"] * 4 < wec["plain"]
    assert wec["q8"] <= wec["q5"] <= wec["q4"]


# ---------------------------------------------------------------------------------------------- registry, parser, result file
def test_registry_parser_and_result_file(tmp_path):
    from ldpc_decoders_amd import bec, biawgn, bpa, bsc, main, models, utils

    assert models.extra_decoder_names == ["NMSA"] and models.fixed_point_decoder_names == ["QMSA"]
    assert utils.fixed_point_decoder_names == ["QMSA"]
    keys = ["max_iter", "msa_bits", "msa_frac_bits", "msa_scale", "msa_offset"]
    for cls in (bpa.QMSA, biawgn.QMSA, bsc.QMSA, bec.QMSA):
        assert cls.id_keys == keys
    p = main.build_parser()
    a = p.parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "QMSA", "--params", "2.0", "--max-iter", "50", "--min-wec", "50"])
    assert (a.decoder, a.msa_bits, a.msa_frac_bits, a.msa_scale, a.msa_offset) == ("QMSA", 6, 2, 0.8125, 0.0)
    # --msa-scale / --msa-offset are NMSA's flags, types and defaults unchanged
    b = p.parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA"])
    assert (b.msa_scale, b.msa_offset) == (0.8125, 0.0) and isinstance(b.msa_offset, float)
    with pytest.raises(SystemExit):
        utils.setup_parser(["1200_3_6_rand_ldpc_1"], ["biawgn"], utils.decoder_names + utils.extra_decoder_names).parse_args(
            ["biawgn", "1200_3_6_rand_ldpc_1", "QMSA"])
    # result file: <channel>-<code>-QMSA-<codeword>-<min_wec>-<max_iter>-<bits>-<frac>-<scale>-<offset>.json, values through str()
    a = p.parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "QMSA", "--params", "2.0", "--max-iter", "50", "--min-wec", "30", "--msa-bits", "5",
                      "--msa-frac-bits", "1", "--msa-scale", "1", "--msa-offset", "1"])
    id_keys = ["channel", "code", "decoder", "codeword", "min_wec"] + getattr(models.models[a.channel], a.decoder).id_keys
    saver = utils.Saver(str(tmp_path), [(k, vars(a)[k]) for k in id_keys])
    assert os.path.basename(saver.file_path) == "biawgn-1200_3_6_rand_ldpc_1-QMSA-0-30-50-5-1-1.0-1.0.json"
    with pytest.raises(NotImplementedError):
        bec.QMSA(0.4, None, max_iter=10)
    with pytest.raises(NotImplementedError):
        getattr(models.models["bec"], "QMSA")(0.4, None, max_iter=10)


def test_prior_grid_with_qmsa_is_refused(tmp_path):
    from ldpc_decoders_amd import main

    a = main.build_parser().parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "QMSA", "--prior-grid", "4", "--data_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="--prior-grid: fp32 min-sum over BI-AWGN"):
        main.test(a)


@pytest.mark.parametrize("bits,frac,scale,offset", [(1, 2, 0.8125, 0), (13, 2, 0.8125, 0), (6, 2, 0.8, 0), (6, 2, 0.0, 0), (6, 2, 1.02, 0),
                                                    (6, 2, 0.8125, 0.5), (6, 2, 0.8125, -1), (6, 9, 0.8125, 0), (6, -9, 0.8125, 0),
                                                    (6.5, 2, 0.8125, 0), (6, 2, float("nan"), 0), (6, 2, 0.8125, float("inf"))])
def test_out_of_range_parameters_raise_before_any_gpu_call(bits, frac, scale, offset, monkeypatch):
    from ldpc_decoders_amd import _device, _lib, biawgn, bpa

    def no_gpu(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(bpa, "DecoderHandle", no_gpu)
    H = np.array([[1, 1, 0, 1, 1, 0, 0], [1, 0, 1, 1, 0, 1, 0], [0, 1, 1, 1, 0, 0, 1]])
    kw = dict(max_iter=10, msa_bits=bits, msa_frac_bits=frac, msa_scale=scale, msa_offset=offset)
    with pytest.raises(ValueError):
        bpa.QMSA(H, **kw)
    with pytest.raises(ValueError):
        biawgn.QMSA(2.0, H, **kw)
    with pytest.raises(ValueError):
        _device.check_fixed_point(bits, frac, scale, offset)


def test_parameters_in_range_pass_the_check():
    from ldpc_decoders_amd import _device

    assert _device.check_fixed_point(6, 2, 0.8125, 0) == (6, 2, 0.8125, 0)
    assert _device.check_fixed_point(2, -8, 1 / 64, 0.0) == (2, -8, 0.015625, 0)
    assert _device.check_fixed_point(12, 8, 1, 7.0) == (12, 8, 1.0, 7)


# ---------------------------------------------------------------------------------------------- the built library
def test_every_min_sum_kernel_has_its_fixed_point_sibling():
    """k_fused_bp<0, ..>, k_fused_f64<0, ..>, k_cn<T, 0, ..>, k_cn16<0, ..> -> the same name with algorithm 4 and otherwise equal template
    arguments; no k_vn / k_vn16 for algorithm 4 (the variable pass does not depend on the rule); the quantiser of the streaming backend."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    names = set(kernel_resources.kernel_code_hashes())
    assert len(names) > 100, "code objects of libldpc_hip.so not found"
    plain, want = [], []
    for nm in names:
        m = re.match(r"(k_fused_bp|k_fused_f64|k_cn16)<0, (.*)>$", nm)
        if m:
            plain.append(nm), want.append("%s<4, %s>" % m.groups())
        m = re.match(r"k_cn<(float|double), 0, (.*)>$", nm)
        if m:
            plain.append(nm), want.append("k_cn<%s, 4, %s>" % m.groups())
    assert len(plain) >= 60, plain
    missing = sorted(w for w in want if w not in names)
    assert not missing, "min-sum kernels without a fixed-point sibling: %s" % missing
    for nm in names:
        m = re.match(r"(k_fused_bp|k_fused_f64|k_cn16)<4, (.*)>$", nm)
        if m:
            assert "%s<0, %s>" % m.groups() in names, nm
    assert not [nm for nm in names if re.match(r"k_vn<(float|double), 4,|k_vn16<4,", nm)]
    assert {"k_quantise_tile<float>", "k_quantise_tile<double>"} <= names


def test_fixed_point_simulate_kernels_do_not_spill_more_than_their_corrected_siblings():
    """The Monte-Carlo LDS kernels of algorithm 4 against those of algorithm 3 (same shapes, same register tuning): no more spilled
    registers, no more scratch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    ks = kernel_resources.kernels_of()
    seen = 0
    for nm, r in ks.items():
        m = re.match(r"(k_fused_bp|k_fused_f64)<4, (.*true.*)>", nm)  # <ALG, DC, DV, CRW, VRW, NW, SIM, ..>: the Monte-Carlo variants
        if not m:
            continue
        sib = ks[nm.replace("%s<4, " % m.group(1), "%s<3, " % m.group(1), 1)]
        assert (r["spill"] or 0) <= (sib["spill"] or 0) and (r["scratch"] or 0) <= (sib["scratch"] or 0), (nm, r, sib)
        seen += 1
    assert seen >= 22

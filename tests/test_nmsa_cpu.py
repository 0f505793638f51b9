"""Corrected (normalised / offset) min-sum, everything that needs no GPU: the CPU restatement (tests/nmsa_oracle.py) against the
reference's golden min-sum cases and both oracles, the commutation of the correction with the minimum, what the correction is worth, the
registry / parser / result-file surface, and the built library's kernel set (every min-sum kernel has its corrected sibling; the kernels
profiles/roofline_counters.json prices are still the ones it was collected on)."""
import json
import os
import re
import sys

import numpy as np
import pytest

import bp_oracle as O
import c_oracle as C
import nmsa_oracle as N
from helpers import case_id, decode_cases, expected_xhat, golden_edges, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSA_CASES = decode_cases("biawgn_MSA_*") + decode_cases("bsc_MSA_*")


def _case_inputs(c):
    if c["channel"] == "biawgn":
        y = c["y"].astype(np.float64)
        return None, O.biawgn_priors(y, c["param"]), y
    y = c["y"].astype(np.int64)
    return y, O.bsc_priors(y, c["param"]), y.astype(np.float64)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("path", MSA_CASES, ids=case_id)
def test_identity_correction_reproduces_the_reference_min_sum(path):
    """(1, 0) in fp64: the reference's own decisions, iteration counts and recorded sum_cols traces; bit for bit bp_oracle.bp_decode."""
    c = load_case(path)
    assert MSA_CASES and c["decoder"] == "MSA"
    g = golden_edges(c["code"])
    y0, pri, y_raw = _case_inputs(c)
    xh, it, soft = N.nmsa_decode(g, y0, pri, c["max_iter"], 1.0, 0.0, np.float64)
    keep = np.setdiff1d(np.arange(len(pri)), c["raw_rows"])  # (rows the reference returned as the raw BI-AWGN word at iteration 0: none recorded)
    assert (xh[keep] == expected_xhat(c)[keep]).all() and (it[keep] == c["iters"][keep]).all()
    xo, io, trace = O.bp_decode(g, "MSA", y_raw, pri, c["max_iter"], return_trace=True)
    assert (xh[keep] == xo[keep]).all() and (it == io).all()
    # soft output == the oracle's marginals of each frame's last executed sweep, bit for bit
    for f in range(len(pri)):
        if it[f] > 0:
            assert np.array_equal(soft[f], trace[it[f] - 1][f])
    tr = c["sumcols_trace"]
    for f in range(tr.shape[0]):
        for j in range(min(tr.shape[1], c["max_iter"])):
            _, itj, sj = N.nmsa_decode(g, None if y0 is None else y0[f], pri[f], j + 1, 1.0, 0.0, np.float64)
            if itj[0] == j + 1:
                assert np.array_equal(sj[0], pri[f] + tr[f, j])


@pytest.mark.parametrize("path", MSA_CASES, ids=case_id)
def test_identity_correction_equals_the_c_oracle_in_fp32(path):
    c = load_case(path)
    g = golden_edges(c["code"])
    y0, pri, _ = _case_inputs(c)
    xh, it, _ = N.nmsa_decode(g, y0, pri, c["max_iter"], 1.0, 0.0, np.float32)
    xc, ic = C.bp_decode(g, "MSA", None if y0 is None else y0.astype(np.float32), pri, c["max_iter"], dtype=np.float32)
    assert (xh == xc).all() and (it == ic).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("scale,offset", [(0.8125, 0.0), (0.75, 0.0), (1.0, 0.5), (0.875, 0.125), (1.0, 0.0), (0.3, 2.0)])
def test_correcting_inputs_before_the_minimum_equals_correcting_outputs_after_it(dtype, scale, offset):
    """x -> max(fl(fl(scale x) - offset), 0) is monotone non-decreasing, rounding included, so it commutes with min exactly: the kernels
    may correct the d inputs of their minimum network or its d outputs.  Random rows with ties, zeros, +inf (padding positions) and
    denormals."""
    rng = np.random.RandomState(5)
    rows = rng.exponential(3.0, (20000, 6)).astype(dtype)
    rows[rng.random_sample(rows.shape) < 0.15] = 0.0
    rows[rng.random_sample(rows.shape) < 0.10] = np.inf
    tie = rng.random_sample(rows.shape[0]) < 0.3
    rows[tie, 1] = rows[tie, 4]
    rows[::97, 2] = np.finfo(dtype).tiny * dtype(0.37)
    rows[::89] *= dtype(1e-3)
    a, b = dtype(scale), dtype(offset)
    for j in range(6):
        others = np.delete(rows, j, axis=1)
        after = N.correct(others.min(axis=1), a, b)
        before = N.correct(others, a, b).min(axis=1)
        assert after.dtype == dtype and np.array_equal(after, before)
        assert (after[np.isinf(others).all(axis=1)] == np.inf).all()  # a row of padding positions only: +inf stays +inf
    if (scale, offset) == (1.0, 0.0):
        assert np.array_equal(N.correct(rows, a, b), rows)  # the identity on magnitudes, +inf included


def test_what_the_correction_is_worth_at_2_dB():
    """The 2.0 dB row of the issue's table from its seed (np.random.RandomState(11), all-zero word, 1200_3_6_rand_ldpc_1, 50 sweeps,
    fp64): plain min-sum 160 word errors in 1 024 frames, scale 0.8125 eight.  The first 512 of those frames here (the margin holds)."""
    g = golden_edges("1200_3_6_rand_ldpc_1")
    B, snr = 512, 2.0
    var = 10 ** (-snr / 10)
    y = -1 + np.random.RandomState(11).normal(0, np.sqrt(var), (1024, g.n))[:B]
    pri = -2 * y / var
    xp, ip, _ = N.nmsa_decode(g, None, pri, 50, 1.0, 0.0)
    xn, inn, _ = N.nmsa_decode(g, None, pri, 50, 0.8125, 0.0)
    wec_plain, wec_corr = int(xp.any(axis=1).sum()), int(xn.any(axis=1).sum())
    print("word errors of %d: plain %d, scale 0.8125 %d; mean sweeps %.2f / %.2f" % (B, wec_plain, wec_corr, ip.mean(), inn.mean()))
    assert wec_plain > 0 and wec_corr * 4 < wec_plain
    assert inn.sum() < ip.sum()


# ---------------------------------------------------------------------------------------------- registry, parser, result file
def test_registry_parser_and_result_file(tmp_path):
    from ldpc_decoders_amd import bec, biawgn, bpa, bsc, main, models, utils

    assert models.decoder_names == ["ML", "SPA", "MSA", "LP", "ADMM", "ADMMA"] and models.extra_decoder_names == ["NMSA"]
    assert utils.decoder_names == models.decoder_names and utils.extra_decoder_names == ["NMSA"]
    assert bpa.MSA.id_keys == ["max_iter"]
    for cls in (bpa.NMSA, biawgn.NMSA, bsc.NMSA):
        assert cls.id_keys == ["max_iter", "msa_scale", "msa_offset"]
    p = main.build_parser()
    a = p.parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA", "--params", "2.0", "--max-iter", "50", "--min-wec", "50"])
    assert (a.decoder, a.msa_scale, a.msa_offset) == ("NMSA", 0.8125, 0.0)
    a = p.parse_args(["bsc", "1200_3_6_rand_ldpc_1", "NMSA", "--msa-scale", "0.75", "--msa-offset", "0.25", "--data_dir", str(tmp_path)])
    assert (a.msa_scale, a.msa_offset) == (0.75, 0.25)
    # the parser of the reference's grammar alone does not know the name (simulations.py's arg-lines never carry it)
    with pytest.raises(SystemExit):
        utils.setup_parser(["1200_3_6_rand_ldpc_1"], ["biawgn"], utils.decoder_names).parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA"])
    # result file: <channel>-<code>-NMSA-<codeword>-<min_wec>-<max_iter>-<scale>-<offset>.json, values through str()
    a = p.parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA", "--params", "2.0", "--max-iter", "50", "--min-wec", "50", "--msa-scale", "0.8125"])
    id_keys = ["channel", "code", "decoder", "codeword", "min_wec"] + getattr(models.models[a.channel], a.decoder).id_keys
    saver = utils.Saver(str(tmp_path), [(k, vars(a)[k]) for k in id_keys])
    assert os.path.basename(saver.file_path) == "biawgn-1200_3_6_rand_ldpc_1-NMSA-0-50-50-0.8125-0.0.json"
    with pytest.raises(NotImplementedError):
        bec.NMSA(0.4, None, max_iter=10)
    with pytest.raises(NotImplementedError):
        getattr(models.models["bec"], "NMSA")(0.4, None, max_iter=10)


def test_prior_grid_with_nmsa_is_refused(tmp_path):
    from ldpc_decoders_amd import main

    a = main.build_parser().parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "NMSA", "--prior-grid", "4", "--data_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="--prior-grid: fp32 min-sum over BI-AWGN"):
        main.test(a)


@pytest.mark.parametrize("scale,offset", [(0.0, 0.0), (-0.5, 0.0), (1.0000001, 0.0), (float("nan"), 0.0), (float("inf"), 0.0),
                                          (0.8, -0.1), (0.8, float("inf")), (0.8, float("nan"))])
def test_out_of_range_correction_raises_before_any_gpu_call(scale, offset, monkeypatch):
    from ldpc_decoders_amd import _device, _lib, biawgn, bpa

    def no_gpu(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_gpu)
    monkeypatch.setattr(bpa, "DecoderHandle", no_gpu)
    H = np.array([[1, 1, 0, 1, 1, 0, 0], [1, 0, 1, 1, 0, 1, 0], [0, 1, 1, 1, 0, 0, 1]])
    with pytest.raises(ValueError):
        bpa.NMSA(H, max_iter=10, msa_scale=scale, msa_offset=offset)
    with pytest.raises(ValueError):
        biawgn.NMSA(2.0, H, max_iter=10, msa_scale=scale, msa_offset=offset)
    with pytest.raises(ValueError):
        _device.check_correction(scale, offset)


# ---------------------------------------------------------------------------------------------- the built library
def _hashes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    h = kernel_resources.kernel_code_hashes()
    assert len(h) > 100, "code objects of libldpc_hip.so not found"
    return h


def test_every_min_sum_kernel_has_its_corrected_sibling():
    """k_fused_bp<0, ..>, k_fused_f64<0, ..>, k_cn<T, 0, ..>, k_cn16<0, ..> -> the same name with algorithm 3 and otherwise equal template
    arguments.  (k_fused_bp_grid has no algorithm argument and no sibling: corrected decoders refuse the exact-in-fp32 mode.)"""
    names = set(_hashes())
    plain, want = [], []
    for nm in names:
        m = re.match(r"(k_fused_bp|k_fused_f64|k_cn16)<0, (.*)>$", nm)
        if m:
            plain.append(nm), want.append("%s<3, %s>" % m.groups())
        m = re.match(r"k_cn<(float|double), 0, (.*)>$", nm)
        if m:
            plain.append(nm), want.append("k_cn<%s, 3, %s>" % m.groups())
    assert len(plain) >= 60, plain
    assert {"k_fused_f64<0, 6, 3, 3, 5, 4, true, 0, 3>", "k_fused_bp<0, 6, 3, 5, 10, 2, true, 0, 3>", "k_cn<float, 0, 6, 6, 2, false>",
            "k_cn16<0, 6, 6, 2, false>"} <= set(plain)
    missing = sorted(w for w in want if w not in names)
    assert not missing, "min-sum kernels without a corrected sibling: %s" % missing
    # and nothing corrected that has no plain sibling (a shape that exists only with the correction on)
    for nm in names:
        m = re.match(r"(k_fused_bp|k_fused_f64|k_cn16)<3, (.*)>$", nm)
        if m:
            assert "%s<0, %s>" % m.groups() in names, nm
    assert not [nm for nm in names if re.match(r"k_vn<(float|double), 3,|k_vn16<3,", nm)], \
        "the variable pass does not depend on the rule: no corrected k_vn instantiations"


def test_priced_kernels_are_still_the_ones_their_counters_were_collected_on():
    """profiles/roofline_counters.json prices a bench line only while the timed kernel's kernel_code_sha matches.  Every entry that
    carries one matched the library before the corrected kernels were added (checked on a build of that commit: no exception to name),
    so every one must still match."""
    with open(os.path.join(ROOT, "profiles", "roofline_counters.json")) as fp:
        counters = json.load(fp)
    hashes = _hashes()
    checked = 0
    for key, entry in counters.items():
        if not isinstance(entry, dict) or "kernel_code_sha" not in entry:
            continue
        name = entry.get("kernel") or key.split(":")[-1]
        assert name in hashes, "kernel %s (entry %s) is not in the built library" % (name, key)
        assert hashes[name] == entry["kernel_code_sha"], "%s: machine code or descriptor changed (%s != %s)" % (key, hashes[name], entry["kernel_code_sha"])
        checked += 1
    assert checked >= 90

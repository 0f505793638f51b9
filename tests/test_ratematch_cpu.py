"""Transmission patterns on the host (ldpc_decoders_amd/ratematch.py): the spec grammar, the refusals, block columns, the stopping-set
report, the shortened code and its encoder, the command-line flags, the run ids with and without a pattern, and the ABI declarations.
No GPU: every refusal of ``main.test`` asserted here is raised before a decoder exists."""
import itertools
import os
import re

import numpy as np
import pytest

import bp_oracle as O
import ratematch_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rm():
    from ldpc_decoders_amd import ratematch

    return ratematch


# ---------------------------------------------------------------------------------------------- the spec grammar
@pytest.mark.parametrize("spec,n", [("0:54,600,1100:1200", 1200), ("5", 6), ("0:6", 6), ("0,2,4", 5), ("3:5,0:2,2", 7)])
def test_parse_round_trips(spec, n):
    rm = _rm()
    idx = rm.parse(spec, n)
    assert idx.dtype == np.int64 and idx.tolist() == RO.parse(spec, n)
    canon = rm.spec_of(idx)
    assert rm.parse(canon, n).tolist() == idx.tolist() and rm.spec_of(rm.parse(canon, n)) == canon
    assert not re.search(r"[^0-9:,]", canon)


def test_canonical_spec_merges_runs():
    rm = _rm()
    assert rm.spec_of(rm.parse("3:5,0:2,2", 7)) == "0:5" and rm.spec_of([7, 1, 2, 9]) == "1:3,7,9" and rm.spec_of([]) == ""


@pytest.mark.parametrize("spec", ["", "a", "1:", ":3", "3:3", "5:2", "0:7", "6", "-1", "1,,2", "1:2:3", "1.5"])
def test_bad_specs_are_refused(spec):
    with pytest.raises(ValueError):
        _rm().parse(spec, 6)


def test_pattern_rules_and_refusals():
    rm = _rm()
    p = rm.Pattern(10, punctured=[3, 4, 3], shortened=(9,))
    assert p.kind.dtype == np.uint8 and np.array_equal(p.kind, RO.kind_of(10, [3, 4], [9]))
    assert (p.n_tx, p.n_counted, p.empty) == (7, 9, False)
    assert (p.puncture_spec, p.shorten_spec) == ("3:5", "9")
    e = rm.Pattern(4)
    assert e.empty and e.n_tx == 4 and e.n_counted == 4 and not e.kind.any()
    for bad in (dict(punctured=[1, 2], shortened=[2]), dict(punctured=[10]), dict(shortened=[-1]), dict(punctured=[[1, 2]]), dict(punctured=[0.5])):
        with pytest.raises(ValueError):
            rm.Pattern(10, **bad)
        if "punctured" in bad and np.asarray(bad["punctured"]).ndim == 1 and np.asarray(bad["punctured"]).dtype.kind == "i":
            with pytest.raises(ValueError):
                RO.kind_of(10, **bad)
    with pytest.raises(ValueError):
        rm.Pattern(0)


def test_block_columns():
    rm = _rm()
    assert rm.block_columns([2, 0], 3).tolist() == [0, 1, 2, 6, 7, 8]
    assert rm.block_columns([], 27).size == 0 and rm.block_columns([5], 1).tolist() == [5]
    with pytest.raises(ValueError):
        rm.block_columns([-1], 3)
    with pytest.raises(ValueError):
        rm.block_columns([1], 0)


# ---------------------------------------------------------------------------------------------- stopping sets
def _edges(code):
    return O.Edges(code.m, code.n, code.edge_chk, code.edge_var)


def test_unrecoverable():
    from ldpc_decoders_amd import codes

    rm = _rm()
    code = codes.Code.from_rows(5, [(0, 1, 2), (2, 3, 4), (0, 1, 3)])
    # the empty set
    assert rm.Pattern(5).unrecoverable(code).size == 0
    # variable 2 has check 1 to itself among the punctured {0, 2}: it is recovered, and then check 0 recovers variable 0
    p = rm.Pattern(5, punctured=[0, 2])
    assert p.unrecoverable(code).size == 0 and RO.peel(_edges(code), p.kind) == []
    # {0, 1}: both lie on checks 0 and 2 and on no other -- every check of theirs sees two erasures: a stopping set
    p = rm.Pattern(5, punctured=[0, 1])
    lost = p.unrecoverable(code)
    assert lost.dtype == np.int64 and lost.tolist() == [0, 1] == RO.peel(_edges(code), p.kind)
    # the neighbourhood of check 0 in a code where its variables share all their other checks: reported whole
    code2 = codes.Code.from_rows(6, [(0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 4), (3, 4, 5)])
    p = rm.Pattern(6, punctured=[0, 1, 2, 5], shortened=[4])
    assert p.unrecoverable(code2).tolist() == [0, 1, 2] == RO.peel(_edges(code2), p.kind)
    # shortened bits are known, not erased
    assert rm.Pattern(6, shortened=[0, 1, 2]).unrecoverable(code2).size == 0
    with pytest.raises(ValueError):
        rm.Pattern(5).unrecoverable(code2)
    # random patterns on a random code against the check-by-check statement
    rng = np.random.RandomState(3)
    code3 = codes.rand_reg_ldpc(60, 3, 6, rng)
    for k in (5, 20, 40):
        p = rm.Pattern(60, punctured=rng.choice(60, k, replace=False))
        assert p.unrecoverable(code3).tolist() == RO.peel(_edges(code3), p.kind)


# ---------------------------------------------------------------------------------------------- the shortened code
def test_shortened_code_and_its_encoder():
    from ldpc_decoders_amd import codes

    rm = _rm()
    code = codes.rand_reg_ldpc(24, 3, 6, np.random.RandomState(5))
    short_set = [1, 5, 7, 23]
    p = rm.Pattern(24, punctured=[0, 2], shortened=short_set)
    short, index = p.shortened_code(code)
    assert (short.m, short.n) == (code.m, 20) and index.dtype == np.int64
    assert index.tolist() == [v for v in range(24) if v not in short_set]
    assert p.shortened_code(code)[0] is short  # kept on the pattern
    H = code.parity_mtx
    assert np.array_equal(short.parity_mtx, H[:, index])
    enc = short.encoder()
    assert enc.k >= 20 - code.m and enc.k <= 14
    u = np.array(list(itertools.product((0, 1), repeat=enc.k)), dtype=np.uint8)
    words = np.zeros((u.shape[0], 24), dtype=np.uint8)
    words[:, index] = enc.encode(u)
    assert not code.syndrome(words).any() and not words[:, short_set].any() and len(np.unique(words, axis=0)) == 2 ** enc.k
    # a check that keeps one variable or none is allowed: only the encoder sees this code
    tiny = codes.Code.from_rows(4, [(0, 1), (2, 3), (1, 2)])
    s2, i2 = rm.Pattern(4, shortened=[0, 1, 2]).shortened_code(tiny)
    assert (s2.m, s2.n, s2.E) == (3, 1, 1) and i2.tolist() == [3] and s2.encoder().k == 0
    # nothing shortened: the code itself, column for column
    s3, i3 = rm.Pattern(24, punctured=[3]).shortened_code(code)
    assert np.array_equal(s3.edge_var, code.edge_var) and np.array_equal(s3.edge_chk, code.edge_chk) and i3.tolist() == list(range(24))


# ---------------------------------------------------------------------------------------------- the command line
def _args(line):
    from ldpc_decoders_amd import main

    return main.build_parser().parse_args(line.split())


def test_parser_flags():
    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA")
    assert (a.puncture, a.shorten, a.puncture_cols, a.shorten_cols, a.short_llr) == (None, None, None, None, 32.0)
    a = _args("bsc 1200_3_6_rand_ldpc_1 LQMSA --puncture 0:54,600 --shorten 1100:1200 --puncture-cols 2,3 --shorten-cols 0 --short-llr 16")
    assert (a.puncture, a.shorten, a.puncture_cols, a.shorten_cols, a.short_llr) == ("0:54,600", "1100:1200", "2,3", "0", 16.0)


def test_no_pattern_flags_no_change_in_the_run_ids(tmp_path):
    """Without pattern flags the id keys and the result file are the parent's: literal strings."""
    from ldpc_decoders_amd import codes, main, models, ratematch, utils

    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA --params 2.0")
    assert ratematch.from_args(a, codes.get_code(a.code)) is None
    keys, vals = main.run_ids(a, models.models["biawgn"].MSA.id_keys)
    assert keys == ["channel", "code", "decoder", "codeword", "min_wec", "max_iter"]
    assert os.path.basename(utils.Saver(str(tmp_path), list(zip(keys, vals))).file_path) == "biawgn-1200_3_6_rand_ldpc_1-MSA-0-100-10.json"
    a = _args("bsc 1200_3_6_rand_ldpc_1 NMSA --codeword -1 --max-iter 20")
    keys, vals = main.run_ids(a, models.models["bsc"].NMSA.id_keys)
    assert keys == ["channel", "code", "decoder", "codeword", "min_wec", "max_iter", "msa_scale", "msa_offset"]
    assert os.path.basename(utils.Saver(str(tmp_path), list(zip(keys, vals))).file_path) == "bsc-1200_3_6_rand_ldpc_1-NMSA--1-100-20-0.8125-0.0.json"
    a = _args("biawgn 1200_3_6_rand_ldpc_1 LQMSA")
    keys, vals = main.run_ids(a, models.models["biawgn"].LQMSA.id_keys)
    assert os.path.basename(utils.Saver(str(tmp_path), list(zip(keys, vals))).file_path) == "biawgn-1200_3_6_rand_ldpc_1-LQMSA-0-100-10-6-2-0.8125-0.0.json"


def test_pattern_flags_enter_the_run_ids(tmp_path):
    from ldpc_decoders_amd import codes, main, models, ratematch, utils

    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture 10:20,3,4 --shorten 1199")
    p = ratematch.from_args(a, codes.get_code(a.code))
    assert (p.puncture_spec, p.shorten_spec, p.n_tx, p.n_counted) == ("3:5,10:20", "1199", 1187, 1199)
    keys, vals = main.run_ids(a, models.models["biawgn"].MSA.id_keys, p)
    assert keys[-2:] == ["puncture", "shorten"] and vals[-2:] == ["3:5,10:20", "1199"]
    assert os.path.basename(utils.Saver(str(tmp_path), list(zip(keys, vals))).file_path) == "biawgn-1200_3_6_rand_ldpc_1-MSA-0-100-10-3:5,10:20-1199.json"
    assert (a.puncture, a.shorten) == ("10:20,3,4", "1199")  # the namespace stays as parsed: a second run of it parses again
    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture 7")
    assert main.run_ids(a, [], ratematch.from_args(a, codes.get_code(a.code)))[1][-2:] == ["7", "none"] and a.shorten is None


def test_block_column_flags_take_the_lifting_size(tmp_path, monkeypatch):
    from ldpc_decoders_amd import codes, qc, ratematch

    code = qc.rand_qc_ldpc(qc.regular_mask(4, 8, 3), 27, np.random.RandomState(14))
    a = _args("biawgn 4_2_test MSA --puncture-cols 6:8 --shorten-cols 0 --puncture 30 --qc-lift 27")
    p = ratematch.from_args(a, code)
    assert (p.puncture_spec, p.shorten_spec) == ("30,162:216", "0:27")
    a.qc_lift = 0  # detected
    assert ratematch.from_args(a, code).puncture_spec == "30,162:216"
    a = _args("biawgn 4_2_test MSA --puncture-cols 8")
    with pytest.raises(ValueError):
        ratematch.from_args(a, code)
    with pytest.raises(ValueError):  # not quasi-cyclic
        ratematch.from_args(a, codes.get_code("1200_3_6_rand_ldpc_1"))


def test_registry_column():
    from ldpc_decoders_amd.registry import BY_NAME

    assert sorted(r.name for r in BY_NAME.values() if r.pattern) == sorted(["SPA", "MSA", "NMSA", "QMSA", "LMSA", "SLQMSA", "OSD", "QCMSA", "LQMSA"])


@pytest.mark.parametrize("line,word", [
    ("biawgn 1200_3_6_rand_ldpc_1 GALB --puncture 0:4", "GALB"),
    ("biawgn 1200_3_6_rand_ldpc_1 ADMM --shorten 0:4", "ADMM"),
    ("biawgn 7_4_hamming ML --puncture 0", "ML"),
    ("bec 1200_3_6_rand_ldpc_1 MSA --puncture 0:4", "bec"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture 0:4 --exact", "--exact"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture 0:4 --prior-grid 4", "--prior-grid"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture 0:1300", "0:1300"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture 0:4 --shorten 3", "both"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --shorten 3 --codeword 1", "all-one"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --shorten 3 --short-llr 0", "--short-llr"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture-cols 0", "quasi-cyclic"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture 0:1200", "stopping set"),
])
def test_main_refuses_before_a_decoder_exists(line, word, tmp_path):
    from ldpc_decoders_amd import main

    with pytest.raises(SystemExit) as e:
        main.test(_args(line + " --data_dir " + str(tmp_path)))
    assert word in str(e.value), str(e.value)


def test_stopping_set_refusal_names_the_first_variable(tmp_path):
    from ldpc_decoders_amd import codes, main

    code = codes.get_code("1200_3_6_rand_ldpc_1")
    rows = code.edge_var[code.edge_chk == 0].tolist()  # every variable of check 0 and of every check they are on: closed under peeling
    grow = set(rows)
    for _ in range(2):
        grow |= set(code.edge_var[np.isin(code.edge_chk, code.edge_chk[np.isin(code.edge_var, list(grow))])].tolist())
    lost = _rm().Pattern(1200, punctured=sorted(grow)).unrecoverable(code)
    assert lost.size
    with pytest.raises(SystemExit) as e:
        main.test(_args("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture %s --data_dir %s" % (_rm().spec_of(sorted(grow)), tmp_path)))
    assert "variable %d " % lost[0] in str(e.value)


# ---------------------------------------------------------------------------------------------- the ABI
def test_abi_declarations():
    from ldpc_decoders_amd import _lib

    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as fp:
        text = fp.read()
    for name, nargs in (("ldpc_channel_pattern", 15), ("ldpc_count_errors_pattern", 10)):
        m = re.search(r"\nint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "Makefile")) as fp:
        assert "ldpc_ratematch.hip" in fp.read()

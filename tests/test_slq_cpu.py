"""Streaming layered fixed-point min-sum (SLQMSA) without a GPU: the registry row, the command line, the refusals of the driver, the ABI
shapes, the Python checks -- and that a code beyond LQMSA's LDS rule passes them."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def padded_code(n=82944):
    """1200_3_6_rand_ldpc_1 with degree-0 variables appended up to n: more than 2^16 variables and 2 n above one CU's LDS"""
    from ldpc_decoders_amd import codes

    c = codes.get_code("1200_3_6_rand_ldpc_1")
    return codes.Code.from_edges(c.m, n, c.edge_chk, c.edge_var)


def test_registry_row_parser_and_channel_classes(tmp_path):
    from ldpc_decoders_amd import bec, biawgn, bsc, layered, main, models, registry, utils

    names = [r.name for r in registry.ROWS]
    row = registry.BY_NAME["SLQMSA"]
    assert names.index("SLQMSA") == names.index("LMSA") + 1 and names[-4:] == ["OSD", "QCMSA", "LQMSA", "GALB"]
    assert row.group == "streaming_fixed_point" and row.integer_streamed and row.backing is layered.SLQMSA
    assert models.streaming_fixed_point_decoder_names == ["SLQMSA"] and utils.streaming_fixed_point_decoder_names is models.streaming_fixed_point_decoder_names
    assert row.bec_refusal is None and row.prior_grid is None
    assert not (row.device_words or row.tie_dominated or row.f16 or row.osd_front or row.pops_layers or row.refuses_fused or row.hard or row.integer_layered
                or row.quasi_cyclic)
    assert [r.name for r in registry.ROWS if r.integer_streamed] == ["SLQMSA"]
    assert registry.Row._fields[-1] == "quasi_cyclic" and registry.Row._fields[-2] == "integer_streamed"
    assert len(registry.Row.__new__.__defaults__) == len(registry.Row._fields) - 3  # name, group and backing have no default
    assert "SLQMSA" in models.all_decoder_names and "SLQMSA" not in registry.osd_fronts()
    args = main.build_parser().parse_args("biawgn 1200_3_6_rand_ldpc_1 SLQMSA --msa-bits 5 --msa-frac-bits 1 --msa-scale 0.75 --msa-offset 1 --max-iter 20".split())
    assert (args.decoder, args.msa_bits, args.msa_frac_bits, args.msa_scale, args.msa_offset) == ("SLQMSA", 5, 1, 0.75, 1.0)
    assert bsc.SLQMSA.id_keys == biawgn.SLQMSA.id_keys == bec.SLQMSA.id_keys == layered.SLQMSA.id_keys == layered.LQMSA.id_keys
    assert bsc.SLQMSA.__module__.endswith(".bsc") and biawgn.SLQMSA.__module__.endswith(".biawgn") and bec.SLQMSA.__module__.endswith(".bec")
    assert issubclass(biawgn.SLQMSA, biawgn.LLR) and issubclass(bsc.SLQMSA, bsc.LLR)
    with pytest.raises(NotImplementedError) as e:
        bec.SLQMSA(0.1, None, max_iter=1)
    assert "does not exist over the bec" in str(e.value) and "SPA / MSA" in str(e.value)
    # the result file is named like LQMSA's
    id_keys = ["channel", "code", "decoder", "codeword", "min_wec"] + biawgn.SLQMSA.id_keys
    saver = utils.Saver(str(tmp_path), [(k, vars(args)[k]) for k in id_keys])
    assert os.path.basename(saver.file_path) == "biawgn-1200_3_6_rand_ldpc_1-SLQMSA-0-100-20-5-1-0.75-1.0.json"
    assert main.build_parser().format_help().count("SLQMSA") >= 4


@pytest.mark.parametrize("argline,needle", [
    ("biawgn 512_3_6_rand_ldpc_1 SLQMSA --precision f16", "--precision f16"),
    ("biawgn 512_3_6_rand_ldpc_1 SLQMSA --prior-grid 4", "--prior-grid"),
    ("bsc 512_3_6_rand_ldpc_1 SLQMSA --backend fused", "--backend fused"),
])
def test_the_driver_refuses_before_a_decoder_exists(argline, needle, tmp_path, monkeypatch):
    from ldpc_decoders_amd import layered, main

    def no_decoder(*a, **k):
        raise AssertionError("a decoder was built")

    monkeypatch.setattr(layered.SLQMSA, "__init__", no_decoder)
    args = main.build_parser().parse_args(argline.split() + ["--data_dir", str(tmp_path), "--console"])
    with pytest.raises(SystemExit) as e:
        main.test(args)
    assert needle in str(e.value) and "SLQMSA" in str(e.value)


@pytest.mark.parametrize("backend", ["auto", "stream"])
def test_the_driver_accepts_auto_and_stream_and_drops_layers(backend, tmp_path, monkeypatch):
    """--backend auto / stream reach the constructor; --layers (ADMMA's network shape) does not; words are drawn on the device (no --exact)."""
    from ldpc_decoders_amd import layered, main

    seen = {}

    def stop(self, parity_mtx, **k):
        seen.update(k)
        raise KeyboardInterrupt

    monkeypatch.setattr(layered.SLQMSA, "__init__", stop)
    argv = ("biawgn 512_3_6_rand_ldpc_1 SLQMSA --params 2.5 --codeword -1 --backend %s" % backend).split()
    args = main.build_parser().parse_args(argv + ["--data_dir", str(tmp_path), "--console"])
    with pytest.raises(KeyboardInterrupt):
        main.test(args)
    assert "layers" not in seen and seen["backend"] == backend and seen["msa_bits"] == 6 and seen["precision"] == "f32"  # (f64 under --exact)


def test_the_abi_declares_the_family_with_lqmsa_shapes():
    from ldpc_decoders_amd import _lib

    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as fp:
        text = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    declared = set(re.findall(r"\b(ldpc_slq_[a-z0-9_]+)\s*\(", text))
    assert declared == {"ldpc_slq_" + s for s in ("create", "destroy", "set_fixed_point", "get_fixed_point", "set_layers", "get_layers", "decode", "simulate",
                                                  "info", "profile", "last_stats")}
    assert declared <= set(_lib.SIGNATURES)
    for fn in ("create", "destroy", "set_fixed_point", "get_fixed_point", "set_layers", "get_layers", "decode", "simulate", "info"):
        assert _lib.SIGNATURES["ldpc_slq_" + fn] == _lib.SIGNATURES["ldpc_lqmsa_" + fn], fn
    assert "SLQMSA" not in _lib.ALG  # a handle family of its own, not an algorithm of ldpc_decoder_create
    # the argument lists in the header are LQMSA's, name for name
    raw = re.sub(r"\s+", " ", text)
    for fn in ("decode", "simulate"):
        a = re.search(r"int ldpc_lqmsa_%s\((.*?)\);" % fn, raw).group(1).replace("ldpc_lqmsa_t", "H")
        b = re.search(r"int ldpc_slq_%s\((.*?)\);" % fn, raw).group(1).replace("ldpc_slq_t", "H")
        assert a == b, fn


def test_parameters_and_degrees_are_checked_in_python(monkeypatch):
    from ldpc_decoders_amd import _lib, codes, layered

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    code = codes.get_code("512_3_6_rand_ldpc_1")
    for kw in (dict(msa_bits=9), dict(msa_bits=1), dict(msa_frac_bits=9), dict(msa_scale=0.8), dict(msa_scale=0.0), dict(msa_offset=-1), dict(msa_offset=0.5),
               dict(precision="f16"), dict(backend="fused"), dict(layers=np.zeros(code.m, dtype=np.int64)), dict(layers=np.arange(code.m - 1))):
        with pytest.raises(ValueError):
            layered.SLQMSA(code, max_iter=5, **kw)
    with pytest.raises(ValueError):  # a check of degree 1
        layered.SLQMSA(np.array([[1, 1, 0], [0, 0, 1]]), max_iter=5)
    # a variable of degree 256: 256 checks {0, 1 + c}
    chk = np.repeat(np.arange(256), 2).astype(np.int32)
    var = np.stack([np.zeros(256, dtype=np.int32), 1 + np.arange(256, dtype=np.int32)], axis=1).reshape(-1)
    with pytest.raises(ValueError, match="degree 256"):
        layered.SLQMSA(codes.Code.from_edges(256, 257, chk, var), max_iter=5)
    with pytest.raises(AssertionError):  # degree 255 passes every Python check and reaches the library
        layered.SLQMSA(codes.Code.from_edges(255, 256, chk[:510], var[:510]), max_iter=5)
    # streaming and auto backends, f32 and f64 priors pass the checks too
    for kw in (dict(backend="stream"), dict(backend="auto", precision="f64")):
        with pytest.raises(AssertionError):
            layered.SLQMSA(code, max_iter=5, **kw)


def test_a_code_beyond_the_lds_rule_passes(monkeypatch):
    """n = 82 944 > 2^16 and 2 n bytes of marginals above one CU's LDS: LQMSA's Python check refuses the code, SLQMSA's takes it."""
    from ldpc_decoders_amd import _lib, layered

    c = padded_code()
    assert c.n == 82944 and c.m == 600 and c.E == 3600 and c.col_degrees()[1200:].max() == 0
    assert layered.lqmsa_lds_bytes(c.m, c.n, c.E, 6) > layered.LDS_BYTES
    with pytest.raises(ValueError, match="LMSA"):
        layered.check_code(c)
    layered.check_code_streamed(c)

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError):
        layered.LQMSA(c, max_iter=5)
    with pytest.raises(AssertionError, match="the library was loaded"):
        layered.SLQMSA(c, max_iter=5)
    # (3, 6) at n = 64 800, the code of BASELINE config 5, by its degrees alone
    big = type("C", (), dict(m=32400, n=64800, E=194400, edge_chk=np.repeat(np.arange(32400), 6), edge_var=np.arange(194400) % 64800))()
    layered.check_code_streamed(big)

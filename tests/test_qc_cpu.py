"""Quasi-cyclic codes without a GPU: construction and detection of the structure (ldpc_decoders_amd/qc.py), the generator's girth condition,
block rows as layers, the LDS and wave rules, the ABI block, the registry row, the command line and the Python-side refusals."""
import os
import re

import numpy as np
import pytest

import bp_oracle as O
import lmsa_oracle as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = np.array([[0, 3, -1, 1], [2, -1, 4, 0]])  # Z = 5


def _dense(base, Z):
    H = np.zeros((base.shape[0] * Z, base.shape[1] * Z), dtype=np.int64)
    for i in range(base.shape[0]):
        for j in range(base.shape[1]):
            for r in range(Z):
                if base[i, j] >= 0:
                    H[i * Z + r, j * Z + (r + base[i, j]) % Z] = 1
    return H


def test_expand_equals_the_dense_construction():
    from ldpc_decoders_amd import qc

    c = qc.expand(BASE, 5)
    assert (c.m, c.n, c.E) == (10, 20, 30) and np.array_equal(c.parity_mtx, _dense(BASE, 5))
    assert np.array_equal(c.qc[0], BASE) and c.qc[1] == 5
    assert np.array_equal(qc.expand(np.array([[0, 0], [0, -1]]), 1).parity_mtx, np.array([[1, 1], [1, 0]]))
    for bad, Z in ((np.array([[0, 5]]), 5), (np.array([[0, -2]]), 5), (np.array([[0.5, 1.0]]), 5), (np.array([0, 1]), 5), (BASE, 0)):
        with pytest.raises(ValueError):
            qc.expand(bad, Z)


def test_find_structure_round_trips(tmp_path):
    from ldpc_decoders_amd import codes, qc

    for base, Z in ((BASE, 5), (np.array([[6, 0, 3], [1, 2, -1]]), 7)):
        c = qc.expand(base, Z)
        got, z = qc.find_structure(c, Z)
        assert z == Z and np.array_equal(got, base)
        got, z = qc.find_structure(codes.Code.from_edges(c.m, c.n, c.edge_chk, c.edge_var))  # detected: no qc attribute to lean on
        assert z == Z and np.array_equal(got, base)
        back = codes.load_parity_mtx(codes.save_parity_mtx(c, "qc_round_trip_%d" % Z, str(tmp_path)))
        assert getattr(back, "qc", None) is None
        got, z = qc.find_structure(back)
        assert z == Z and np.array_equal(got, base)
    # every divisor of Z for which the blocks stay shifted identities is a structure too; detection returns the largest
    c = qc.expand(np.array([[0, 2], [4, 0]]), 6)
    assert qc.find_structure(c)[1] == 6
    sub, z = qc.find_structure(c, 1)
    assert z == 1 and np.array_equal(sub >= 0, c.parity_mtx > 0)


def test_detection_refusals():
    from ldpc_decoders_amd import codes, qc

    c = qc.expand(BASE, 5)
    var = c.edge_var.copy()
    k = int(np.flatnonzero((c.edge_chk == 5 + 2) & (c.edge_var // 5 == 2))[0])
    var[k] = 10 + (var[k] + 1) % 5  # one edge moved inside block (1, 2)
    moved = codes.Code.from_edges(c.m, c.n, c.edge_chk, var)
    with pytest.raises(ValueError, match=r"block \(1, 2\)"):
        qc.find_structure(moved, 5)
    with pytest.raises(ValueError, match="no quasi-cyclic structure"):
        qc.find_structure(moved)
    two = _dense(BASE, 5)
    two[0:5, 10:15] = np.eye(5) + np.roll(np.eye(5), 1, axis=1)  # a block with two ones per row: a circulant of weight 2
    with pytest.raises(ValueError, match=r"block \(0, 2\)"):
        qc.find_structure(codes.Code(None, two), 5)
    for Z in (3, 4, 0, -5, 2.5):
        with pytest.raises(ValueError, match="dividing"):
            qc.find_structure(c, Z)
    shipped = codes.get_code("1200_3_6_rand_ldpc_1")
    with pytest.raises(ValueError, match="no quasi-cyclic structure"):
        qc.find_structure(shipped)
    with pytest.raises(ValueError, match=r"block \(\d+, \d+\)"):
        qc.find_structure(shipped, 200)


def test_the_generator_keeps_girth_6_and_gives_up_where_it_cannot():
    from ldpc_decoders_amd import qc

    dense = np.ones((3, 6), dtype=bool)
    for Z in (7, 27, 64, 200):
        c = qc.rand_qc_ldpc(dense, Z, np.random.RandomState(Z))
        base = c.qc[0]
        assert not qc.has_4_cycle(base, Z) and ((base >= 0) == dense).all() and (c.m, c.n) == (3 * Z, 6 * Z)
        # the condition itself, on the expanded H: no two checks share two variables
        H = c.parity_mtx
        common = H @ H.T
        np.fill_diagonal(common, 0)
        assert common.max() <= 1
    with pytest.raises(ValueError, match="4-cycle"):  # six distinct differences mod 5 do not exist
        qc.rand_qc_ldpc(dense, 5, np.random.RandomState(1))
    loose = qc.rand_qc_ldpc(dense, 2, np.random.RandomState(1), girth6=False)
    assert loose.qc[1] == 2 and qc.has_4_cycle(loose.qc[0], 2)
    a = qc.rand_qc_ldpc(qc.regular_mask(6, 12, 3), 100, np.random.RandomState(4))
    b = qc.rand_qc_ldpc(qc.regular_mask(6, 12, 3), 100, np.random.RandomState(4))
    assert np.array_equal(a.qc[0], b.qc[0]) and (a.col_degrees() == 3).all() and (a.row_degrees() == 6).all()
    mask = qc.regular_mask(4, 8, 3)
    assert mask.sum(axis=0).tolist() == [3] * 8 and mask.sum(axis=1).tolist() == [6] * 4 and mask[:, 1].tolist() == [False, True, True, True]


def test_the_generator_command_line(tmp_path):
    from ldpc_decoders_amd import codes, qc

    paths = qc.gen_rand_qc(qc.setup_parser().parse_args(["2", "4", "8", "27", "--seed", "5", "--dir", str(tmp_path)]))
    assert [os.path.basename(p) for p in paths] == ["216_qc_4x8_z27_1.txt", "216_qc_4x8_z27_2.txt"]
    a, b = (codes.load_parity_mtx(p) for p in paths)
    assert (a.m, a.n) == (108, 216) and qc.find_structure(a)[1] == 27 and not np.array_equal(a.edge_var, b.edge_var)
    with open(paths[0]) as fp:
        first = fp.readline().split()
    assert len(first) == 6 and min(int(t) for line in open(paths[0]) for t in line.split()) == 1  # 1-based, one check per line


def test_block_rows_in_any_order_are_a_valid_layering():
    from ldpc_decoders_amd import qc

    c = qc.rand_qc_ldpc(qc.regular_mask(4, 8, 3), 9, np.random.RandomState(2))
    g = O.Edges(c.m, c.n, c.edge_chk, c.edge_var)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        lay = qc.layers_of(9, np.array(order))
        assert np.array_equal(L.check_layers(g, lay), lay) and lay[9 * order[0]] == 0 and lay[9 * order[3] + 8] == 3
    with pytest.raises(ValueError):  # two block rows in one layer share variables
        L.check_layers(g, np.arange(c.m) // 18)
    for bad in ([0, 1, 2], [0, 1, 2, 2], [0, 1, 2, 4], [[0, 1, 2, 3]], [0.0, 1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            qc.check_order(4, np.array(bad))
    assert qc.check_order(4, [2, 0, 3, 1]).dtype == np.int32


def test_the_lds_rule_and_the_wave_rule():
    from ldpc_decoders_amd import layered, qc

    # LQMSA's layout with the largest block-row degree: dense 3 x 6 at Z = 200 is the n = 1200 frame of 7216 bytes
    assert layered.lqmsa_lds_bytes(600, 1200, 3600, 6) == 7216
    # waves: lqmsa_waves(F) capped at the smallest of 1, 2, 4, 8 >= ceil(Z / 64)
    assert [qc.qc_waves(1, z) for z in (1, 64, 65, 128, 129, 256, 257, 512, 513, 5000)] == [1, 1, 2, 2, 4, 4, 8, 8, 8, 8]
    assert [qc.qc_waves(f, 4550) for f in (1, 7, 8, 15, 16, 31, 32, 400)] == [8, 8, 4, 4, 2, 2, 1, 1]
    assert qc.qc_waves(22, 200) == 2 and qc.qc_waves(22, 63) == 1 and qc.qc_waves(4, 129) == 4 and qc.qc_waves(4, 100) == 2
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "ldpc_qc.hpp")) as fp:
        text = fp.read()
    assert "while (cap < 8 && cap < passes) cap *= 2;" in text and "lqmsa_waves(frames_per_cu)" in text and '#include "ldpc_lqmsa.hpp"' in text
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "ldpc_qc.hip")) as fp:
        text = fp.read()
    assert "lqmsa_lds_bytes(code->m, code->n, code->E, h->dc_max)" in text and "need > LQMSA_LDS_BYTES" in text and "asm" not in text
    # check_code: the rule on either side of 160 KiB, a block row of degree 1
    z_ok = (layered.LDS_BYTES - 16) // 36
    dense = np.zeros((3, 6), dtype=np.int64)
    qc.check_code(qc.expand(dense, z_ok), dense, z_ok)
    with pytest.raises(ValueError, match="LMSA"):
        qc.check_code(qc.expand(dense, z_ok + 1), dense, z_ok + 1)
    one = np.array([[0, 1, -1], [-1, -1, 2]])
    with pytest.raises(ValueError, match="at least two"):
        qc.check_code(qc.expand(one, 5), one, 5)


def test_the_abi_declares_and_binds_the_family():
    from ldpc_decoders_amd import _lib

    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as fp:
        text = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    declared = set(re.findall(r"\b(ldpc_qc_[a-z0-9_]+)\s*\(", text))
    assert declared == {"ldpc_qc_create", "ldpc_qc_destroy", "ldpc_qc_set_fixed_point", "ldpc_qc_get_fixed_point", "ldpc_qc_get_base", "ldpc_qc_set_order",
                        "ldpc_qc_get_order", "ldpc_qc_decode", "ldpc_qc_simulate", "ldpc_qc_info"}
    assert declared <= set(_lib.SIGNATURES)
    for name in ("decode", "simulate", "info", "set_fixed_point", "get_fixed_point", "destroy"):  # the call shapes of the LQMSA family
        assert _lib.SIGNATURES["ldpc_qc_" + name] == _lib.SIGNATURES["ldpc_lqmsa_" + name]
    assert len(_lib.SIGNATURES["ldpc_qc_create"][1]) == 3 and "QCMSA" not in _lib.ALG


def test_registry_row_parser_and_channel_classes(tmp_path):
    from ldpc_decoders_amd import bec, biawgn, bsc, layered, main, models, qc, registry, utils

    names = [r.name for r in registry.ROWS]
    row = registry.BY_NAME["QCMSA"]
    assert names.index("OSD") + 1 == names.index("QCMSA") == names.index("LQMSA") - 1 and names[-2:] == ["LQMSA", "GALB"]
    assert row.group == "quasi_cyclic" and row.quasi_cyclic and row.backing is qc.QCMSA and row.bec_refusal is None and row.prior_grid is None
    assert not (row.device_words or row.tie_dominated or row.f16 or row.osd_front or row.pops_layers or row.refuses_fused or row.hard or row.integer_layered)
    assert [r.name for r in registry.ROWS if r.quasi_cyclic] == ["QCMSA"] and registry.Row._fields[-1] == "quasi_cyclic"
    assert models.quasi_cyclic_decoder_names == ["QCMSA"] and utils.quasi_cyclic_decoder_names is models.quasi_cyclic_decoder_names
    assert "QCMSA" in models.all_decoder_names and "QCMSA" not in registry.osd_fronts()
    args = main.build_parser().parse_args("biawgn 512_3_6_rand_ldpc_1 QCMSA --qc-lift 27 --msa-bits 5 --msa-frac-bits 1 --msa-scale 0.75 --msa-offset 1 --max-iter 20".split())
    assert (args.decoder, args.qc_lift, args.msa_bits, args.msa_frac_bits, args.msa_scale, args.msa_offset) == ("QCMSA", 27, 5, 1, 0.75, 1.0)
    assert main.build_parser().parse_args("bsc 512_3_6_rand_ldpc_1 QCMSA".split()).qc_lift == 0
    keys = layered.LQMSA.id_keys + ["qc_lift"]
    assert bsc.QCMSA.id_keys == biawgn.QCMSA.id_keys == bec.QCMSA.id_keys == qc.QCMSA.id_keys == keys
    assert issubclass(biawgn.QCMSA, biawgn.LLR) and issubclass(bsc.QCMSA, bsc.LLR) and bec.QCMSA.__module__.endswith(".bec")
    with pytest.raises(NotImplementedError) as e:
        bec.QCMSA(0.1, None, max_iter=1)
    assert "does not exist over the bec" in str(e.value) and "SPA / MSA" in str(e.value)
    id_keys = ["channel", "code", "decoder", "codeword", "min_wec"] + biawgn.QCMSA.id_keys
    saver = utils.Saver(str(tmp_path), [(k, vars(args)[k]) for k in id_keys])
    assert os.path.basename(saver.file_path) == "biawgn-512_3_6_rand_ldpc_1-QCMSA-0-100-20-5-1-0.75-1.0-27.json"
    assert main.build_parser().format_help().count("QCMSA") >= 3


@pytest.mark.parametrize("argline,needle", [
    ("biawgn 512_3_6_rand_ldpc_1 QCMSA --precision f16", "--precision f16"),
    ("biawgn 512_3_6_rand_ldpc_1 QCMSA --prior-grid 4", "--prior-grid"),
    ("bsc 512_3_6_rand_ldpc_1 QCMSA --backend stream", "--backend stream"),
    ("bsc 512_3_6_rand_ldpc_1 QCMSA", "no quasi-cyclic structure"),
    ("bsc 512_3_6_rand_ldpc_1 QCMSA --qc-lift 64", "block (0, 0)"),
])
def test_the_driver_refuses_before_a_decoder_exists(argline, needle, tmp_path, monkeypatch):
    from ldpc_decoders_amd import main, qc

    def no_decoder(*a, **k):
        raise AssertionError("a decoder was built")

    monkeypatch.setattr(qc.QCMSA, "__init__", no_decoder)
    args = main.build_parser().parse_args(argline.split() + ["--data_dir", str(tmp_path), "--console"])
    with pytest.raises(SystemExit) as e:
        main.test(args)
    assert needle in str(e.value) and "QCMSA" in str(e.value)


def test_the_driver_resolves_the_lift_draws_words_on_the_device_and_drops_layers(tmp_path, monkeypatch):
    from ldpc_decoders_amd import codes, main, qc

    monkeypatch.setenv(codes.file_codes_dir_string, str(tmp_path))
    qc.gen_rand_qc(qc.setup_parser().parse_args(["1", "4", "8", "27", "--seed", "5", "--dir", str(tmp_path)]))
    seen = {}

    def stop(self, parity_mtx, **k):
        seen.update(k)
        raise KeyboardInterrupt

    monkeypatch.setattr(qc.QCMSA, "__init__", stop)
    args = main.build_parser().parse_args("biawgn 216_qc_4x8_z27_1 QCMSA --params 2.5 --codeword -1 --backend fused".split() + ["--data_dir", str(tmp_path), "--console"])
    with pytest.raises(KeyboardInterrupt):
        main.test(args)
    # (precision f32: --codeword -1 did not select the reference's sequential fp64 loop, so the words are drawn on the device)
    assert "layers" not in seen and seen["qc_lift"] == 27 and seen["backend"] == "fused" and seen["msa_bits"] == 6 and seen["precision"] == "f32"


def test_everything_is_checked_in_python_before_the_library_loads(monkeypatch):
    from ldpc_decoders_amd import _lib, codes, qc

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    code = qc.rand_qc_ldpc(np.ones((3, 6), dtype=bool), 7, np.random.RandomState(1))
    for kw in (dict(msa_bits=9), dict(msa_scale=0.8), dict(msa_offset=-1), dict(precision="f16"), dict(backend="stream"), dict(qc_lift=5), dict(qc_lift=3),
               dict(qc_order=[0, 1]), dict(qc_order=[0, 1, 1]), dict(qc_order=[1, 2, 3])):
        with pytest.raises(ValueError):
            qc.QCMSA(code, max_iter=5, **kw)
    with pytest.raises(ValueError, match="no quasi-cyclic structure"):
        qc.QCMSA(codes.get_code("1200_3_6_rand_ldpc_1"), max_iter=5)
    with pytest.raises(ValueError, match="at least two"):
        qc.QCMSA(qc.expand(np.array([[0, 1, -1], [-1, -1, 2]]), 5), max_iter=5)
    with pytest.raises(ValueError, match="LMSA"):
        qc.QCMSA(qc.expand(np.zeros((3, 6), dtype=np.int64), 4551), max_iter=5)
    for kw in (dict(), dict(qc_lift=7), dict(qc_lift=1), dict(qc_order=[2, 0, 1])):  # the accepted side passes every Python check and reaches the library
        with pytest.raises(AssertionError, match="the library was loaded"):
            qc.QCMSA(code, max_iter=5, **kw)

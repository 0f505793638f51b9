"""Gallager-B without a GPU: properties of the numpy statement (galb_oracle.py), the registry row, the command line and the ABI."""
import os
import time

import numpy as np
import pytest

import galb_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["12_3_4_ldpc", "7_4_hamming", "512_3_6_rand_ldpc_1"]


def _code(name):
    from ldpc_decoders_amd import codes

    return codes.get_code(name)


def _words(code, B, rng):
    enc = code.encoder()
    return enc.encode(rng.integers(0, 2, size=(B, enc.k)))


def _syndrome(code, x):
    return (x.astype(np.int64) @ code.parity_mtx.T.astype(np.int64)) & 1


@pytest.mark.parametrize("name", SMALL)
def test_a_codeword_leaves_at_iteration_zero(name):
    code = _code(name)
    w = _words(code, 9, np.random.default_rng(1))
    assert not _syndrome(code, w).any()
    for t in (0, 1, 255):
        x, it = G.galb_decode(code, w, t=t, max_iter=5)
        assert (x == w).all() and (it == 0).all()


@pytest.mark.parametrize("name", SMALL)
def test_the_vectorised_statement_equals_the_plain_one(name):
    code = _code(name)
    rng = np.random.default_rng(2)
    B = 24 if code.n < 100 else 6
    y = _words(code, B, rng) ^ (rng.random((B, code.n)) < 0.06).astype(np.uint8)
    for t in (0, 1, 2, 255):
        for flags in (0, G.NO_EARLY_EXIT):
            x, it = G.galb_decode(code, y, t=t, max_iter=6, flags=flags)
            for f in range(B):
                xp, ip = G.galb_decode_plain(code, y[f], t=t, max_iter=6, flags=flags)
                assert (x[f] == xp).all() and it[f] == ip, (name, t, flags, f)


@pytest.mark.parametrize("name", SMALL)
def test_threshold_255_is_threshold_0_up_to_degree_3(name):
    code = _code(name)
    assert code.col_degrees().max() <= 3
    rng = np.random.default_rng(3)
    y = _words(code, 64, rng) ^ (rng.random((64, code.n)) < 0.05).astype(np.uint8)
    a, b = G.galb_decode(code, y, t=0, max_iter=10), G.galb_decode(code, y, t=255, max_iter=10)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


@pytest.mark.parametrize("name", ["12_3_4_ldpc", "512_3_6_rand_ldpc_1"])
def test_a_single_flipped_bit_is_corrected_in_one_sweep(name):
    code = _code(name)
    assert set(code.col_degrees()) == {3}
    w = _words(code, code.n, np.random.default_rng(4))
    y = w ^ np.eye(code.n, dtype=np.uint8)
    for t in (0, 1, 255):
        x, it = G.galb_decode(code, y, t=t, max_iter=4)
        assert (x == w).all() and (it == 1).all()


@pytest.mark.parametrize("name", SMALL)
def test_iteration_counts_and_exits(name):
    code = _code(name)
    rng = np.random.default_rng(5)
    B, max_iter = 200, 7
    y = _words(code, B, rng) ^ (rng.random((B, code.n)) < 0.07).astype(np.uint8)
    y[:3] = _words(code, 3, rng)
    x, it = G.galb_decode(code, y, max_iter=max_iter)
    xn, itn = G.galb_decode(code, y, max_iter=max_iter, flags=G.NO_EARLY_EXIT)
    assert (itn == max_iter).all() and (it[:3] == 0).all() and it.max() <= max_iter
    ok = ~_syndrome(code, x).any(axis=1)
    assert ((it < max_iter) <= ok).all()  # a frame leaves early only with a codeword
    # a frame without a codeword ran every sweep; one with a codeword left before the cap or at the last sweep
    assert (it[~ok] == max_iter).all()
    # early exit only latches what the free-running decoder passes through: the word of sweep `it` (checked by cutting the run there)
    for f in np.flatnonzero((it > 0) & (it < max_iter))[:5]:
        xc, _ = G.galb_decode(code, y[f:f + 1], max_iter=int(it[f]), flags=G.NO_EARLY_EXIT)
        assert (xc[0] == x[f]).all()
    with pytest.raises(ValueError):
        G.galb_decode(code, y, max_iter=0)
    with pytest.raises(ValueError):
        G.galb_decode(code, y, t=256)


def test_flip_thresholds_on_the_irregular_degrees():
    from ldpc_decoders_amd import hard

    code = _code("1200_rho_x5_rand_ldpc_10")
    assert sorted(int(d) for d in set(code.col_degrees())) == [0, 2, 3, 4, 6, 7, 8]  # (degree 1 occurs in 7_4_hamming; the formula covers it)
    d = np.array([0, 1, 2, 3, 4, 6, 7, 8])
    assert G.flip_threshold(d, 0).tolist() == [1, 1, 1, 2, 2, 3, 4, 4]      # floor((d - 1) / 2) + 1
    assert G.flip_threshold(d, 1).tolist() == [1] * 8
    assert G.flip_threshold(d, 3).tolist() == [1, 1, 1, 2, 3, 3, 3, 3]      # min(t, max(d - 1, 1))
    assert G.flip_threshold(d, 255).tolist() == [1, 1, 1, 2, 3, 5, 6, 7]    # Gallager A: all d - 1 others
    for t in (0, 1, 3, 255):
        assert hard.flip_threshold(d, t).tolist() == G.flip_threshold(d, t).tolist()
    # variables without an edge keep the received bit; the batch runs through
    rng = np.random.default_rng(6)
    y = (rng.random((40, code.n)) < 0.004).astype(np.uint8)
    x, it = G.galb_decode(code, y, max_iter=10)
    iso = code.col_degrees() == 0
    assert iso.any() and (x[:, iso] == y[:, iso]).all()


def test_the_oracle_is_fast():
    code = _code("1200_3_6_rand_ldpc_1")
    rng = np.random.default_rng(7)
    y = (rng.random((300, code.n)) < 0.03).astype(np.uint8)
    t0 = time.perf_counter()
    x, it = G.galb_decode(code, y, max_iter=20)
    assert time.perf_counter() - t0 < 4.0  # a plain np.add.at version needs about 8 s here
    assert (it == 0).sum() == 0 and ((it > 0) & (it < 20)).sum() > 200


def test_registry_row_parser_and_channel_classes(tmp_path):
    from ldpc_decoders_amd import bec, biawgn, bsc, hard, main, models, registry, utils

    assert models.hard_decision_decoder_names == ["GALB"] and utils.hard_decision_decoder_names is models.hard_decision_decoder_names
    row = registry.BY_NAME["GALB"]
    assert registry.ROWS[-1] is row and row.group == "hard_decision" and row.hard and row.bec_refusal is None and row.prior_grid is None
    assert not (row.device_words or row.tie_dominated or row.f16 or row.osd_front or row.pops_layers or row.refuses_fused)
    assert [r.name for r in registry.ROWS if r.hard] == ["GALB"]
    args = main.build_parser().parse_args("bsc 512_3_6_rand_ldpc_1 GALB --gal-threshold 2 --max-iter 20 --backend stream".split())
    assert args.decoder == "GALB" and args.gal_threshold == 2 and args.max_iter == 20 and args.backend == "stream"
    assert main.build_parser().parse_args("biawgn 12_3_4_ldpc GALB".split()).gal_threshold == 0
    assert bsc.GALB.id_keys == biawgn.GALB.id_keys == bec.GALB.id_keys == hard.GALB.id_keys == ["max_iter", "gal_threshold"]
    assert bsc.GALB.__module__.endswith(".bsc") and biawgn.GALB.__module__.endswith(".biawgn") and bec.GALB.__module__.endswith(".bec")
    with pytest.raises(NotImplementedError) as e:
        bec.GALB(0.1, None, max_iter=1)
    assert "no erasures to work on" in str(e.value) and "SPA / MSA" in str(e.value) and "ML" in str(e.value)
    # the result file: <channel>-<code>-<decoder>-<codeword>-<min_wec>-<max_iter>-<gal_threshold>.json
    id_keys = ["channel", "code", "decoder", "codeword", "min_wec"] + bsc.GALB.id_keys
    saver = utils.Saver(str(tmp_path), [(k, vars(args)[k]) for k in id_keys])
    assert os.path.basename(saver.file_path) == "bsc-512_3_6_rand_ldpc_1-GALB-0-100-20-2.json"


@pytest.mark.parametrize("argline,needle", [
    ("bsc 512_3_6_rand_ldpc_1 GALB --precision f16", "--precision f16"),
    ("biawgn 512_3_6_rand_ldpc_1 GALB --prior-grid 4", "--prior-grid"),
    ("bsc 512_3_6_rand_ldpc_1 GALB --max-iter 0", "--max-iter"),
    ("bsc 512_3_6_rand_ldpc_1 GALB --max-iter -1", "--max-iter"),
])
def test_the_driver_refuses_before_a_decoder_exists(argline, needle, tmp_path, monkeypatch):
    from ldpc_decoders_amd import hard, main

    def no_decoder(*a, **k):
        raise AssertionError("a decoder was built")

    monkeypatch.setattr(hard.GALB, "__init__", no_decoder)
    args = main.build_parser().parse_args(argline.split() + ["--data_dir", str(tmp_path), "--console"])
    with pytest.raises(SystemExit) as e:
        main.test(args)
    assert needle in str(e.value)


def test_parameters_are_checked_in_python():
    from ldpc_decoders_amd import hard

    assert hard.check_params(20, 0) == (20, 0) and hard.check_params(1, 255) == (1, 255) and hard.check_params(3, None) == (3, 0)
    for bad in ((0, 0), (-1, 0), (5, 256), (5, -1), (5, 1.5)):
        with pytest.raises(ValueError):
            hard.check_params(*bad)


def test_every_shipped_code_fits_the_lds_kernel():
    from ldpc_decoders_amd import codes, hard

    names = [n for n in codes.get_code_names() if os.path.exists(os.path.join(ROOT, "ldpc_decoders_amd", "data", "codes", n + ".txt"))]
    assert len(names) == 27 and "margulis" in names
    for name in names:
        c = codes.get_code(name)
        assert hard.hard_lds_bytes(c.m, c.n, c.E) <= hard.LDS_BYTES, name
        assert c.col_degrees().max() <= 63


def test_the_abi_declares_and_binds_the_family():
    import re

    from ldpc_decoders_amd import _lib

    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as fp:
        text = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    declared = set(re.findall(r"\b(ldpc_hard_[a-z0-9_]+)\s*\(", text))
    assert declared == {"ldpc_hard_create", "ldpc_hard_destroy", "ldpc_hard_set_threshold", "ldpc_hard_get_threshold", "ldpc_hard_decode",
                        "ldpc_hard_simulate", "ldpc_hard_last_backend", "ldpc_hard_info"}
    assert declared <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["ldpc_hard_decode"][1]) == 9 and len(_lib.SIGNATURES["ldpc_hard_simulate"][1]) == 13
    assert "GALB" not in _lib.ALG  # a handle family of its own, not an algorithm of ldpc_decoder_create

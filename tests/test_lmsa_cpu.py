"""Layered min-sum (LDPC_ALG_LMSA, bpa.LMSA) without a GPU: the layering, the restatement (tests/lmsa_oracle.py) on a hand-worked
example and against the flooding restatement where the two schedules coincide, what the schedule is worth, and the registry, command
line and C ABI declarations."""
import os
import re

import numpy as np
import pytest

import bp_oracle as O
import lmsa_oracle as L
import nmsa_oracle as N
from helpers import CODES_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def edges_of(name):
    from ldpc_decoders_amd import codes

    path = os.path.join(CODES_DIR, name + ".txt")
    c = codes.load_parity_mtx(path) if os.path.exists(path) else codes.get_code(name)
    return O.Edges(c.m, c.n, c.edge_chk, c.edge_var)


def frames_2db(g, B=48, seed=1, snr=2.0):
    """the frames of the issue's table: all-zero word over BI-AWGN, np.random.RandomState(seed)"""
    rng = np.random.RandomState(seed)
    return O.biawgn_priors(-1 + rng.normal(0, np.sqrt(O.biawgn_noise_var(snr)), (B, g.n)), snr)


@pytest.mark.parametrize("name,nlayers", [("1200_3_6_rand_ldpc_1", 3), ("1200_3_6_rand_ldpc_7", 3), ("512_3_6_rand_ldpc_1", 4), ("margulis", 8),
                                          ("1200_rho_x5_rand_ldpc_5", 12), ("12_3_4_ldpc", 3)])
def test_greedy_layering_of_the_shipped_codes(name, nlayers):
    g = edges_of(name)
    lay = L.greedy_layers(g)
    assert (L.check_layers(g, lay) == lay).all()  # valid: no two checks of a layer on one variable
    assert lay.max() + 1 == nlayers and set(lay.tolist()) == set(range(nlayers))
    if name.startswith("1200_3_6"):
        assert np.bincount(lay).tolist() == [200, 200, 200]
    # minimal in the greedy sense: every check clashes with an earlier check in each layer below its own
    chk, var = np.asarray(g.chk), np.asarray(g.var)
    for c in range(0, g.m, 37):
        mine = set(var[chk == c].tolist())
        for l in range(lay[c]):
            assert any(mine & set(var[chk == o].tolist()) for o in np.flatnonzero(lay[:c] == l))


def test_check_layers_refuses_what_the_contract_refuses():
    g = edges_of("12_3_4_ldpc")
    lay = L.greedy_layers(g)
    for bad in (lay[:-1], -lay - 1, np.zeros(g.m, dtype=np.int64), lay.astype(np.float64)):
        with pytest.raises(ValueError):
            L.check_layers(g, bad)
    assert (L.check_layers(g, np.arange(g.m)[::-1]) == np.arange(g.m)[::-1]).all()  # one check per layer, any numbering


def test_hand_worked_two_check_example():
    """H = [[1 1 1 0], [0 0 1 1]]: the checks share variable 2, so they are layers 0 and 1.  Priors (4, -1, 2, -3), scale 0.5, offset 0.25.
    Check 0 sees v = (4, -1, 2):   c2v = (-max(.5*1-.25, 0), +max(.5*2-.25, 0), -max(.5*1-.25, 0)) = (-.25, .75, -.25); marg = (3.75, -.25, 1.75, -3).
    Check 1 sees v = (1.75, -3):   c2v = (-max(.5*3-.25, 0), +max(.5*1.75-.25, 0)) = (-1.25, .625);                     marg = (3.75, -.25, .5, -2.375).
    x_hat = (0, 1, 0, 1): check 0 fails (parity 1), so a second sweep runs:
    Check 0: v = (3.75 + .25, -.25 - .75, .5 + .25) = (4, -1, .75): c2v = (-.125, .125, -.25); marg = (3.875, -.875, .5, -2.375)
    Check 1: v = (.5 + 1.25, -2.375 - .625) = (1.75, -3): c2v as before; marg = (3.875, -.875, .5, -2.375)."""
    g = O.Edges(2, 4, np.array([0, 0, 0, 1, 1]), np.array([0, 1, 2, 2, 3]))
    assert L.greedy_layers(g).tolist() == [0, 1]
    pri = np.array([[4.0, -1.0, 2.0, -3.0]])
    for dt in (np.float64, np.float32):
        x, it, soft = L.lmsa_decode(g, None, pri, 1, 0.5, 0.25, dtype=dt)
        assert soft.dtype == dt and soft.tolist() == [[3.75, -0.25, 0.5, -2.375]] and x.tolist() == [[0, 1, 0, 1]] and it.tolist() == [1]
        x, it, soft = L.lmsa_decode(g, None, pri, 2, 0.5, 0.25, dtype=dt)
        assert soft.tolist() == [[3.875, -0.875, 0.5, -2.375]] and it.tolist() == [2]
        # the other order of the two layers gives another result: check 1 first sees v = (2, -3)
        _, _, other = L.lmsa_decode(g, None, pri, 1, 0.5, 0.25, layers=[1, 0], dtype=dt)
        assert other.tolist() != [[3.75, -0.25, 0.5, -2.375]]
    # the iteration-0 rule: a received codeword leaves with iters = 0, its word, soft output 0
    x, it, soft = L.lmsa_decode(g, np.array([[1, 1, 0, 0]], dtype=np.uint8), pri, 5, 0.5, 0.25)
    assert it.tolist() == [0] and x.tolist() == [[1, 1, 0, 0]] and not soft.any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_layer_is_the_flooding_schedule(dtype):
    """Pairwise disjoint checks (one layer, every variable of degree 1): marg - c2v_old is the prior again in every sweep up to rounding
    -- here exactly, on priors that are multiples of 1/8 with scale 1/2 -- and the layered restatement equals the flooding one, frame
    for frame."""
    m, dc = 5, 4
    g = O.Edges(m, m * dc, np.repeat(np.arange(m), dc), np.arange(m * dc))
    assert not L.greedy_layers(g).any()
    rng = np.random.RandomState(3)
    pri = rng.randint(-40, 41, size=(64, g.n)) / 8.0
    for scale, offset in ((1.0, 0.0), (0.5, 0.0), (0.5, 0.25)):
        a = L.lmsa_decode(g, None, pri, 6, scale, offset, dtype=dtype)
        b = N.nmsa_decode(g, None, pri, 6, scale, offset, dtype)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and np.array_equal(a[2], b[2])
        assert 0 < (a[1] < 6).sum() < 64


def test_processing_a_layer_at_once_is_processing_its_checks_one_by_one():
    g = edges_of("512_3_6_rand_ldpc_1")
    pri = frames_2db(g, B=6, seed=5)
    for dt in (np.float64, np.float32):
        a = L.lmsa_decode(g, None, pri, 8, 0.8125, 0.0, dtype=dt)
        b = L.lmsa_decode(g, None, pri, 8, 0.8125, 0.0, dtype=dt, one_by_one=True)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and np.array_equal(a[2], b[2])


def test_the_layered_schedule_needs_fewer_sweeps():
    """1200_3_6_rand_ldpc_1, 2.0 dB, 48 frames of np.random.RandomState(1), scale 0.8125, cap 50: layered total <= 0.75 x flooding total
    (measured: 334 against 584 sweeps, 0.57)."""
    g = edges_of("1200_3_6_rand_ldpc_1")
    pri = frames_2db(g)
    _, it_l, _ = L.lmsa_decode(g, None, pri, 50, 0.8125, 0.0)
    _, it_f, _ = N.nmsa_decode(g, None, pri, 50, 0.8125, 0.0)
    print("layered %d sweeps, flooding %d: %.3f" % (it_l.sum(), it_f.sum(), it_l.sum() / it_f.sum()))
    assert it_l.sum() <= 0.75 * it_f.sum()


def test_registry_parser_and_result_file(tmp_path):
    from ldpc_decoders_amd import _lib, bec, biawgn, bpa, bsc, main, models, utils

    assert models.layered_decoder_names == ["LMSA"] == utils.layered_decoder_names
    assert models.extra_decoder_names == ["NMSA"] and models.fixed_point_decoder_names == ["QMSA"] and models.post_processing_decoder_names == ["OSD"]
    assert _lib.ALG["LMSA"] == 5
    for mod in (biawgn, bsc, bec):
        assert mod.LMSA.id_keys == bpa.LMSA.id_keys == ["max_iter", "msa_scale", "msa_offset"]
    with pytest.raises(NotImplementedError):
        bec.LMSA(0.4, None, max_iter=10)
    p = main.build_parser()
    a = p.parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "LMSA", "--params", "2.5", "--max-iter", "20", "--min-wec", "3", "--max-frames", "4096",
                      "--batch", "1024"])
    assert (a.decoder, a.msa_scale, a.msa_offset) == ("LMSA", 0.8125, 0.0)
    id_keys = ["channel", "code", "decoder", "codeword", "min_wec"] + biawgn.LMSA.id_keys
    saver = utils.Saver(str(tmp_path), [(k, vars(a)[k]) for k in id_keys])
    assert os.path.basename(saver.file_path) == "biawgn-1200_3_6_rand_ldpc_1-LMSA-0-3-20-0.8125-0.0.json"


@pytest.mark.parametrize("extra,match", [(["--prior-grid", "4"], "--prior-grid"), (["--precision", "f16"], "--precision f16"), (["--backend", "fused"], "--backend fused")])
def test_refused_on_the_command_line_before_a_decoder_exists(tmp_path, extra, match, monkeypatch):
    from ldpc_decoders_amd import _lib, main

    def no_gpu(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_gpu)
    a = main.build_parser().parse_args(["biawgn", "1200_3_6_rand_ldpc_1", "LMSA", "--data_dir", str(tmp_path)] + extra)
    with pytest.raises(SystemExit, match=match):
        main.test(a)


def test_bad_layering_and_degree_one_checks_raise_before_any_gpu_call(monkeypatch):
    from ldpc_decoders_amd import _lib, bpa, codes

    def no_gpu(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_gpu)
    code = codes.get_code("12_3_4_ldpc")
    for bad in (np.zeros(code.m, dtype=np.int64), np.arange(code.m - 1), -np.arange(code.m)):
        with pytest.raises(ValueError):
            bpa.LMSA(code, max_iter=10, layers=bad)
    with pytest.raises(ValueError, match="at least two"):
        bpa.LMSA(np.array([[1, 1, 0], [0, 0, 1]]), max_iter=10)
    for kw in (dict(msa_scale=0.0), dict(msa_offset=-1.0), dict(precision="f16"), dict(backend="fused")):
        with pytest.raises(ValueError):
            bpa.LMSA(code, max_iter=10, **kw)


def test_header_and_signatures_declare_the_two_new_entry_points():
    from ldpc_decoders_amd import _lib

    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as fp:
        header = fp.read()
    assert re.search(r"enum \{ LDPC_ALG_LMSA = 5 \};", header)
    assert re.search(r"int ldpc_decoder_set_layers\(ldpc_decoder_t \w+, const int32_t\* \w+, int32_t m\);", header)
    assert re.search(r"int ldpc_decoder_get_layers\(ldpc_decoder_t \w+, int32_t\* nlayers, int32_t\* \w+\);", header)
    declared = set(re.findall(r"\b(ldpc_[a-z0-9_]+)\s*\(", header))
    assert {"ldpc_decoder_set_layers", "ldpc_decoder_get_layers"} <= declared & set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["ldpc_decoder_set_layers"][1]) == 3 and len(_lib.SIGNATURES["ldpc_decoder_get_layers"][1]) == 3
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "ldpc_api.hip")) as fp:
        api = fp.read()
    for name in ("ldpc_decoder_set_layers", "ldpc_decoder_get_layers"):
        assert re.search(r"int %s\([^)]*\) \{\s*return guarded\(\"%s\"" % (name, name), api)
    assert "int ldpc_abi_version(void) { return 4; }" in api

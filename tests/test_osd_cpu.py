"""Ordered-statistics post-processing (bpa.OSD, csrc/ldpc_osd.hip): the numpy statement of the contract (osd_oracle.py) checked against
the code books of the toy codes, the size rule, the parser and the registry.  No GPU needed; test_gpu_osd.py holds the device to the
statement bit for bit."""
import numpy as np
import pytest

import osd_oracle as OSD


def random_frame(rng, n, sent):
    """(post, prior) float64 for one frame: noisy LLRs of ``sent``, then -- frame by frame -- ties, zeros, infinities, a NaN."""
    sigma = rng.choice([0.6, 0.9, 1.3])
    prior = 2.0 * ((1 - 2.0 * sent) + sigma * rng.standard_normal(n)) / sigma ** 2
    post = prior + rng.choice([0.0, 1.0]) * 2.0 * rng.standard_normal(n)  # post and prior may disagree in sign
    kind = rng.randint(6)
    if kind == 1:  # massive ties: a BSC-like frame
        post = np.sign(post) * 1.5
        prior = np.sign(prior) * 1.5
    elif kind == 2:  # zero reliabilities
        post[rng.random_sample(n) < 0.4] = 0.0
        prior[rng.random_sample(n) < 0.2] = -0.0
    elif kind == 3:  # all zero: the order is the variable index
        post = np.zeros(n)
    elif kind == 4:
        post[rng.randint(n)] = np.inf
        prior[rng.randint(n)] = -np.inf
        post[rng.randint(n)] = np.nan
    return post, prior


def codebook_cost(cb, post, prior):
    """The contract's cost of every code-book word: the fp64 sum in the sorted order of ``post``, position by position."""
    pi = OSD.sort_order(post)
    g = OSD.hard(prior).astype(np.int64)
    w = np.abs(np.where(np.isnan(prior), 0, prior)).astype(np.float64)
    cost = np.zeros(len(cb), dtype=np.float64)
    for v in pi:
        d = cb[:, v] != g[v]
        cost[d] = cost[d] + w[v]
    return cost


@pytest.mark.parametrize("name", ["7_4_hamming", "12_3_4_ldpc", "6_2_3_ldpc", "4_2_test"])
def test_statement_against_the_code_book(name):
    """The output is always a code-book word, its cost is no less than the code book's minimum, order 1 never costs more than order 0,
    order 1 with every flip allowed reaches at least every word one information flip away, and pass-through frames are untouched."""
    from ldpc_decoders_amd import codes

    code = codes.get_code(name)
    H = code.parity_mtx.astype(np.uint8)
    cb = code.cb.astype(np.int64)
    words = {c.astype(np.uint8).tobytes() for c in cb}
    rng = np.random.RandomState(11)
    touched = 0
    for trial in range(300):
        post, prior = random_frame(rng, code.n, cb[rng.randint(len(cb))])
        x0, t0, c0 = OSD.osd_frame(H, post, prior, 0, 0)
        x1, t1, c1 = OSD.osd_frame(H, post, prior, 1, 3)
        xa, ta, ca = OSD.osd_frame(H, post, prior, 1, 10 ** 6)
        h = OSD.hard(post)
        if h.tobytes() in words:
            for x, t, c in ((x0, t0, c0), (x1, t1, c1), (xa, ta, ca)):
                assert (x == h).all() and t == -1 and c == -1.0
            continue
        touched += 1
        best = codebook_cost(cb, post, prior).min()
        for x, t, c in ((x0, t0, c0), (x1, t1, c1), (xa, ta, ca)):
            assert x.tobytes() in words, (name, trial)
            assert c >= best, (name, trial)
            assert c == codebook_cost(x[None, :].astype(np.int64), post, prior)[0]
        assert t0 == 0 and 0 <= t1 <= 3 and 0 <= ta <= code.encoder().k
        assert ca <= c1 <= c0
        # (1, depth 0) is order 0
        xz, tz, cz = OSD.osd_frame(H, post, prior, 1, 0)
        assert (xz == x0).all() and tz == 0 and cz == c0
        # float32 inputs with the same values give the same order and the same word
        p32, q32 = post.astype(np.float32), prior.astype(np.float32)
        if (p32.astype(np.float64) == post)[~np.isnan(post)].all():
            assert (OSD.osd_frame(H, p32, q32, 0, 0)[0] == x0).all()
    assert touched >= 100, touched


def test_sort_order_is_total_and_breaks_ties_by_index():
    post = np.array([0.5, -0.5, 0.0, np.nan, -0.0, 2.0, np.inf, 1e300, 0.5], dtype=np.float64)
    # zeros (and the NaN) first by index, then the 0.5s by index, then 2, then 1e300 -> inf in fp32 and inf, by index
    assert OSD.sort_order(post).tolist() == [2, 3, 4, 0, 1, 8, 5, 6, 7]
    # the key is the fp32 rounding: 1 + 2^-30 and 1 tie
    assert OSD.sort_order(np.array([1.0 + 2.0 ** -30, 1.0])).tolist() == [0, 1]


def test_rref_does_not_depend_on_the_pivot_choice():
    rng = np.random.RandomState(3)
    A = (rng.random_sample((9, 14)) < 0.4).astype(np.uint8)
    A[7] = A[1] ^ A[2]  # a dependent row
    A[:, 5] = 0          # an all-zero column
    R, rowof = OSD.rref(A)
    perm = rng.permutation(9)
    R2, rowof2 = OSD.rref(A[perm])
    assert ((rowof >= 0) == (rowof2 >= 0)).all() and rowof[5] == -1
    key = lambda M: sorted(r.tobytes() for r in M)  # noqa: E731
    assert key(R) == key(R2)
    piv = np.flatnonzero(rowof >= 0)
    assert (R[np.ix_(rowof[piv], piv)] == np.eye(len(piv), dtype=np.uint8)).all()


def test_margulis_raises_value_error_without_loading_the_library(monkeypatch):
    from ldpc_decoders_amd import _lib, biawgn, bpa, codes

    def boom():
        raise AssertionError("the library must not be loaded for a code above the limit")

    monkeypatch.setattr(_lib, "load", boom)
    code = codes.get_code("margulis")
    with pytest.raises(ValueError, match="160 KiB"):
        bpa.OSD(code, max_iter=10)
    with pytest.raises(ValueError, match="160 KiB"):
        biawgn.OSD(2.0, code, max_iter=10)


def test_size_rule_covers_the_reference_codes():
    from ldpc_decoders_amd import bpa, codes

    for name in codes.get_code_names():
        c = codes.get_code(name)
        fits = bpa.osd_lds_bytes(c.m, c.n) <= bpa.OSD_LDS_BYTES
        assert fits == (name != "margulis"), name
    assert bpa.osd_lds_bytes(600, 1200) == 4 * (2 * 2048 + 38 * 640 + 4 * 1200 + 5 * 38)
    assert bpa.osd_lds_bytes(256, 512) == 4 * (2 * 512 + 16 * 256 + 4 * 512 + 5 * 16)
    assert bpa.osd_lds_bytes(9, 12) == 4 * (2 * 16 + 1 * 64 + 4 * 12 + 5)


def test_bad_parameters_raise_before_the_library_is_loaded(monkeypatch):
    from ldpc_decoders_amd import _lib, bec, bpa, codes

    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("no library call expected")))
    code = codes.get_code("12_3_4_ldpc")
    for kw in (dict(osd_order=2), dict(osd_depth=-1), dict(osd_bp="BEC"), dict(precision="f16")):
        with pytest.raises(ValueError):
            bpa.OSD(code, max_iter=10, **kw)
    with pytest.raises(NotImplementedError, match="ML"):
        bec.OSD(0.3, code, max_iter=10)


def test_parser_accepts_osd_and_its_flags():
    from ldpc_decoders_amd import main

    p = main.build_parser()
    a = p.parse_args(["biawgn", "512_3_6_rand_ldpc_1", "OSD", "--params", "2", "--max-iter", "20"])
    assert a.decoder == "OSD" and a.osd_order == 0 and a.osd_depth == 64
    a = p.parse_args(["bsc", "1200_3_6_rand_ldpc_1", "OSD", "--osd-order", "1", "--osd-depth", "17", "--msa-scale", "1", "--msa-offset", "0"])
    assert (a.osd_order, a.osd_depth, a.msa_scale, a.msa_offset) == (1, 17, 1.0, 0.0)
    with pytest.raises(SystemExit):
        p.parse_args(["biawgn", "512_3_6_rand_ldpc_1", "OSD", "--osd-order", "2"])


def test_cli_refuses_f16_and_prior_grid_for_osd(tmp_path):
    from ldpc_decoders_amd import main

    p = main.build_parser()
    for extra in (["--precision", "f16"], ["--prior-grid", "4"]):
        args = p.parse_args(["biawgn", "12_3_4_ldpc", "OSD", "--params", "2", "--console", "--data_dir", str(tmp_path)] + extra)
        with pytest.raises(SystemExit):
            main.test(args)


def test_registry_has_the_new_list_and_keeps_the_old_ones():
    from ldpc_decoders_amd import biawgn, bsc, models, utils

    assert models.post_processing_decoder_names == ["OSD"] and utils.post_processing_decoder_names == ["OSD"]
    assert models.decoder_names == ["ML", "SPA", "MSA", "LP", "ADMM", "ADMMA"]
    assert models.extra_decoder_names == ["NMSA"] and models.fixed_point_decoder_names == ["QMSA"]
    keys = ["max_iter", "msa_scale", "msa_offset", "osd_order", "osd_depth"]
    assert biawgn.OSD.id_keys == keys and bsc.OSD.id_keys == keys and models.models["bec"].OSD.id_keys == keys

"""Several frames per wave for quasi-cyclic codes of lifting size up to 32, without a GPU: the rule ``qc.qc_pack`` and the stride it rests
on, their source lines in csrc/ldpc_qc.hpp, the two ``ldpc_qcpack_*`` entries (declared, bound, exported), the command line and the
Python-side refusals of ``qc.QCMSA(..., qc_pack=P)``."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 163840


def test_the_rule():
    from ldpc_decoders_amd import layered, qc

    small = layered.lqmsa_lds_bytes(3 * 7, 6 * 7, 18 * 7, 6)
    assert [qc.qc_pack(z, small) for z in (1, 2, 7, 21, 22, 32)] == [64, 32, 9, 3, 2, 2]
    assert qc.qc_pack(33, small) == 1 and qc.qc_pack(64, small) == 1 and qc.qc_pack(200, small) == 1
    # the LDS cap: regular_mask(250, 500, 3) at Z = 16 is n = 8000 with 48 016 bytes, three of which fit where the lanes take four
    assert layered.lqmsa_lds_bytes(4000, 8000, 24000, 6) == 48016 and qc.qc_pack(16, 48016) == 3
    assert qc.qc_pack(16, 81921) == 1 and qc.qc_pack(2, LDS) == 1 and qc.qc_pack(16, 40000) == 4


def test_the_stride():
    """At least the frame's bytes, a multiple of 16, and congruent to 2 Z rounded up to 16 modulo the 128 bytes of the 32 banks."""
    from ldpc_decoders_amd import qc

    for z in (1, 2, 7, 8, 9, 16, 21, 27, 31, 32):
        for need in (56, 64, 100, 3904, 3905, 48016, 81920):
            s = qc.qc_pack_stride(need, z)
            assert need <= s < need + 16 + 128 and s % 16 == 0 and s % 128 == (2 * z + 15) // 16 * 16 % 128, (z, need, s)
            assert qc.qc_pack_stride(s, z) == s
    assert qc.qc_pack_stride(48016, 16) == 48032 and qc.qc_pack_stride(3904, 27) == 3904


def test_the_source_states_the_rule_once():
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "ldpc_qc.hpp")) as fp:
        text = fp.read()
    assert "if (Z > 32) return 1;" in text
    assert "const int64_t lanes = 64 / Z, fit = LQMSA_LDS_BYTES / qc_pack_stride(lds_bytes_per_frame, Z);" in text
    assert "return s + (want - s % 128 + 128) % 128;" in text
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "ldpc_qc.hip")) as fp:
        kernel = fp.read()
    assert "k_qc_pack" in kernel and "qc_pack_stride(h->lds_bytes, h->Z)" in kernel and "LDPC_QC_PACK_GRID" in kernel


def test_the_abi_declares_binds_and_exports_the_two_entries():
    import ctypes

    from ldpc_decoders_amd import _lib

    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as fp:
        raw = fp.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ldpc_qcpack_[a-z0-9_]+)\s*\(", text))
    assert declared == {"ldpc_qcpack_set", "ldpc_qcpack_get"} and declared <= set(_lib.SIGNATURES)
    assert "int ldpc_qcpack_set(ldpc_qc_t h, int32_t frames_per_wave);" in text
    assert "int ldpc_qcpack_get(ldpc_qc_t h, int32_t* frames_per_wave, int32_t* rule_pick);" in text
    assert "With Z < 64 part of the\n * wave idles.  Handles" not in raw and "LDPC_QC_PACK_GRID" in raw and "stride(bytes, Z)" in raw
    assert _lib.SIGNATURES["ldpc_qcpack_set"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert len(_lib.SIGNATURES["ldpc_qcpack_get"][1]) == 3
    lib = ctypes.CDLL(_lib.library_path())  # the built library exports them
    assert lib.ldpc_qcpack_set and lib.ldpc_qcpack_get
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "ldpc_api.hip")) as fp:
        api = fp.read()
    # defined under their own names, inside the guard (handle_entry's whole body is `return guarded(entry, ...)`) and on a Qc handle
    assert "static int handle_entry(const char* entry, T h, bool ok, const char* what, F&& f) {\n    return guarded(entry, [&]() -> int {" in api
    for name in ("ldpc_qcpack_set", "ldpc_qcpack_get"):
        assert re.search(r'^int %s\(ldpc_qc_t h, [^{]*\{\s*return handle_entry<Qc>\("%s", h, ' % (name, name), api, re.M), name


def test_the_parser_takes_the_flag_and_the_id_keys_stay():
    from ldpc_decoders_amd import biawgn, bsc, layered, main, qc

    args = main.build_parser().parse_args("biawgn 512_3_6_rand_ldpc_1 QCMSA --qc-lift 27 --qc-pack 2".split())
    assert args.qc_pack == 2 and args.qc_lift == 27
    assert main.build_parser().parse_args("bsc 512_3_6_rand_ldpc_1 QCMSA".split()).qc_pack == 0
    keys = layered.LQMSA.id_keys + ["qc_lift"]
    assert qc.QCMSA.id_keys == biawgn.QCMSA.id_keys == bsc.QCMSA.id_keys == keys and "qc_pack" not in keys


def test_the_driver_hands_the_flag_to_the_class(tmp_path, monkeypatch):
    from ldpc_decoders_amd import codes, main, qc

    monkeypatch.setenv(codes.file_codes_dir_string, str(tmp_path))
    qc.gen_rand_qc(qc.setup_parser().parse_args(["1", "4", "8", "27", "--seed", "5", "--dir", str(tmp_path)]))
    seen = {}

    def stop(self, parity_mtx, **k):
        seen.update(k)
        raise KeyboardInterrupt

    monkeypatch.setattr(qc.QCMSA, "__init__", stop)
    for extra, want in (([], 0), (["--qc-pack", "1"], 1), (["--qc-pack", "2"], 2)):
        args = main.build_parser().parse_args("biawgn 216_qc_4x8_z27_1 QCMSA --params 2.5".split() + extra + ["--data_dir", str(tmp_path), "--console"])
        with pytest.raises(KeyboardInterrupt):
            main.test(args)
        assert seen["qc_pack"] == want and seen["qc_lift"] == 27
    # a number of frames the wave cannot take is refused before a decoder exists
    args = main.build_parser().parse_args("biawgn 216_qc_4x8_z27_1 QCMSA --qc-pack 3".split() + ["--data_dir", str(tmp_path), "--console"])
    with pytest.raises(SystemExit) as e:
        main.test(args)
    assert "--qc-pack" in str(e.value) and "Z = 27" in str(e.value)


def test_an_explicit_pack_is_checked_before_the_library_loads(monkeypatch):
    from ldpc_decoders_amd import _device, _lib, layered, qc

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    dense = np.ones((3, 6), dtype=bool)
    z7 = qc.rand_qc_ldpc(dense, 7, np.random.RandomState(1))
    z40 = qc.rand_qc_ldpc(dense, 40, np.random.RandomState(1))
    big = qc.rand_qc_ldpc(qc.regular_mask(250, 500, 3), 16, np.random.RandomState(1))  # 48 016 bytes a frame: three fit, four lanes' worth do not
    assert layered.lqmsa_lds_bytes(big.m, big.n, big.E, 6) == 48016
    for code, P, needle in ((z7, 10, "Z = 7"), (z7, 64, "Z = 7"), (z40, 2, "Z = 40"), (big, 4, "48032 bytes"), (z7, -1, "qc_pack"), (z7, 2.5, "qc_pack")):
        with pytest.raises(ValueError, match=needle):
            qc.QCMSA(code, max_iter=5, qc_pack=P)
    # the accepted side passes every Python check and reaches the library
    for code, P in ((z7, 0), (z7, 1), (z7, 2), (z7, 9), (z40, 0), (z40, 1), (big, 3), (big, 0)):
        with pytest.raises(AssertionError, match="the library was loaded"):
            qc.QCMSA(code, max_iter=5, qc_pack=P)
    # and the value arrives there: the class hands the handle what it was given, the handle passes it on
    seen = []

    class Lib:
        def ldpc_qcpack_set(self, h, P):
            seen.append((h, P))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    made = []
    monkeypatch.setattr(qc, "QcHandle", lambda *a: made.append(a) or "handle")
    for P in (0, 1, 9):
        assert qc.QCMSA(z7, max_iter=5, qc_pack=P).qc_pack == P and made[-1][-1] == P
    h = object.__new__(_device.QcHandle)
    h.h = "the handle"
    h.set_pack(3)
    assert seen == [("the handle", 3)]
    del h.h

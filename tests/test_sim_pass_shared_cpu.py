"""The layer every auxiliary handle family passes through is stated once: the Monte-Carlo pass loop with its two codeword refusals and the
odd-degree scan in csrc/ldpc_sim.hpp, and the refusal of a null handle -- which names its entry point -- in the helpers of csrc/ldpc_api.hip.
No GPU: a null handle is refused before any device work."""
import ctypes
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ldpc_decoders_amd", "csrc")
HEADER = "ldpc_sim.hpp"
E_ARG = -1  # include/ldpc_hip.h
CORE = {"ldpc_code", "ldpc_decoder", "ldpc_encoder"}  # the families of the main decoder, not stated through the helpers
ALIASES = {"ldpc_qcpack": "ldpc_qc"}                  # a second prefix on the handle of another family


def _families():
    from ldpc_decoders_amd import _lib

    return sorted({name[:-len("_create")] for name in _lib.SIGNATURES if name.endswith("_create")} - CORE)


def _entries():
    """every entry point of the auxiliary families: (name, argtypes)"""
    from ldpc_decoders_amd import _lib

    prefixes = tuple(f + "_" for f in _families() + sorted(ALIASES))
    return [(name, sig[1]) for name, sig in sorted(_lib.SIGNATURES.items()) if name.startswith(prefixes)]


def _zero(argtype):
    if argtype in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(argtype, "contents"):
        return None
    return argtype(0)


def _refused_by_name(lib, name, argtypes):
    # a different error first, so that a message left behind cannot pass
    info = (ctypes.c_double * 4)()
    assert lib.ldpc_plan_layout(-1, 4, 4, None, None, 0, 0, 1000, None, info) < 0 and b"bad graph arguments" in lib.ldpc_last_error()
    rc = getattr(lib, name)(*[_zero(t) for t in argtypes])
    msg = lib.ldpc_last_error().decode()
    assert rc == E_ARG and msg.startswith(name + ":"), (name, rc, msg)


def test_a_null_handle_is_refused_under_the_entry_points_own_name():
    from ldpc_decoders_amd import _lib

    lib = _lib.load()
    calls = [(n, a) for n, a in _entries() if not n.endswith(("_create", "_destroy"))]
    assert len(calls) >= 43 and {"ldpc_hard_info", "ldpc_slq_profile", "ldpc_admm_last_repacks", "ldpc_qcpack_get"} <= {n for n, _ in calls}
    for name, argtypes in calls:
        assert argtypes[0] is ctypes.c_void_p, name  # the handle
        _refused_by_name(lib, name, argtypes)


def test_create_refuses_a_null_code_under_its_own_name():
    from ldpc_decoders_amd import _lib

    lib = _lib.load()
    on_a_code = [(n, a) for n, a in _entries() if n.endswith("_create") and a[0] is ctypes.c_void_p]
    assert len(on_a_code) >= 7
    for name, argtypes in on_a_code:
        _refused_by_name(lib, name, argtypes)
        out = ctypes.c_void_p()
        assert getattr(lib, name)(*([_zero(t) for t in argtypes[:-1]] + [ctypes.byref(out)])) == E_ARG and not out.value
        assert lib.ldpc_last_error().decode().startswith(name + ":")


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            with open(os.path.join(CSRC, name)) as fp:
                out[name] = fp.read()
    return out


def test_the_pass_loop_is_stated_once():
    texts = _sources()
    odd_scan = re.compile(r"row_ptr\[\w+ \+ 1\] - \S*row_ptr\[\w+\]\) & 1")  # is the degree of a check odd
    for needle in ("all-ones word is no codeword", "codeword must be 0 or 1", odd_scan):
        count = (lambda t: len(needle.findall(t))) if hasattr(needle, "findall") else (lambda t: t.count(needle))
        where = {name: count(text) for name, text in texts.items() if count(text)}
        assert where == {HEADER: 1}, (needle, where)
    assert "LDPC_SIM_PASS_FRAMES" in texts[HEADER] and sum("getenv(\"LDPC_SIM_PASS_FRAMES\")" in t for t in texts.values()) == 1
    for user in ("ldpc_hard.hip", "ldpc_osd.hip", "ldpc_bec_ml.hip", "ldpc_layered_fx.hpp", "ldpc_api.hip"):
        assert '#include "%s"' % HEADER in texts[user], user
    with open(os.path.join(CSRC, "Makefile")) as fp:
        assert HEADER in fp.read().split("HDRS :=")[1].splitlines()[0]

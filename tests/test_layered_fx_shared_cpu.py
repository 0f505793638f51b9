"""The layered fixed-point min-sum is stated once, in csrc/ldpc_layered_fx.hpp, for LQMSA, QCMSA and SLQMSA: the rule's two telling lines, the
refusal texts the three families share and the names the copies once carried, counted over the four source files.  No GPU."""
import os

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ldpc_decoders_amd", "csrc")
HEADER = "ldpc_layered_fx.hpp"
FAMILIES = ("ldpc_lqmsa.hip", "ldpc_qc.hip", "ldpc_slq.hip")


def _texts():
    out = {}
    for name in FAMILIES + (HEADER,):
        with open(os.path.join(CSRC, name)) as fp:
            out[name] = fp.read()
    return out


def test_the_source_states_the_rule_once():
    texts = _texts()
    for needle in (">> 6) - offset",                                                            # the scaled, offset magnitude
                   "min2 = min1;",                                                              # the two running minima
                   "scale a multiple of 1/64 in (0, 1]",                                        # *_set_fixed_point
                   "min-sum has no magnitudes to work on over the erasure channel",             # *_simulate
                   "at most 2^31 frames per call"):                                             # *_decode
        counts = {name: text.count(needle) for name, text in texts.items()}
        assert counts == {"ldpc_lqmsa.hip": 0, "ldpc_qc.hip": 0, "ldpc_slq.hip": 0, HEADER: 1}, (needle, counts)


def test_no_copy_keeps_its_old_name():
    for name, text in _texts().items():
        for gone in ("lq_mag", "qc_mag", "slq_mag", "qc_pack_write"):
            assert gone not in text, (name, gone)


def test_the_three_families_use_the_header_and_the_library_builds_with_it():
    texts = _texts()
    for name in FAMILIES:
        assert '#include "%s"' % HEADER in texts[name], name
    with open(os.path.join(CSRC, "Makefile")) as fp:
        assert HEADER in fp.read().split("HDRS :=")[1].splitlines()[0]

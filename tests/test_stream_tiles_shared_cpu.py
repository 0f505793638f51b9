"""The tile machinery of the streaming decoders -- tile helpers, bookkeeping kernels, repack policy, the poll / repack protocol of the sweep
loop -- is stated once, in csrc/ldpc_tiles.hpp (the six kernels in ldpc_stream.hip), for run<T, ALG>, run16<ALG> and SLQMSA's run_chunk<T>:
telling lines and the names the copies once carried, counted over the two source files and the header.  (ldpc_admm.hip reads
LDPC_STREAM_REPACK_FILL with a rule of its own and is not counted.)  No GPU."""
import os

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ldpc_decoders_amd", "csrc")
HEADER = "ldpc_tiles.hpp"
USERS = ("ldpc_stream.hip", "ldpc_slq.hip")


def _texts():
    out = {}
    for name in USERS + (HEADER,):
        with open(os.path.join(CSRC, name)) as fp:
            out[name] = fp.read()
    return out


def test_the_source_states_the_machinery_once():
    texts = _texts()
    for needle in ('getenv("LDPC_STREAM_REPACK_FILL")',       # the repack policy
                   "pending.size() >= 2",                      # the drain condition of the poll ring
                   "int64_t plane_at(int tile, int64_t v, int n) {"):  # the tile helpers
        counts = {name: text.count(needle) for name, text in texts.items()}
        assert counts == {"ldpc_stream.hip": 0, "ldpc_slq.hip": 0, HEADER: 1}, (needle, counts)


def test_no_copy_keeps_its_old_name():
    for name, text in _texts().items():
        for gone in ("k_slq_syndrome", "k_slq_unpack", "k_slq_finish_iters", "k_slq_init_live", "SlqRepackPolicy"):
            assert gone not in text, (name, gone)


def test_both_decoders_use_the_header_and_the_library_builds_with_it():
    texts = _texts()
    for name in USERS:
        assert '#include "%s"' % HEADER in texts[name], name
    with open(os.path.join(CSRC, "Makefile")) as fp:
        assert HEADER in fp.read().split("HDRS :=")[1].splitlines()[0]

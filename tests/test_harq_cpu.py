"""The HARQ schedule on the host (ldpc_decoders_amd/ratematch.py ``Harq``, ``rv_starts``), the command-line flags and their refusals, the
run ids with and without a schedule, the ABI declarations, and the extra counter words of ``montecarlo.DeviceSimulator`` with a stand-in
handle.  No GPU: every refusal of ``main.test`` asserted here is raised before a decoder exists."""
import os
import re

import numpy as np
import pytest

import harq_oracle as HO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rm():
    from ldpc_decoders_amd import ratematch

    return ratematch


def _args(line):
    from ldpc_decoders_amd import main

    return main.build_parser().parse_args(line.split())


# ---------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("Ncb", [1, 3, 7, 64])
def test_tables_against_enumeration(Ncb):
    """cnt / first of every (E, k) of the edge list against the enumeration of the sent positions, the transmissions of one schedule taken
    together (so ``first`` sums over real predecessors); the buffer sits between punctured and shortened variables."""
    rm = _rm()
    n = Ncb + 5
    punct, short = [0, 2, 4 if Ncb >= 3 else n - 2], [1, n - 1]
    p = rm.Pattern(n, punct, short)
    assert p.n_tx == Ncb
    cases = [(E, k) for E in sorted({1, max(Ncb - 1, 1), Ncb, Ncb + 1, 2 * Ncb + 3}) for k in sorted({0, Ncb - 1})]
    bits, starts = [E for E, _ in cases], [k for _, k in cases]
    h = rm.Harq(p, bits, starts)
    cnt, first = HO.tables(p.kind, bits, starts)
    assert h.T == len(cases) and h.Ncb == Ncb and h.buffer.tolist() == np.flatnonzero(p.kind == 0).tolist()
    assert h.cnt.dtype == np.uint8 and h.first.dtype == np.uint8 and h.cnt.shape == (h.T, n) == h.first.shape
    assert np.array_equal(h.cnt, cnt) and np.array_equal(h.first, first)
    assert not h.cnt[:, punct + short].any() and not h.first[:, punct + short].any()
    assert h.cnt.sum(axis=1).tolist() == bits  # every sent bit is a copy of some variable
    for t in range(h.T):
        for pos in range(Ncb):
            assert h.copies(t, pos) == cnt[t, h.buffer[pos]] and h.first_copy(t, pos) == first[t, h.buffer[pos]]
    # one transmission alone: first is zero
    for E, k in cases:
        one = rm.Harq(p, [E], [k])
        assert np.array_equal(one.cnt, HO.tables(p.kind, [E], [k])[0]) and not one.first.any()


def test_default_starts_are_chase_and_the_specs():
    rm = _rm()
    p = rm.Pattern(10, [0], [9])
    h = rm.Harq(p, (5, 8, 19))
    assert h.starts == (0, 0, 0) and (h.bits_spec, h.starts_spec) == ("5,8,19", "0,0,0")
    assert h.cnt[2].tolist() == [0, 3, 3, 3, 2, 2, 2, 2, 2, 0]
    assert rm.Harq(p, [5, 8], [7, 3]).starts_spec == "7,3"


def test_schedule_refusals():
    rm = _rm()
    p = rm.Pattern(6, [0], [5])  # Ncb = 4
    for bits, starts in (((), None), ((0,), None), ((3, -1), None), ((1,) * 17, None), ((3,), (4,)), ((3,), (-1,)), ((3, 3), (0,)), ((2.5,), None),
                         ("ab", None)):
        with pytest.raises(ValueError):
            rm.Harq(p, bits, starts)
    with pytest.raises(ValueError):
        rm.Harq(rm.Pattern(3, [0, 1], [2]), (1,))  # an empty buffer
    # 255 copies of a variable are the most the byte tables hold: 4 * 255 bits over a buffer of 4 pass, one more does not
    ok = rm.Harq(p, (4 * 200, 4 * 55))
    assert ok.cnt[1].max() == 55 and ok.first[1].max() == 200
    with pytest.raises(ValueError, match="255"):
        rm.Harq(p, (4 * 200, 4 * 55, 1))
    with pytest.raises(ValueError, match="255"):
        rm.Harq(p, (4 * 255 + 1,))
    assert rm.Harq(p, (16,) * 16).first[15].tolist() == [0, 60, 60, 60, 60, 0]


def test_rv_starts():
    rm = _rm()
    assert rm.rv_starts(1200, 4) == (0, 600, 900, 300)
    assert rm.rv_starts(1200, 6) == (0, 600, 900, 300, 0, 600)
    assert rm.rv_starts(1173, 4) == (0, 586, 879, 293)
    assert rm.rv_starts(1173, 4, 27) == (0, 567, 864, 270)
    assert rm.rv_starts(3, 4) == (0, 1, 2, 0) and rm.rv_starts(1, 3) == (0, 0, 0)
    for bad in ((0, 1, 1), (4, 0, 1), (4, 1, 0)):
        with pytest.raises(ValueError):
            rm.rv_starts(*bad)


# ---------------------------------------------------------------------------------------------- the command line
def test_parser_flags_and_grammar():
    from ldpc_decoders_amd import codes

    rm = _rm()
    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA")
    assert (a.harq_bits, a.harq_starts) == (None, None) and rm.harq_from_args(a, rm.Pattern(1200)) is None
    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800,800,400 --harq-starts rv --puncture 0:40")
    code = codes.get_code(a.code)
    h = rm.harq_from_args(a, rm.from_args(a, code))
    assert (h.tx_bits, h.starts, h.Ncb) == ((800, 800, 400), (0, 580, 870), 1160)
    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800,1300 --harq-starts 5,1199")
    h = rm.harq_from_args(a, rm.Pattern(1200))
    assert (h.bits_spec, h.starts_spec) == ("800,1300", "5,1199")
    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800 --harq-starts rv --qc-lift 27")
    assert rm.harq_from_args(a, rm.Pattern(1200)).starts == (0,)
    for bits, starts in (("800,", None), ("a", None), ("-3", None), ("8 0", None), ("800", "0,0"), ("800", "1200"), ("800", "r"), ("0", None),
                         (",".join(["1"] * 17), None)):
        a.harq_bits, a.harq_starts = bits, starts
        with pytest.raises(ValueError):
            rm.harq_from_args(a, rm.Pattern(1200))
    a.harq_bits, a.harq_starts = None, "rv"
    with pytest.raises(ValueError, match="--harq-bits"):
        rm.harq_from_args(a, rm.Pattern(1200))


@pytest.mark.parametrize("line,word", [
    ("biawgn 1200_3_6_rand_ldpc_1 OSD --harq-bits 800", "OSD"),
    ("biawgn 1200_3_6_rand_ldpc_1 GALB --harq-bits 800", "GALB"),
    ("biawgn 1200_3_6_rand_ldpc_1 ADMM --harq-bits 800", "ADMM"),
    ("biawgn 7_4_hamming ML --harq-bits 7", "ML"),
    ("bec 1200_3_6_rand_ldpc_1 MSA --harq-bits 800", "bec"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800 --exact", "--exact"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800 --prior-grid 4", "--prior-grid"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800 --shorten 3 --codeword 1", "all-one"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800 --puncture 0:1200", "stopping set"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-starts 0", "--harq-bits"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800,x", "--harq-bits"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 800 --harq-starts 1200", "--harq-starts"),
    ("biawgn 1200_3_6_rand_ldpc_1 MSA --harq-bits 400000", "255"),
])
def test_main_refuses_before_a_decoder_exists(line, word, tmp_path):
    from ldpc_decoders_amd import main

    with pytest.raises(SystemExit) as e:
        main.test(_args(line + " --data_dir " + str(tmp_path)))
    assert word in str(e.value), str(e.value)


def test_run_ids_without_the_flags_are_the_parents(tmp_path):
    """Literal strings: without --harq-bits neither the keys nor the file names move, with or without a pattern."""
    from ldpc_decoders_amd import codes, main, models, ratematch, utils

    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA --params 2.0")
    keys, vals = main.run_ids(a, models.models["biawgn"].MSA.id_keys)
    assert keys == ["channel", "code", "decoder", "codeword", "min_wec", "max_iter"]
    assert os.path.basename(utils.Saver(str(tmp_path), list(zip(keys, vals))).file_path) == "biawgn-1200_3_6_rand_ldpc_1-MSA-0-100-10.json"
    a = _args("biawgn 1200_3_6_rand_ldpc_1 MSA --puncture 10:20,3,4 --shorten 1199")
    keys, vals = main.run_ids(a, models.models["biawgn"].MSA.id_keys, ratematch.from_args(a, codes.get_code(a.code)))
    assert keys[-2:] == ["puncture", "shorten"]
    assert os.path.basename(utils.Saver(str(tmp_path), list(zip(keys, vals))).file_path) == "biawgn-1200_3_6_rand_ldpc_1-MSA-0-100-10-3:5,10:20-1199.json"


def test_run_ids_with_a_schedule(tmp_path):
    from ldpc_decoders_amd import codes, main, models, ratematch, utils

    a = _args("biawgn 1200_3_6_rand_ldpc_1 LQMSA --harq-bits 800,800,800 --harq-starts rv")
    p = ratematch.Pattern(1200)
    h = ratematch.harq_from_args(a, p)
    keys, vals = main.run_ids(a, models.models["biawgn"].LQMSA.id_keys, p, h)
    assert keys[-4:] == ["puncture", "shorten", "harq_bits", "harq_starts"] and vals[-4:] == ["none", "none", "800,800,800", "0,600,900"]
    assert os.path.basename(utils.Saver(str(tmp_path), list(zip(keys, vals))).file_path) \
        == "biawgn-1200_3_6_rand_ldpc_1-LQMSA-0-100-10-6-2-0.8125-0.0-none-none-800,800,800-0,600,900.json"
    a = _args("bsc 1200_3_6_rand_ldpc_1 MSA --puncture 0:40 --shorten 1199 --harq-bits 1159,500")
    p = ratematch.from_args(a, codes.get_code(a.code))
    keys, vals = main.run_ids(a, models.models["bsc"].MSA.id_keys, p, ratematch.harq_from_args(a, p))
    assert os.path.basename(utils.Saver(str(tmp_path), list(zip(keys, vals))).file_path) \
        == "bsc-1200_3_6_rand_ldpc_1-MSA-0-100-10-0:40-1199-1159,500-0,0.json"
    assert (a.harq_bits, a.harq_starts) == ("1159,500", None)  # the namespace stays as parsed


def test_harq_record():
    from ldpc_decoders_amd import main

    # 100 frames: 60 acknowledged at once, 25 at the second transmission, 5 at the third, 10 never; 2 acknowledged wrongly
    rec = dict(main.harq_record([60, 25, 5, 2, 800 * (100 + 40 + 15)], 3, dict(tot=100, wec=12), 600))
    assert rec["ack"] == [60, 25, 5] and rec["undetected"] == 2 and rec["sym"] == 124000
    assert rec["avg_tx"] == pytest.approx(1.55) and rec["tput"] == pytest.approx(88 * 600 / 124000)


# ---------------------------------------------------------------------------------------------- the ABI
def test_abi_declarations():
    from ldpc_decoders_amd import _lib

    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as fp:
        text = fp.read()
    for name, nargs in (("ldpc_harq_transmit", 21), ("ldpc_harq_syndrome", 5), ("ldpc_harq_tally", 16)):
        m = re.search(r"\nint %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "Makefile")) as fp:
        mk = fp.read()
    assert "ldpc_harq.hip" in mk and "ldpc_harq.hpp" in mk
    with open(os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "ldpc_api.hip")) as fp:
        api = fp.read()
    for name in ("ldpc_harq_transmit", "ldpc_harq_syndrome", "ldpc_harq_tally"):
        assert re.search(r"^int %s\([^{]*\{\s*return guarded\(\"%s\"" % (name, name), api, re.M), name


def test_library_exports_the_symbols():
    from ldpc_decoders_amd import _lib

    lib = _lib.load()
    for name in ("ldpc_harq_transmit", "ldpc_harq_syndrome", "ldpc_harq_tally"):
        assert hasattr(lib, name)


# ---------------------------------------------------------------------------------------------- the simulator's extra words
class _StandIn:
    """A handle that counts by rule, on the CPU: every frame is one frame, frame f fails when f % 10 == 0; with ``extra`` words it adds
    (frames, frame0 of the call, 7) behind the histogram."""

    def __init__(self, extra=None):
        if extra is not None:
            self.extra_counters = extra
        self.rows = []

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        self.rows.append(counters.numel())
        bad = sum(1 for f in range(frame0, frame0 + B) if f % 10 == 0)
        counters[0] += B
        counters[1] += bad
        counters[2] += 3 * bad
        counters[3] += 2 * B
        if hist_bins:
            counters[4 + min(2, hist_bins - 1)] += B
        if hasattr(self, "extra_counters"):
            counters[4 + hist_bins] += B
            counters[4 + hist_bins + 1] += frame0
            counters[4 + hist_bins + 2] += 7


@pytest.mark.parametrize("bins", [0, 4])
def test_simulator_sums_the_extra_words(bins):
    from ldpc_decoders_amd.montecarlo import DeviceSimulator

    h = _StandIn(extra=3)
    sim = DeviceSimulator(h, "biawgn", 10, hist_bins=bins, device="cpu")
    seen = []
    out = sim.run_point(1.0, 0, min_wec=25, batch_per_rank=100, on_progress=lambda tot, wec, bec, hist: seen.append(None if hist is None else list(hist)))
    assert set(h.rows) == {4 + bins + 3}
    assert (out["tot"], out["wec"], out["bec"], out["iter_sum"]) == (300, 30, 90, 600)
    assert out["extra"] == [300, 0 + 100 + 200, 21]
    if bins:
        assert out["hist"] == [0, 0, 300, 0] and seen[-1] == [0, 0, 300, 0]
    else:
        assert "hist" not in out and seen[-1] is None
    with pytest.raises(ValueError):
        DeviceSimulator(h, "biawgn", 10, device="cpu", prior_grid=4)


@pytest.mark.parametrize("bins", [0, 4])
def test_simulator_without_the_attribute_is_the_parents(bins):
    from ldpc_decoders_amd.montecarlo import DeviceSimulator

    h = _StandIn()
    sim = DeviceSimulator(h, "biawgn", 10, hist_bins=bins, device="cpu")
    out = sim.run_point(1.0, 0, min_wec=25, batch_per_rank=100)
    assert set(h.rows) == {4 + bins}
    assert sorted(out) == sorted(["tot", "wec", "bec", "iter_sum", "capped"] + (["hist"] if bins else []))
    assert (out["tot"], out["wec"], out["bec"], out["iter_sum"], out["capped"]) == (300, 30, 90, 600, False)
    assert sim.run_round(1.0, 0, 0, 50).shape == (4 + bins,)

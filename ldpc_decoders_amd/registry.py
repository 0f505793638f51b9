"""THE table of the decoder names this build knows: one row per name, in the order the command line lists them.

Everything that is a fact about a NAME is a column here -- the class behind it, what the bec says to it, what ``main.test`` may do with
it -- and everything that used to repeat those facts is derived: the wrapper classes of ``biawgn`` / ``bsc``, the refusing classes of
``bec``, the name lists of ``models`` (and the parser's choices), the front decoders of ``bpa.OSD``.  A new variant is one row here, plus
its row in the library's own table (``kAlgs``, csrc/ldpc_common.hpp).
"""
from collections import namedtuple

from . import admm, bpa, hard, layered, ml, qc

Row = namedtuple("Row", [
    "name",
    "group",          # which list of ``models`` carries the name: reference (src/utils.py:16), extra, fixed_point, layered, post_processing, quasi_cyclic, layered_fixed_point, streaming_fixed_point, hard_decision
    "backing",        # the bpa / admm class the LLR wrappers of biawgn / bsc hold ({channel: class}: the channel's own class; None: not built)
    "bec_refusal",    # None: the bec module has its own class of this name; else (docstring, sentence) of the class that raises there
    "osd_front",      # may run in front of bpa.OSD (osd_bp)
    "device_words",   # --codeword -1 is drawn on the device (else: the reference's sequential loop on host noise)
    "tie_dominated",  # over the bsc only the reference's fp64 arithmetic reproduces its curves: --precision defaults to f64 there
    "f16",            # accepts --precision f16 (over biawgn / bsc, device noise)
    "prior_grid",     # True: takes --prior-grid (in fp32 over biawgn); False: refused before a decoder exists; None: refused where the device loop would use it
    "pops_layers",    # the ADMMA flag --layers must not reach it (to LMSA ``layers`` is a layering of the checks)
    "refuses_fused",  # --backend fused is refused before a decoder exists
    "hard",           # decodes hard decisions (one bit per message): words drawn on the device, no --precision f16, no --prior-grid, --max-iter >= 1
    "pattern",        # takes a transmission pattern (--puncture / --shorten, ratematch.Pattern): its handle decodes LLR priors, so _device.PatternHandle wraps it
    "integer_layered",  # the LDS-resident integer kernel on the layered schedule: words drawn on the device, --layers dropped, no --precision f16, no --prior-grid, no --backend stream
    "integer_streamed",  # the integer kernels on the layered schedule with the state in HBM tiles: words drawn on the device, --layers dropped, no --precision f16, no --prior-grid, no --backend fused
    "quasi_cyclic",   # the shift-addressed integer kernel for quasi-cyclic codes: as integer_layered, and --qc-lift resolved to the code's lifting size
])
Row.__new__.__defaults__ = (None, False, False, False, False, None, False, False, False, False, False, False, False)

ROWS = [
    Row("ML", "reference", {"biawgn": ml.BiawgnML, "bsc": ml.BscML}),
    Row("SPA", "reference", bpa.SPA, osd_front=True, device_words=True, f16=True, pattern=True),
    Row("MSA", "reference", bpa.MSA, osd_front=True, device_words=True, tie_dominated=True, f16=True, prior_grid=True, pattern=True),
    Row("LP", "reference", None),
    Row("ADMM", "reference", admm.ADMM),
    Row("ADMMA", "reference", None),
    # this build's own decoders (no upstream counterpart), wrapped like MSA
    Row("NMSA", "extra", bpa.NMSA,  # corrected (normalised / offset) min-sum
        ("Corrected min-sum has no meaning over the erasure channel: the ternary decoder has no magnitudes to scale or offset.",
         "decoder NMSA (corrected min-sum) does not exist over the bec: the erasure decoder has no magnitudes to correct; use SPA / MSA there"),
        osd_front=True, device_words=True, tie_dominated=True, f16=True, prior_grid=False, pattern=True),
    Row("QMSA", "fixed_point", bpa.QMSA,  # fixed-point min-sum (q-bit saturating messages); its integers are the same in every arithmetic
        ("Fixed-point min-sum has no meaning over the erasure channel either: the ternary decoder has no magnitudes to quantise.",
         "decoder QMSA (fixed-point min-sum) does not exist over the bec: the erasure decoder has no magnitudes to quantise; use SPA / MSA there"),
        osd_front=True, device_words=True, f16=True, prior_grid=False, pattern=True),
    Row("LMSA", "layered", bpa.LMSA,  # layered (serial-C) corrected min-sum on the streaming kernels
        ("Layered min-sum is corrected min-sum on another schedule: it has no meaning over the erasure channel either.",
         "decoder LMSA (layered corrected min-sum) does not exist over the bec: the erasure decoder has no magnitudes to correct; use SPA / MSA there"),
        osd_front=True, device_words=True, tie_dominated=True, prior_grid=False, pops_layers=True, refuses_fused=True, pattern=True),
    # LQMSA's contract with the integer state in HBM tiles, for the codes beyond the LDS; bec writes its own (refusing) class of this name
    Row("SLQMSA", "streaming_fixed_point", layered.SLQMSA, integer_streamed=True, pattern=True),
    Row("OSD", "post_processing", bpa.OSD,  # BP + ordered-statistics decoding of the frames BP fails on (NMSA in front)
        ("Ordered-statistics post-processing orders soft values; over the erasure channel ``ML`` (elimination of the erased bits) is exact.",
         "decoder OSD (BP + ordered-statistics post-processing) does not exist over the bec: use ML there, the elimination decoder is exact"),
        device_words=True, tie_dominated=True, prior_grid=False, pops_layers=True, pattern=True),
    # LQMSA's contract on a quasi-cyclic code with the block rows as layers, shift-addressed; bec writes its own (refusing) class of this name
    Row("QCMSA", "quasi_cyclic", qc.QCMSA, quasi_cyclic=True, pattern=True),
    # QMSA's integer rule on LMSA's schedule, the frame resident in the LDS as integers; bec writes its own (refusing) class of this name
    Row("LQMSA", "layered_fixed_point", layered.LQMSA, integer_layered=True, pattern=True),
    # hard-decision decoding of the received bits (bit-sliced Gallager-B); biawgn / bsc / bec write their own class of this name, as for ADMM
    Row("GALB", "hard_decision", hard.GALB, hard=True),
]
BY_NAME = {r.name: r for r in ROWS}


def names(group):
    return [r.name for r in ROWS if r.group == group]


def osd_fronts():
    """{name: bpa class} of the decoders that may run in front of ``bpa.OSD``."""
    return {r.name: r.backing for r in ROWS if r.osd_front}


def _llr_wrapper(name, base, backing, module):
    def __init__(self, param, _code, **kwargs):
        base.__init__(self, param, backing(_code, **kwargs))

    return type(name, (base,), {"id_keys": backing.id_keys, "__init__": __init__, "__module__": module})


def add_llr_wrappers(namespace, base):
    """``class NAME(base)`` holding ``backing(_code, **kwargs)`` for every row with a backing class, into a channel module's namespace
    (a name the module defines itself -- ADMM, which has its own decode_batch and stats -- is left alone)."""
    for row in ROWS:
        if isinstance(row.backing, type) and row.name not in namespace:
            namespace[row.name] = _llr_wrapper(row.name, base, row.backing, namespace["__name__"])


def _refusing(name, doc, sentence, id_keys, module):
    def __init__(self, *a, **k):
        raise NotImplementedError(sentence)

    return type(name, (), {"__doc__": doc, "id_keys": id_keys, "__init__": __init__, "__module__": module})


def add_bec_refusals(namespace):
    """The classes of the bec module that raise: the decoders whose rule has nothing to work on over the erasure channel."""
    for row in ROWS:
        if row.bec_refusal is not None:
            namespace[row.name] = _refusing(row.name, row.bec_refusal[0], row.bec_refusal[1], row.backing.id_keys, namespace["__name__"])

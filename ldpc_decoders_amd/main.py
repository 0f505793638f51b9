"""Experiment driver -- the build's counterpart of the reference's ``src/main.py``.

    python -m ldpc_decoders_amd.main <channel> <code> <decoder> [--codeword C --min-wec W --params P.. --max-iter I ..]

Same positional/flag grammar, same logger names, same JSON result files (see ``utils``), so the arg-lines emitted by
the reference's ``simulations.py`` run unchanged and ``graph.py`` reads the outputs.  Differences, all additive:
frames are decoded in batches on the GPU (``--batch`` per round and rank, ``--seed`` for the device noise, ``--precision`` /
``--backend`` for the kernels, ``--puncture`` / ``--shorten`` for a transmission pattern and ``--harq-bits`` / ``--harq-starts`` for a retransmission schedule over it
(``ratematch``), ``--max-frames`` to stop a
parameter whose error rate is too low to reach ``--min-wec``); ``--exact``
selects the reference-exact mode (host noise, sequential stopping rule, ``--np-seed``); under ``torchrun`` each rank drives one GPU
and the counters are all-reduced once per round.
"""
import logging
import time
from collections import OrderedDict

import numpy as np

from . import codes, dist, qc, ratematch, utils
from ._device import HarqHandle, PatternHandle, check_pattern_run
from .models import all_decoder_names, models
from .registry import BY_NAME
from .montecarlo import DeviceSimulator, run_point_exact


def run_ids(args, decoder_id_keys, pattern=None, harq=None):
    """-> (id keys, their values): what names a run -- its logger, its result file (``utils.Saver``) and the head of that file.  A
    transmission pattern adds ``puncture`` / ``shorten``, a HARQ schedule ``harq_bits`` / ``harq_starts`` behind them; without either the
    keys are exactly the reference's and the decoder's own."""
    id_keys = ["channel", "code", "decoder", "codeword", "min_wec"] + list(decoder_id_keys)
    id_val = [vars(args)[key] for key in id_keys]
    if pattern is not None:  # (the canonical spec strings, block columns merged in, so two patterns never share a file; ``args`` stays as parsed)
        id_keys, id_val = id_keys + ["puncture", "shorten"], id_val + [pattern.puncture_spec or "none", pattern.shorten_spec or "none"]
    if harq is not None:  # (the canonical strings too: ``rv`` is written out as the starts it stands for)
        id_keys, id_val = id_keys + ["harq_bits", "harq_starts"], id_val + [harq.bits_spec, harq.starts_spec]
    return id_keys, id_val


def harq_record(extra, T, c, K):
    """What a HARQ point adds to its record, from the ``extra`` words of ``DeviceSimulator.run_point`` (ack[T], undetected, sym): ``avg_tx``
    is decode attempts per frame, ``tput`` the information bits delivered per transmitted symbol, ``(tot - wec) K / sym``."""
    ack, undetected, sym = [int(a) for a in extra[:T]], int(extra[T]), int(extra[T + 1])
    tot, wec = int(c["tot"]), int(c["wec"])
    attempts = sum((tot - sum(ack[:t])) for t in range(T))
    return [("ack", ack), ("undetected", undetected), ("sym", sym), ("avg_tx", attempts / tot if tot else 0.),
            ("tput", (tot - wec) * K / sym if sym else 0.)]


def test(args, comm=None):
    comm = comm or dist.Comm()
    model = models[args.channel]
    dec_fac = getattr(model, args.decoder)
    row = BY_NAME[args.decoder]  # what this driver may do with the name
    if row.integer_layered or row.quasi_cyclic:  # (an integer kernel in the LDS: refused before a decoder exists)
        if args.precision == "f16":
            raise SystemExit("--precision f16: %s keeps int16 marginals and int8 messages in the LDS and has no arithmetic to store in fp16" % row.name)
        if getattr(args, "prior_grid", None) is not None:
            raise SystemExit("--prior-grid: fp32 min-sum over BI-AWGN (biawgn <code> MSA, without --precision f64); %s quantises its priors itself" % row.name)
        if args.backend == "stream":
            raise SystemExit("--backend stream: %s is LDS-resident (--backend auto / fused); layered min-sum on the streaming kernels is LMSA" % row.name)
    if row.integer_streamed:  # (integer tiles in HBM: refused before a decoder exists)
        if args.precision == "f16":
            raise SystemExit("--precision f16: %s keeps int16 marginals and int8 messages and has no arithmetic to store in fp16" % row.name)
        if getattr(args, "prior_grid", None) is not None:
            raise SystemExit("--prior-grid: fp32 min-sum over BI-AWGN (biawgn <code> MSA, without --precision f64); %s quantises its priors itself" % row.name)
        if args.backend == "fused":
            raise SystemExit("--backend fused: %s runs on the streaming kernels (--backend auto / stream); the LDS-resident integer kernel is LQMSA" % row.name)
    code = codes.get_code(args.code)
    if row.quasi_cyclic:  # (the result file carries the lifting size the decoder runs with, not the 0 that asks for it)
        try:
            base, args.qc_lift = qc.resolve(code, args.qc_lift)
        except ValueError as e:
            raise SystemExit("QCMSA: %s (LQMSA decodes any code)" % e)
        try:
            qc.check_pack(getattr(args, "qc_pack", 0), args.qc_lift, qc.frame_bytes(code, base))
        except ValueError as e:
            raise SystemExit("--qc-pack: %s" % e)
    # a transmission pattern (--puncture / --shorten and their block-column forms; ratematch.Pattern): everything it cannot be combined with
    # is refused here, before a decoder exists; without the flags nothing below differs from a run of the mother code
    try:
        pattern = ratematch.from_args(args, code)
    except ValueError as e:
        raise SystemExit("--puncture / --shorten: %s" % e)
    harq_flags = getattr(args, "harq_bits", None) is not None or getattr(args, "harq_starts", None) is not None
    if harq_flags and pattern is None:  # (a schedule without pattern flags runs over the empty pattern: every bit is in the buffer)
        pattern = ratematch.Pattern(code.n)
    if pattern is not None:
        if not row.pattern:
            raise SystemExit("--puncture / --shorten: %s takes no transmission pattern; the LLR decoders do (%s)"
                             % (row.name, ", ".join(r.name for r in BY_NAME.values() if r.pattern)))
        try:
            check_pattern_run(args.channel, bool(args.exact), getattr(args, "prior_grid", None))
        except ValueError as e:
            raise SystemExit("--puncture / --shorten: %s" % e)
        if not 0.0 < args.short_llr < float("inf"):
            raise SystemExit("--short-llr must be finite and > 0")
        if args.codeword == 1 and pattern.shortened.size:
            raise SystemExit("--codeword 1: the all-one word is no codeword of a shortened code (a shortened bit is 0)")
        lost = pattern.unrecoverable(code)
        if lost.size:
            raise SystemExit("--puncture: the punctured set contains a stopping set -- no BP decoder can recover variable %d (and %d more)"
                             % (lost[0], lost.size - 1))
    # a HARQ schedule over the pattern (--harq-bits / --harq-starts; ratematch.Harq): refused where the pattern is, and for OSD
    harq = None
    if harq_flags:
        if row.group == "post_processing":
            raise SystemExit("--harq-bits: OSD always returns a codeword, so the acknowledgement rule (a satisfied syndrome) never asks for a retransmission")
        try:
            harq = ratematch.harq_from_args(args, pattern)
        except ValueError as e:
            raise SystemExit("--harq-bits / --harq-starts: %s" % e)
        if len(args.params) > 65536:  # (the parameter index is the stream id, and the copy ordinal lives above its 16 bits)
            raise SystemExit("--harq-bits: at most 65536 parameters in one run")
    id_keys, id_val = run_ids(args, dec_fac.id_keys, pattern, harq)
    log = logging.getLogger(".".join(utils.strl(id_val)))
    code_n = code.get_n()
    n_counted = code_n if pattern is None else pattern.n_counted  # (a shortened bit is known: its errors are not counted, nor is it a bit of the BER)
    saver = utils.Saver(args.data_dir, list(zip(id_keys, id_val))) if comm.is_root else None
    # --codeword -1 (a random codeword per frame, src/main.py:38): on the device for the BP decoders -- from the code book where the code
    # has one, from the systematic GF(2) encoder (Code.encoder()) otherwise -- and for ML over the BEC of a code without a code book (the
    # elimination decoder, encoder words); the reference's sequential loop on host noise for the others
    device_words = row.device_words or row.hard or row.integer_layered or row.integer_streamed or row.quasi_cyclic or (args.channel == "bec" and args.decoder == "ML" and code.gen_mtx is None)
    exact = bool(args.exact) or (args.codeword == -1 and not device_words)
    if exact and comm.world > 1:
        raise SystemExit("--exact / --codeword -1 follow the reference's sequential rule and run on a single rank")
    if exact and args.np_seed is not None:
        np.random.seed(args.np_seed)
    kwargs = dict(vars(args))
    if row.pops_layers or row.integer_layered or row.integer_streamed or row.quasi_cyclic:
        kwargs.pop("layers", None)  # (--layers is ADMMA's network shape, src/utils.py:43: not a layering of the checks; LMSA takes the greedy one)
    # fp32 message arithmetic in the throughput mode -- except min-sum over the BSC: every LLR is +-L there, the decoder is
    # tie-dominated and only the reference's fp64 arithmetic reproduces its curves
    # (fixed-point min-sum is no exception: its integers are the same in every arithmetic)
    tie_dominated = args.channel == "bsc" and row.tie_dominated  # (OSD: NMSA in front)
    kwargs["precision"] = args.precision or ("f64" if (exact or tie_dominated) else "f32")
    # (OSD orders the soft output of an f32 / f64 decoder: fp16 storage keeps none in the decoder's type)
    if row.hard:  # (one bit per message: nothing of a precision, a prior grid or an unbounded run applies; refused before a decoder exists)
        if args.precision == "f16":
            raise SystemExit("--precision f16: GALB passes one bit per message and has no arithmetic to store in fp16")
        if getattr(args, "prior_grid", None) is not None:
            raise SystemExit("--prior-grid: fp32 min-sum over BI-AWGN (biawgn <code> MSA, without --precision f64); GALB reads no priors")
        if args.max_iter <= 0:
            raise SystemExit("--max-iter must be >= 1 for GALB: a hard-decision decoder may oscillate for ever and has no exit of its own")
    if kwargs["precision"] == "f16" and (not row.f16 or args.channel == "bec" or exact):
        raise SystemExit("--precision f16 (fp16 storage of the messages): the LLR decoders SPA / MSA over biawgn / bsc, device-noise mode")
    if row.refuses_fused and args.backend == "fused":  # (refused before a decoder exists, like the two around it)
        raise SystemExit("--backend fused: layered min-sum (LMSA) runs on the streaming kernels (--backend auto / stream)")
    # (NMSA, and OSD with NMSA in front: a scale takes values off the grid; QMSA quantises its priors itself; refused before a decoder exists)
    if getattr(args, "prior_grid", None) is not None and row.prior_grid is False:
        raise SystemExit("--prior-grid: fp32 min-sum over BI-AWGN (biawgn <code> MSA, without --precision f64)")
    results = OrderedDict()

    for pi, param in enumerate(args.params):
        log.info("Starting parameter: %f" % param)
        channel = model.Channel(param)
        decoder = dec_fac(param, code, **kwargs)
        state = dict(t=time.time())

        def log_status(c, final=False):
            tot, wec, bec = c["tot"], c["wec"], c["bec"]
            wer, ber = (wec / tot, bec / (tot * n_counted)) if tot else (0., 0.)
            keys = ["tot", "wec", "wer", "bec", "ber"]
            vals = [int(tot), int(wec), float(wer), int(bec), float(ber)]
            if comm.is_root:
                log.info(", ".join("%s:%s" % (k.upper(), v) for k, v in zip(keys, vals)))
            if hasattr(decoder, "stats"):  # e.g. the ADMM iteration histogram (src/main.py:34)
                keys.append("dec"), vals.append(decoder.stats())
            if c.get("harq"):  # a HARQ point: acknowledgements per transmission, undetected errors, symbols, mean transmissions, throughput
                for k, v in c["harq"]:
                    keys.append(k), vals.append(v)
            if c.get("capped"):  # an addition: the point was stopped by --max-frames before reaching --min-wec
                keys.append("capped"), vals.append(True)
            if comm.is_root:
                saver.add(param, OrderedDict(zip(keys, vals)))
            return OrderedDict(zip(keys, vals))

        def progress(tot, wec, bec, hist=None):
            if time.time() - state["t"] > args.log_freq:
                state["t"] = time.time()
                if hist is not None and state.get("hist_into") is not None:  # the decoder's own histogram follows the reduced counters
                    into, bins = state["hist_into"]
                    into[:] = 0
                    into[:bins] = hist[:bins]
                log_status(dict(tot=tot, wec=wec, bec=bec))

        inner = decoder if hasattr(decoder, "handle") else getattr(decoder, "dec", None)
        on_device = hasattr(getattr(inner, "handle", None), "simulate")  # BP and ML: channel + decode + count on the GPU
        if not exact and not on_device and comm.world > 1:
            raise SystemExit("decoder %s runs its Monte-Carlo loop on host noise and a single rank" % args.decoder)
        if exact or not on_device:
            pick = None
            if args.codeword == -1:
                pick = lambda: code.cb[np.random.choice(code.cb.shape[0], 1)[0]]  # noqa: E731  (src/main.py:38)
                x = code.cb[0]
            else:
                x = np.zeros(code_n, dtype=np.int64) + args.codeword
            # one frame per call keeps numpy's stream in the reference's order (send, [ML pick], send, ..)
            if exact:
                chunk = 1 if (code_n < 64 or args.decoder in ("ML", "ADMM")) else 32
            else:  # a decoder without a device Monte-Carlo path: host noise, frames decoded in batches
                chunk = max(1, min(args.batch, 4096))
            c = run_point_exact(channel, decoder, x, args.min_wec, chunk=chunk, on_progress=progress, pick_word=pick)
        else:
            handle = decoder.handle if hasattr(decoder, "handle") else decoder.dec.handle
            if harq is not None:
                handle = HarqHandle(handle, harq, args.short_llr)
            elif pattern is not None:
                handle = PatternHandle(handle, pattern, args.short_llr)
            # a decoder that reports statistics (ADMM: iteration histogram, src/main.py:34) gets them from the REDUCED counters, so
            # that `dec` describes the same frames as tot/wec/bec -- the whole job, not rank 0's shard
            own_hist = hasattr(decoder, "stats") and hasattr(inner, "iter")
            bins = min(len(inner.iter), args.max_iter + 1 if args.max_iter > 0 else len(inner.iter)) if own_hist else 0
            if own_hist:
                handle.on_iters = None
                state["hist_into"] = (inner.iter, bins)  # intermediate result files then carry a real histogram, not zeros
            grid = getattr(args, "prior_grid", None)
            if grid is not None and (row.prior_grid is not True or args.channel != "biawgn" or kwargs["precision"] != "f32"):
                raise SystemExit("--prior-grid: fp32 min-sum over BI-AWGN (biawgn <code> MSA, without --precision f64)")
            sim = DeviceSimulator(handle, args.channel, args.max_iter, args.codeword, args.seed, comm, hist_bins=bins, prior_grid=grid)
            c = sim.run_point(param, stream_id=pi, min_wec=args.min_wec, batch_per_rank=args.batch, on_progress=progress,
                              max_frames=(args.max_frames or None))
            if harq is not None:
                c["harq"] = harq_record(c["extra"], harq.T, c, pattern.shortened_code(code)[0].encoder().k)
            if own_hist:
                inner.iter[:] = 0
                inner.iter[:bins] = c["hist"]
            if grid is not None and comm.is_root:
                log.info("prior grid 2^-%d: %d of %d frames were beyond the fp32 exactness guard and decoded again in fp64" % (grid, sim.redone, c["tot"]))
        results[param] = log_status(c, final=True)
    log.info("Done!")
    return results


def build_parser():
    """The reference's grammar with the reference's decoder names, plus this build's own (``registry.ROWS``: NMSA, QMSA, LMSA, SLQMSA, OSD, QCMSA, LQMSA, GALB)."""
    return utils.setup_parser(codes.get_code_names(), models.keys(), all_decoder_names)


def main(argv=None):
    args = build_parser().parse_args(argv)
    comm = dist.init_from_env()
    log_level = logging.DEBUG if args.debug else logging.INFO
    if args.console:
        utils.setup_console_logger(log_level)
    else:
        utils.make_dir_if_not_exists(args.data_dir)
        utils.setup_file_logger(args.data_dir, "test", log_level)
    if comm.is_root:
        print(vars(args))
    try:
        return test(args, comm)
    finally:
        dist.finalize()


if __name__ == "__main__":
    # np.random is deliberately left unseeded, as upstream (src/main.py:68); use --np-seed / --seed for repeatability
    main()

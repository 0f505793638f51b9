"""What a transmission pattern (ratematch.Pattern, ldpc_channel_pattern, _device.PatternHandle) costs and what it does to a curve, on one
GPU; writes profiles/r18_ratematch.md.

    python tools/ratematch_rate.py [--reps R] [--out FILE]

(a) the channel kernel: ldpc_channel_pattern with an all-sent pattern against ldpc_channel_sent on the same words, 65 536 x 1200 fp32 over
    BI-AWGN, interleaved, HIP events around each launch, median / min / max of R (>= 3) after a warm-up launch of each;
(b) the whole pass: PatternHandle with an empty pattern against the inner handle's own simulate, 65 536 frames at 2.0 dB, cap 50, wall
    clock around the call and a synchronise, median of R after a counted warm-up; the counters of the two are compared;
(c) rate curves: QCMSA on one 12 x 24 dv = 3 mask at Z = 27 (generated here with a fixed seed; not a standard's), all sent and with 2 and
    4 parity block columns punctured, the columns chosen so that every check sees one punctured bit (``unrecoverable`` is empty)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, SNR, CAP, SEED = 65536, 1200, 2.0, 50, 2025
CURVE_SNRS = (1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0)
CURVE_FRAMES = 4 * 65536
PUNCTURED_COLUMNS = {0: [], 2: [12, 18], 4: [12, 15, 18, 21]}  # column j of regular_mask(12, 24, 3) meets block rows j, j + 1, j + 2 (mod 12)


def _event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _wall_ms(fn):
    import torch

    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def channel_times(reps):
    """-> {name: (median, min, max) ms} of one launch at B x N fp32"""
    import torch

    from ldpc_decoders_amd import _device

    words = torch.randint(0, 2, (B, N), dtype=torch.uint8, device="cuda")
    kind = torch.zeros(N, dtype=torch.uint8, device="cuda")
    runs = {"ldpc_channel_sent": lambda: _device.channel_sent("biawgn", "f32", SNR, words, SEED, 0, 0),
            "ldpc_channel_pattern, all sent": lambda: _device.channel_pattern("biawgn", "f32", SNR, words, 0, kind, 32.0, SEED, 0, 0)}
    a, b = (fn()[0] for fn in runs.values())  # the warm-up launches; the outputs are the same bits
    assert torch.equal(a, b)
    del a, b
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(_event_ms(fn))
    return {k: _stats(v) for k, v in ms.items()}


def pass_rates(reps):
    """-> rows (decoder, code, inner counters, (median, min, max) ms of inner.simulate, the same of PatternHandle.simulate)"""
    import numpy as np
    import torch

    from ldpc_decoders_amd import _device, _lib, codes, qc, ratematch

    code = codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, "1200_3_6_rand_ldpc_1.txt"))
    qcode = qc.rand_qc_ldpc(qc.regular_mask(12, 24, 3), 27, np.random.RandomState(1827))
    cases = [("MSA fp32", "1200_3_6_rand_ldpc_1", lambda: _device.DecoderHandle(code, "MSA", "f32", "auto"), code),
             ("QCMSA, Z = 1", "1200_3_6_rand_ldpc_1", lambda: _device.QcHandle(code, 1), code),
             ("LQMSA", "1200_3_6_rand_ldpc_1", lambda: _device.LqmsaHandle(code), code),
             ("QCMSA, Z = 27", "12 x 24 mask, n = 648", lambda: _device.QcHandle(qcode, 27), qcode)]
    rows = []
    for name, where, make, c in cases:
        try:
            inner = make()
        except _lib.LdpcHipError as e:
            rows.append((name, where, None, str(e), None))
            continue
        ph = _device.PatternHandle(inner, ratematch.Pattern(c.n))
        cnt = [torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2)]
        runs = [lambda: inner.simulate("biawgn", SNR, 0, SEED, 0, 0, B, CAP, cnt[0]), lambda: ph.simulate("biawgn", SNR, 0, SEED, 0, 0, B, CAP, cnt[1])]
        for fn in runs:
            fn()
        torch.cuda.synchronize()
        counted = [t.cpu().tolist() for t in cnt]
        ms = [[], []]
        for _ in range(reps):
            for i, fn in enumerate(runs):
                ms[i].append(_wall_ms(fn))
        rows.append((name, where, counted, _stats(ms[0]), _stats(ms[1])))
        print(rows[-1], flush=True)
        del inner, ph
    return rows


def curves():
    """-> (n, {punctured columns: [(dB, tot, wec, bec, n_counted)]})"""
    import numpy as np
    import torch

    from ldpc_decoders_amd import _device, qc, ratematch

    code = qc.rand_qc_ldpc(qc.regular_mask(12, 24, 3), 27, np.random.RandomState(1827))
    inner = _device.QcHandle(code, 27)
    out = {}
    for k, cols in PUNCTURED_COLUMNS.items():
        p = ratematch.Pattern(code.n, punctured=ratematch.block_columns(cols, 27))
        assert p.unrecoverable(code).size == 0
        h = _device.PatternHandle(inner, p)
        out[k] = []
        for i, snr in enumerate(CURVE_SNRS):
            cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            h.simulate("biawgn", snr, 0, SEED, i, 0, CURVE_FRAMES, CAP, cnt)
            tot, wec, bec, _ = cnt.cpu().tolist()
            out[k].append((snr, tot, wec, bec, p.n_counted))
            print(k, out[k][-1], flush=True)
    return code.n, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_ratematch.md"))
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("--reps: at least 3 timed launches")
    import torch

    ch = channel_times(a.reps)
    rates = pass_rates(a.reps)
    n, cv = curves()
    sent, pat = ch["ldpc_channel_sent"], ch["ldpc_channel_pattern, all sent"]
    inside = pat[0] <= sent[2] and sent[0] <= pat[2]
    out = ["# Punctured and shortened transmission: the pattern channel, the composed pass, rate curves", "",
           "Written by `python tools/ratematch_rate.py --reps %d` on %s (%d CUs)." % (a.reps, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count), "",
           "## (a) The channel kernel", "",
           "One launch at %d x %d fp32 over BI-AWGN at %.1f dB on given words; HIP events around the launch (it includes the allocation of the output "
           "by the caching allocator), interleaved, median of %d (min-max) after a warm-up launch of each; the two outputs are asserted equal bit "
           "for bit.  The pattern kernel reads n more bytes per frame, from the cache.  In the code the two differ in one more way: `k_biawgn_sent` "
           "reads its four sent bytes and writes its four priors one by one, `k_biawgn_pattern` reads one dword of each and writes one float4 when "
           "n is a multiple of 4, as `k_biawgn` does; no hardware counter was collected to attribute a difference to that." % (B, N, SNR, a.reps), "",
           "| kernel | ms (min-max) | GB/s written |", "|---|---|---|"]
    for k, (med, lo, hi) in ch.items():
        out.append("| %s | %.3f (%.3f-%.3f) | %.0f |" % (k, med, lo, hi, B * N * 4 / (med * 1e-3) / 1e9))
    out += ["", "The pattern kernel's median is %.3f of `ldpc_channel_sent`'s: %s." % (
        pat[0] / sent[0], "each min-max range contains the other's median, i.e. within the run-to-run spread" if inside else
        ("faster, beyond the run-to-run spread" if pat[0] < sent[0] else "slower, beyond the run-to-run spread")), "",
        "## (b) The whole pass: composing in Python against the C pass", "",
        "%d frames at %.1f dB, cap %d, all-zero word, empty pattern; wall clock around `simulate` and a synchronise, interleaved, median of %d "
        "(min-max) after a counted warm-up.  `PatternHandle` writes the priors of a chunk to HBM and reads them back in the decode; the LDS-resident "
        "fp32 min-sum pass draws them inside its kernel, the integer passes run channel kernel + decode + count from C." % (B, SNR, CAP, a.reps), "",
        "| decoder | code | word errors (inner / pattern) | inner.simulate ms (min-max) | frames/s | PatternHandle ms (min-max) | frames/s | pattern / inner |",
        "|---|---|---|---|---|---|---|---|"]
    for name, where, counted, t0, t1 in rates:
        if counted is None:
            out.append("| %s | %s | refused: %s | | | | | |" % (name, where, t0))
            continue
        out.append("| %s | %s | %d / %d%s | %.2f (%.2f-%.2f) | %.3e | %.2f (%.2f-%.2f) | %.3e | %.2f |" % (
            name, where, counted[0][1], counted[1][1], "" if counted[0] == counted[1] else " (counters differ: the fused pass draws in its kernel)",
            t0[0], t0[1], t0[2], B / (t0[0] * 1e-3), t1[0], t1[1], t1[2], B / (t1[0] * 1e-3), t1[0] / t0[0]))
    out += ["", "## (c) Rate curves", "",
            "QCMSA (default parameters, cap %d) on one 12 x 24 dv = 3 mask at Z = 27 (n = %d; generated by the tool, seed 1827), %d frames per point, "
            "all-zero word, dB per TRANSMITTED symbol (no rate correction).  Punctured block columns: %s; every check then sees exactly one punctured "
            "bit, so `unrecoverable` is empty (asserted)." % (CAP, n, CURVE_FRAMES, "; ".join("%d: %s" % (k, c) for k, c in PUNCTURED_COLUMNS.items() if k)), "",
            "| dB | " + " | ".join("%d punctured columns (rate %.3f): WER / BER" % (k, (n // 2) / (n - 27 * k)) for k in cv) + " |", "|---|" + "---|" * len(cv)]
    for i, snr in enumerate(CURVE_SNRS):
        out.append("| %.1f | " % snr + " | ".join("%.3e / %.3e" % (cv[k][i][2] / cv[k][i][1], cv[k][i][3] / (cv[k][i][1] * cv[k][i][4])) for k in cv) + " |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

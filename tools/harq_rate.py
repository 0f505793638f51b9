"""What incremental-redundancy HARQ (ratematch.Harq, csrc/ldpc_harq.hip, _device.HarqHandle) costs and what it buys, on one GPU; writes
profiles/r19_harq.md.

    python tools/harq_rate.py [--reps R] [--frames F] [--out FILE]

(a) the transmit kernel: ldpc_harq_transmit for one non-repeating first transmission (E = Ncb, k = 0, every bit sent) against
    ldpc_channel_pattern of the same library, 65 536 x 1200 fp32 over BI-AWGN on given words, interleaved, HIP events around each launch,
    median / min / max of R (>= 3) after a warm-up launch of each; the two outputs are asserted equal;
(b) throughput and mean transmissions of 1200_3_6_rand_ldpc_1 under LQMSA with E = 800 per transmission, four transmissions, rv starts
    against Chase combining (all starts 0), 0 to 3 dB per transmitted symbol, random codewords;
(c) the share of a point's time spent outside the decoder: HIP events around every ``decode_device`` call of the point against the wall
    clock of the whole ``simulate``."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, SNR, CAP, SEED = 65536, 1200, 2.0, 50, 2026
CODE = "1200_3_6_rand_ldpc_1"
E_TX, T_TX = 800, 4
CURVE_SNRS = (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0)


def _event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def transmit_times(reps):
    """-> {name: (median, min, max) ms} of one launch at B x N fp32"""
    import torch

    from ldpc_decoders_amd import _device, ratematch

    h = ratematch.Harq(ratematch.Pattern(N), [N])
    words = torch.randint(0, 2, (B, N), dtype=torch.uint8, device="cuda")
    kind, cnt, first = (torch.from_numpy(a).cuda() for a in (h.pattern.kind, h.cnt[0], h.first[0]))
    runs = {"ldpc_channel_pattern, all sent": lambda: _device.channel_pattern("biawgn", "f32", SNR, words, 0, kind, 32.0, SEED, 0, 0)[0],
            "ldpc_harq_transmit, first transmission, E = Ncb": lambda: _device.harq_transmit("biawgn", "f32", SNR, words, 0, kind, cnt, first, 32.0, SEED, 0, 0, B)}
    a, b = (fn() for fn in runs.values())  # the warm-up launches; the outputs are the same bits
    assert torch.equal(a, b)
    del a, b
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(_event_ms(fn))
    return {k: _stats(v) for k, v in ms.items()}


class _TimedDecode:
    """The inner handle with HIP events around every ``decode_device``; everything else is the handle's own."""

    def __init__(self, inner):
        self.__dict__["inner"], self.__dict__["spans"] = inner, []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def decode_device(self, *a, **k):
        import torch

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = self.inner.decode_device(*a, **k)
        e1.record()
        self.spans.append((e0, e1))
        return out

    def decode_ms(self):
        import torch

        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in self.spans)
        del self.spans[:]
        return ms


def curves(frames):
    """-> {schedule name: [(dB, counters list, K, wall ms, decode ms)]}"""
    import torch

    from ldpc_decoders_amd import _device, codes, ratematch

    code = codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, CODE + ".txt"))
    pattern = ratematch.Pattern(code.n)
    K = code.encoder().k
    inner = _device.LqmsaHandle(code)
    out = {}
    for name, starts in (("rv starts", ratematch.rv_starts(code.n, T_TX)), ("Chase (all starts 0)", None)):
        harq = ratematch.Harq(pattern, (E_TX,) * T_TX, starts)
        hh = _device.HarqHandle(inner, harq)
        timed = _TimedDecode(inner)
        hh.inner = timed
        out[name] = []
        for i, snr in enumerate(CURVE_SNRS):
            for counted in (False, True):  # a warm-up pass of every point, then the timed one
                cnt = torch.zeros(4 + T_TX + 2, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                t = time.perf_counter()
                hh.simulate("biawgn", snr, -1, SEED, i, 0, frames, CAP, cnt)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t) * 1e3
                dec = timed.decode_ms()
            out[name].append((snr, cnt.cpu().tolist(), K, wall, dec))
            print(name, out[name][-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_harq.md"))
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("--reps: at least 3 timed launches")
    import torch

    tx = transmit_times(a.reps)
    cv = curves(a.frames)
    pat, har = tx["ldpc_channel_pattern, all sent"], tx["ldpc_harq_transmit, first transmission, E = Ncb"]
    inside = pat[1] <= har[0] <= pat[2] and har[1] <= pat[0] <= har[2]
    out = ["# Incremental-redundancy HARQ: the transmit kernel, throughput against Chase combining, time outside the decoder", "",
           "Written by `python tools/harq_rate.py --reps %d --frames %d` on %s (%d CUs)." % (a.reps, a.frames, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count), "",
           "## (a) The transmit kernel", "",
           "One launch at %d x %d fp32 over BI-AWGN at %.1f dB on given words; HIP events around the launch (it includes the allocation of the output "
           "by the caching allocator), interleaved, median of %d (min-max) after a warm-up launch of each; the two outputs are asserted equal bit for "
           "bit.  For a first transmission that sends every bit once the transmit kernel does the draws and stores of the pattern kernel, reads two "
           "more bytes per variable (cnt, first; from the cache) and, with a survivor list, one index per row.  A report, not a gate." % (B, N, SNR, a.reps), "",
           "| kernel | ms (min-max) | GB/s written |", "|---|---|---|"]
    for k, (med, lo, hi) in tx.items():
        out.append("| %s | %.3f (%.3f-%.3f) | %.0f |" % (k, med, lo, hi, B * N * 4 / (med * 1e-3) / 1e9))
    out += ["", "The transmit kernel's median is %.3f of `ldpc_channel_pattern`'s: %s." % (
        har[0] / pat[0], "each min-max range contains the other's median, i.e. within the run-to-run spread" if inside else
        ("faster, beyond the run-to-run spread" if har[0] < pat[0] else "slower, beyond the run-to-run spread")), "",
        "## (b) Throughput and mean transmissions", "",
        "`%s` under LQMSA (default parameters, cap %d), E = %d per transmission, up to %d transmissions, %d frames per point, a random codeword "
        "per frame, dB per TRANSMITTED symbol (no rate correction).  `tput` = (tot - wec) K / sym information bits per transmitted symbol with "
        "K = %d; `avg tx` = decode attempts per frame." % (CODE, CAP, E_TX, T_TX, a.frames, next(iter(cv.values()))[0][2]), "",
        "| dB | " + " | ".join("%s: ack per transmission / never / undetected / avg tx / tput" % k for k in cv) + " |", "|---|" + "---|" * len(cv)]
    for i, snr in enumerate(CURVE_SNRS):
        cells = []
        for k in cv:
            _, c, K, _, _ = cv[k][i]
            tot, wec, ack, und, sym = c[0], c[1], c[4:4 + T_TX], c[4 + T_TX], c[4 + T_TX + 1]
            attempts = sum(tot - sum(ack[:t]) for t in range(T_TX))
            cells.append("%s / %d / %d / %.3f / %.4f" % (ack, tot - sum(ack), und, attempts / tot, (tot - wec) * K / sym))
        out.append("| %.1f | " % snr + " | ".join(cells) + " |")
    out += ["", "## (c) Time outside the decoder", "",
            "Per point of (b): wall clock around `HarqHandle.simulate` and a synchronise (second pass of the point; the first is a warm-up), and the "
            "sum of the HIP-event spans around its `decode_device` calls.  The rest is the encoder of the sent words, the transmit, syndrome and tally "
            "kernels, the survivor list (torch) with its one host read per transmission and chunk, and launch gaps.  No hardware counter was collected.", "",
            "| dB | " + " | ".join("%s: wall ms / decode ms / share outside" % k for k in cv) + " |", "|---|" + "---|" * len(cv)]
    for i, snr in enumerate(CURVE_SNRS):
        out.append("| %.1f | " % snr + " | ".join("%.1f / %.1f / %.2f" % (cv[k][i][3], cv[k][i][4], 1.0 - cv[k][i][4] / cv[k][i][3]) for k in cv) + " |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

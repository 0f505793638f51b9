"""What a one-bit message decoder reaches on one GPU: Gallager-B (ldpc_hard_*) on the LDS-resident kernel and on the streaming kernels,
beside the erasure decoder and fp32 min-sum; writes profiles/r13_galb.md.

    python tools/galb_rate.py [--reps R] [--out FILE] [--skip-64800]

1. With early exit, cap 20, device noise over the BSC through ldpc_hard_simulate / ldpc_simulate: frames/s, mean sweeps and WER of GALB
   (LDS kernel with the graph tables read through L2, the same with 16-bit tables in the LDS -- LDPC_HARD_TABLES=lds --, streaming
   kernels), fp32 MSA and fp32 NMSA (scale 0.8125) on 1200_3_6_rand_ldpc_1 at p = 0.02, 0.03, 0.035 and on a (3,6) n = 64 800 code.
2. At equal sweeps (LDPC_FLAG_NO_EARLY_EXIT, 10 sweeps): GALB on both kernels beside the erasure decoder, with the time per frame-sweep
   against the models of DESIGN.md section 20 (streaming: (5E + 3n + m) / 8 bytes of HBM traffic per frame-sweep; LDS: (7E + 3n + m) / 32
   dword accesses per frame-sweep, 32 per clock and CU).
Every time is the median of R launches between HIP events, after a counted warm-up launch; the decoders of a point are interleaved."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP, FIXED_SWEEPS, SCALE = 20, 10, 0.8125
SEED_OF_GENERATED_CODES = 20261002  # bench.py load_code: the same ensemble member as its config 5
CLOCK_HZ = 2.4e9


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def decoders(code, lds_fits):
    """{label: (handle, channel)} -- every handle has simulate() in one call shape"""
    from ldpc_decoders_amd._device import DecoderHandle, HardHandle

    out = {}
    if lds_fits:
        os.environ.pop("LDPC_HARD_TABLES", None)
        out["GALB, LDS kernel (tables through L2)"] = HardHandle(code, "fused")
        os.environ["LDPC_HARD_TABLES"] = "lds"
        out["GALB, LDS kernel (16-bit tables in the LDS)"] = HardHandle(code, "fused")
        os.environ.pop("LDPC_HARD_TABLES", None)
    out["GALB, streaming kernels"] = HardHandle(code, "stream")
    out["MSA fp32"] = DecoderHandle(code, "MSA", "f32")
    out["NMSA fp32 (scale %s)" % SCALE] = DecoderHandle(code, "NMSA", "f32")
    out["NMSA fp32 (scale %s)" % SCALE].set_correction(SCALE, 0.0)
    return out


def measure(hs, channel_of, param, B, max_iter, flags, reps):
    """-> {label: (tot, wec, mean sweeps, median ms, min ms, max ms)}"""
    import torch

    counted, ms = {}, {k: [] for k in hs}
    for k, h in hs.items():  # the counted launch is the warm-up of the operating point
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        h.simulate(channel_of(k), param, 0, 2024, 0, 0, B, max_iter, cnt, flags=flags)
        torch.cuda.synchronize()
        counted[k] = cnt.cpu().tolist()
    scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
    for _ in range(reps):
        for k, h in hs.items():
            ms[k].append(_timed(lambda: h.simulate(channel_of(k), param, 0, 2024, 0, 0, B, max_iter, scratch, flags=flags)))
    return {k: (counted[k][0], counted[k][1], counted[k][3] / counted[k][0], statistics.median(ms[k]), min(ms[k]), max(ms[k])) for k in hs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_galb.md"))
    ap.add_argument("--skip-64800", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch

    from ldpc_decoders_amd import _lib, codes, hard
    from ldpc_decoders_amd._device import DecoderHandle

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    points = [("1200_3_6_rand_ldpc_1", codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, "1200_3_6_rand_ldpc_1.txt")), 65536, (0.02, 0.03, 0.035))]
    if not a.skip_64800:
        points.append(("(3,6) n = 64 800", codes.rand_reg_ldpc(64800, 3, 6, np.random.RandomState(SEED_OF_GENERATED_CODES)), 8192, (0.03,)))
    out = ["# Gallager-B (GALB): what a one-bit message decoder reaches", "",
           "Written by `python tools/galb_rate.py --reps %d` on %s (%d CUs); HIP-event times of whole simulate launches (channel kernel + decode + "
           "count), median of %d (min-max), after a counted warm-up launch; the decoders of a point are interleaved." % (a.reps, torch.cuda.get_device_name(0), cus, a.reps), "",
           "## 1. With early exit over the BSC, cap %d sweeps, all-zero word, one seed per point" % CAP, "",
           "| code | p | decoder | frames | word errors | WER | mean sweeps | ms (min-max) | frames/s |", "|---|---|---|---|---|---|---|---|---|"]
    fixed = []
    for name, code, B, ps in points:
        fits = hard.hard_lds_bytes(code.m, code.n, code.E) <= hard.LDS_BYTES
        hs = decoders(code, fits)
        for p in ps:
            res = measure(hs, lambda k: "bsc", p, B, CAP, 0, a.reps)
            for k, (tot, wec, its, med, lo, hi) in res.items():
                out.append("| %s | %s | %s | %d | %d | %.3e | %.2f | %.3f (%.3f-%.3f) | %.3e |" % (name, p, k, tot, wec, wec / tot, its, med, lo, hi, tot / (med * 1e-3)))
                print(out[-1], flush=True)
        # equal sweeps: GALB beside the erasure decoder
        eq = {k: h for k, h in hs.items() if k.startswith("GALB")}
        eq["erasure decoder (BEC, eps = 0.4)"] = DecoderHandle(code, "BEC", "f32")
        res = measure(eq, lambda k: "bec" if k.startswith("erasure") else "bsc", 0.03, B, FIXED_SWEEPS, _lib.FLAG_NO_EARLY_EXIT, a.reps)
        # the decode alone (no channel kernel, no count): load + FIXED_SWEEPS sweeps + unload
        y = torch.empty((B, code.n), dtype=torch.uint8, device="cuda")
        _lib.check(_lib.load().ldpc_channel(_lib.CHANNEL["bsc"], 0, 0.03, 0, 2024, 0, 0, B, code.n, None, y.data_ptr(), torch.cuda.current_stream().cuda_stream))
        for k, h in eq.items():
            alone = None
            if k.startswith("GALB"):
                h.decode_device_bits(y, FIXED_SWEEPS, _lib.FLAG_NO_EARLY_EXIT)
                alone = statistics.median(_timed(lambda: h.decode_device_bits(y, FIXED_SWEEPS, _lib.FLAG_NO_EARLY_EXIT)) for _ in range(a.reps))
            fixed.append((name, code, k, B, res[k], alone))
        del hs, eq
    out += ["", "## 2. Equal sweeps: %d sweeps for every frame (LDPC_FLAG_NO_EARLY_EXIT), p = 0.03 (erasure decoder: eps = 0.4)" % FIXED_SWEEPS, "",
            "`decode alone` is `ldpc_hard_decode` with packed output on frames already in HBM (load, sweeps, unload; no channel kernel, no count). "
            "Models (DESIGN.md section 20): streaming (5E + 3n + m) / 8 bytes of HBM traffic per frame-sweep; LDS kernel (7E + 3n + m) / 32 dword "
            "accesses per frame-sweep at 32 per clock and CU (%.1f GHz assumed)." % (CLOCK_HZ / 1e9), "",
            "| code | decoder | frames | simulate ms (min-max) | frames/s | decode alone ms | ns per frame-sweep | against the model |", "|---|---|---|---|---|---|---|---|"]
    for name, code, k, B, (tot, wec, its, med, lo, hi), alone in fixed:
        note, per = "-", "-"
        if alone is not None:
            per_s = alone * 1e-3 / (B * FIXED_SWEEPS)
            per = "%.3f" % (per_s * 1e9)
            if "streaming" in k:
                model = (5 * code.E + 3 * code.n + code.m) / 8
                note = "%d B per frame-sweep -> %.2f TB/s" % (model, model / per_s / 1e12)
            else:
                model = (7 * code.E + 3 * code.n + code.m) / 32 / 32  # CU clocks per frame-sweep
                note = "%.1f CU clocks per frame-sweep in the model, %.1f measured" % (model, per_s * cus * CLOCK_HZ)
        out.append("| %s | %s | %d | %.3f (%.3f-%.3f) | %.3e | %s | %s | %s |" % (name, k, tot, med, lo, hi, tot / (med * 1e-3), "-" if alone is None else "%.3f" % alone, per, note))
        print(out[-1], flush=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

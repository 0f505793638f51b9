"""What the LDS-resident layered fixed-point decoder (LQMSA, ldpc_lqmsa_*) reaches on one GPU; writes profiles/r14_lqmsa.md.

    python tools/lqmsa_rate.py [--reps R] [--out FILE]

1. With early exit, cap 50, device noise, the same Philox frames for every decoder of a point: frames/s, mean executed sweeps and word errors of
   LQMSA (6, 2, 0.8125, 0), QMSA (6, 2, 0.8125, 0) and fp32 NMSA 0.8125 on the LDS-resident kernels (backend auto where a code has no
   LDS-resident shape; the backend that ran is reported) and LMSA 0.8125 on the streaming kernels, interleaved in one process (median of R
   timed simulate launches, HIP events, after a counted warm-up launch).
2. LQMSA under every wave count (LDPC_LQMSA_NW = 1, 2, 4, 8, a fresh handle each): what the rule of ldpc_lqmsa.hpp lqmsa_waves picks against
   the alternatives."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_OF_GENERATED_CODES = 20261002  # bench.py load_code: the same ensemble member as its config 4
SCALE, CAP, FIXED = 0.8125, 50, (6, 2, 0.8125, 0)


def cases():
    import numpy as np

    from ldpc_decoders_amd import codes

    def shipped(name):
        return lambda: codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, name + ".txt"))

    return [("512_3_6_rand_ldpc_1", shipped("512_3_6_rand_ldpc_1"), 65536, 2.5),
            ("1200_3_6_rand_ldpc_1", shipped("1200_3_6_rand_ldpc_1"), 65536, 2.0),
            ("margulis", shipped("margulis"), 65536, 2.0),
            ("irregular n = 10 000", lambda: codes.rand_irregular_ldpc(10000, codes.LAMBDA_RHO_X5_HALF_RATE, 6, np.random.RandomState(SEED_OF_GENERATED_CODES)), 131072, 1.8)]


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def decoders(code):
    """-> {label: (handle, what ran)} of the decoders this build has for the code"""
    import torch

    from ldpc_decoders_amd import _lib
    from ldpc_decoders_amd._device import DecoderHandle, LqmsaHandle

    out = {}
    h = LqmsaHandle(code, None, *FIXED)
    info = h.info()
    out["LQMSA"] = (h, lambda: "LDS, %d B per frame, %d wave(s), %d frames per CU, %d layers" % (info["lds_bytes_per_frame"], info["waves_per_frame"], info["frames_per_cu"], h.layers()[0]))
    for label, alg, backend, setup in (("QMSA fp32", "QMSA", "fused", lambda d: d.set_fixed_point(*FIXED)),
                                       ("NMSA fp32", "NMSA", "fused", lambda d: d.set_correction(SCALE, 0.0)),
                                       ("LMSA fp32", "LMSA", "stream", lambda d: d.set_correction(SCALE, 0.0))):
        def make(bk):
            d = DecoderHandle(code, alg, "f32", bk)
            setup(d)
            d.simulate("biawgn", 2.0, 0, 1, 0, 0, 64, 2, torch.zeros(4, dtype=torch.int64, device="cuda"))
            return d

        try:
            d = make(backend)
        except _lib.LdpcHipError:  # no LDS-resident shape for this code: whatever auto resolves to
            d = make("auto")
        out[label] = (d, lambda d=d: d.last_stats()[0])
    return out


def rate_rows(reps):
    """-> rows (case, n, decoder, what ran, frames, word errors, mean sweeps, median ms, min ms, max ms)"""
    import torch

    rows = []
    for what, make, B, snr in cases():
        code = make()
        hs = decoders(code)
        counted, ms = {}, {k: [] for k in hs}
        for k, (h, _) in hs.items():  # the counted round is the warm-up of the operating point
            cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, cnt)
            torch.cuda.synchronize()
            counted[k] = cnt.cpu().tolist()
        scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
        for _ in range(reps):  # interleaved: clock and temperature drift hit all alike
            for k, (h, _) in hs.items():
                ms[k].append(_timed(lambda: h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, scratch)))
        for k, (h, ran) in hs.items():
            tot, wec, _, its = counted[k]
            rows.append([what, code.n, snr, k, ran(), tot, wec, its / tot, statistics.median(ms[k]), min(ms[k]), max(ms[k])])
            print(rows[-1], flush=True)
        del hs
    return rows


def wave_rows(reps):
    """-> rows (case, waves, frames per CU, median ms, min ms, max ms)"""
    import torch

    from ldpc_decoders_amd._device import LqmsaHandle

    rows = []
    for what, make, B, snr in cases():
        code = make()
        scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
        os.environ.pop("LDPC_LQMSA_NW", None)
        picked = LqmsaHandle(code).info()["waves_per_frame"]
        for nw in (1, 2, 4, 8):
            os.environ["LDPC_LQMSA_NW"] = str(nw)
            h = LqmsaHandle(code, None, *FIXED)
            h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, scratch)
            torch.cuda.synchronize()
            ms = [_timed(lambda: h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, scratch)) for _ in range(reps)]
            rows.append([what, nw, nw == picked, h.info()["frames_per_cu"], B, statistics.median(ms), min(ms), max(ms)])
            print(rows[-1], flush=True)
        os.environ.pop("LDPC_LQMSA_NW", None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_lqmsa.md"))
    a = ap.parse_args()
    import torch

    rows = rate_rows(a.reps)
    out = ["# Layered fixed-point min-sum in the LDS (LQMSA, ldpc_lqmsa_*)", "",
           "Written by `python tools/lqmsa_rate.py --reps %d` on %s (%d CUs); HIP-event times of whole simulate launches (channel kernel + decode + count; "
           "the LDS-resident kernels of `ldpc_simulate` draw their noise in the decode kernel), median of %d (min-max), after a counted warm-up launch; "
           "the decoders of a point are interleaved and see the same Philox frames."
           % (a.reps, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps), "",
           "## 1. With early exit over BI-AWGN, cap %d sweeps, all-zero word, one seed per point" % CAP, "",
           "| code | n | dB | decoder | kernels | frames | word errors | mean sweeps | ms (min-max) | frames/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for what, n, snr, k, ran, tot, wec, its, med, lo, hi in rows:
        out.append("| %s | %d | %.1f | %s | %s | %d | %d | %.2f | %.3f (%.3f-%.3f) | %.3e |" % (what, n, snr, k, ran, tot, wec, its, med, lo, hi, tot / (med * 1e-3)))
    by = {(r[0], r[3]): r for r in rows}
    out += ["", "| code | LQMSA sweeps / QMSA sweeps | LQMSA rate / QMSA rate | LQMSA rate / NMSA rate | LQMSA rate / LMSA rate |", "|---|---|---|---|---|"]
    for what in dict.fromkeys(r[0] for r in rows):
        q = by[(what, "LQMSA")]
        out.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (what, q[7] / by[(what, "QMSA fp32")][7], by[(what, "QMSA fp32")][8] / q[8], by[(what, "NMSA fp32")][8] / q[8],
                                                          by[(what, "LMSA fp32")][8] / q[8]))
    out += ["", "## 2. LQMSA under every wave count (LDPC_LQMSA_NW), the same launches", "",
            "| code | waves per frame | the rule's pick | frames per CU | frames | ms (min-max) | frames/s |", "|---|---|---|---|---|---|---|"]
    for what, nw, picked, fpc, B, med, lo, hi in wave_rows(a.reps):
        out.append("| %s | %d | %s | %d | %d | %.3f (%.3f-%.3f) | %.3e |" % (what, nw, "yes" if picked else "", fpc, B, med, lo, hi, B / (med * 1e-3)))
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

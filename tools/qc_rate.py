"""What the shift-addressed decoder of quasi-cyclic codes (QCMSA, ldpc_qc_*) reaches on one GPU beside the generic lane-per-check kernel
(LQMSA) at the same layering; writes profiles/r15_qcmsa.md.

    python tools/qc_rate.py [--reps R] [--out FILE]

1. With early exit, cap 50, device noise, the same Philox frames for every decoder of a point: frames/s, mean executed sweeps and word
   errors of QCMSA, LQMSA with layers = check // Z (the same schedule, so the counters are asserted identical), fused fp32 QMSA and
   streaming LMSA 0.8125, interleaved in one process (median of R timed simulate launches, HIP events, after a counted warm-up launch).
2. QCMSA under every wave count (LDPC_QC_NW = 1, 2, 4, 8, a fresh handle each): what the rule of ldpc_qc.hpp qc_waves picks against the
   alternatives.
The codes are generated here with fixed seeds (ldpc_decoders_amd/qc.py rand_qc_ldpc, girth >= 6).  The 12 x 24 mask is a random one of
row weight 7 and column weight >= 2, not the base matrix of any standard."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP, FIXED, SCALE, B = 50, (6, 2, 0.8125, 0), 0.8125, 65536


def random_mask(mb, nb, row_weight, rng):
    import numpy as np

    while True:
        mask = np.zeros((mb, nb), dtype=bool)
        for i in range(mb):
            mask[i, rng.choice(nb, row_weight, replace=False)] = True
        if mask.sum(axis=0).min() >= 2:
            return mask


def cases():
    import numpy as np

    from ldpc_decoders_amd import qc

    dense = np.ones((3, 6), dtype=bool)
    return [("dense 3 x 6, Z = 200", lambda: qc.rand_qc_ldpc(dense, 200, np.random.RandomState(1501)), 2.0),
            ("dense 3 x 6, Z = 192", lambda: qc.rand_qc_ldpc(dense, 192, np.random.RandomState(1502)), 2.0),
            ("6 x 12, dv = 3, Z = 100", lambda: qc.rand_qc_ldpc(qc.regular_mask(6, 12, 3), 100, np.random.RandomState(1503)), 2.0),
            ("12 x 24 random mask, Z = 81", lambda: qc.rand_qc_ldpc(random_mask(12, 24, 7, np.random.RandomState(1504)), 81, np.random.RandomState(1505)), 2.0)]


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
    import numpy as np
    import torch

    from ldpc_decoders_amd import _lib
    from ldpc_decoders_amd._device import DecoderHandle, LqmsaHandle, QcHandle

    Z = code.qc[1]
    out = {}
    q = QcHandle(code, Z, None, *FIXED)
    qi = q.info()
    out["QCMSA"] = (q, lambda: "LDS, %d B per frame, %d wave(s), %d frames per CU, %d block rows" % (qi["lds_bytes_per_frame"], qi["waves_per_frame"], qi["frames_per_cu"], code.m // Z))
    h = LqmsaHandle(code, None, *FIXED)
    h.set_layers(np.arange(code.m) // Z)
    hi = h.info()
    out["LQMSA"] = (h, lambda: "LDS, %d B per frame, %d wave(s), %d frames per CU, %d layers" % (hi["lds_bytes_per_frame"], hi["waves_per_frame"], hi["frames_per_cu"], h.layers()[0]))
    for label, alg, backend, setup in (("QMSA fp32", "QMSA", "fused", lambda d: d.set_fixed_point(*FIXED)),
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
    """-> rows (case, n, dB, decoder, what ran, frames, word errors, mean sweeps, median ms, min ms, max ms)"""
    import torch

    rows = []
    for what, make, snr in cases():
        code = make()
        hs = decoders(code)
        counted, ms = {}, {k: [] for k in hs}
        for k, (h, _) in hs.items():  # the counted round is the warm-up of the operating point
            cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, cnt)
            torch.cuda.synchronize()
            counted[k] = cnt.cpu().tolist()
        assert counted["QCMSA"] == counted["LQMSA"], (what, counted["QCMSA"], counted["LQMSA"])  # one schedule, one integer rule
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
    """-> rows (case, waves, the rule's pick, frames per CU, frames, median ms, min ms, max ms)"""
    import torch

    from ldpc_decoders_amd._device import QcHandle

    rows = []
    for what, make, snr in cases():
        code = make()
        Z = code.qc[1]
        scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
        os.environ.pop("LDPC_QC_NW", None)
        picked = QcHandle(code, Z).info()["waves_per_frame"]
        for nw in (1, 2, 4, 8):
            os.environ["LDPC_QC_NW"] = str(nw)
            h = QcHandle(code, Z, None, *FIXED)
            h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, scratch)
            torch.cuda.synchronize()
            ms = [_timed(lambda: h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, scratch)) for _ in range(reps)]
            rows.append([what, nw, nw == picked, h.info()["frames_per_cu"], B, statistics.median(ms), min(ms), max(ms)])
            print(rows[-1], flush=True)
        os.environ.pop("LDPC_QC_NW", None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_qcmsa.md"))
    a = ap.parse_args()
    import torch

    rows = rate_rows(a.reps)
    out = ["# Quasi-cyclic codes: shift-addressed layered fixed-point min-sum (QCMSA, ldpc_qc_*)", "",
           "Written by `python tools/qc_rate.py --reps %d` on %s (%d CUs); HIP-event times of whole simulate launches (channel kernel + decode + count; "
           "the LDS-resident kernels of `ldpc_simulate` draw their noise in the decode kernel), median of %d (min-max), after a counted warm-up launch; "
           "the decoders of a point are interleaved and see the same Philox frames.  The codes are generated by the tool with fixed seeds; the "
           "12 x 24 mask is a random one (row weight 7), not a standard's table.  `LQMSA` runs with layers = check // Z, the schedule of `QCMSA`: "
           "the tool asserts that the two return identical counters."
           % (a.reps, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps), "",
           "## 1. With early exit over BI-AWGN, cap %d sweeps, all-zero word, one seed per point" % CAP, "",
           "| code | n | dB | decoder | kernels | frames | word errors | mean sweeps | ms (min-max) | frames/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for what, n, snr, k, ran, tot, wec, its, med, lo, hi in rows:
        out.append("| %s | %d | %.1f | %s | %s | %d | %d | %.2f | %.3f (%.3f-%.3f) | %.3e |" % (what, n, snr, k, ran, tot, wec, its, med, lo, hi, tot / (med * 1e-3)))
    by = {(r[0], r[3]): r for r in rows}
    out += ["", "| code | QCMSA rate / LQMSA rate | QCMSA rate / QMSA rate | QCMSA rate / LMSA rate | QCMSA sweeps / QMSA sweeps |", "|---|---|---|---|---|"]
    for what in dict.fromkeys(r[0] for r in rows):
        q = by[(what, "QCMSA")]
        out.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (what, by[(what, "LQMSA")][8] / q[8], by[(what, "QMSA fp32")][8] / q[8], by[(what, "LMSA fp32")][8] / q[8],
                                                          q[7] / by[(what, "QMSA fp32")][7]))
    out += ["", "## 2. QCMSA under every wave count (LDPC_QC_NW), the same launches", "",
            "| code | waves per frame | the rule's pick | frames per CU | frames | ms (min-max) | frames/s |", "|---|---|---|---|---|---|---|"]
    for what, nw, picked, fpc, nfr, med, lo, hi in wave_rows(a.reps):
        out.append("| %s | %d | %s | %d | %d | %.3f (%.3f-%.3f) | %.3e |" % (what, nw, "yes" if picked else "", fpc, nfr, med, lo, hi, nfr / (med * 1e-3)))
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""What corrected min-sum (LDPC_ALG_NMSA) costs and what it buys, on one GPU; writes profiles/r09_nmsa.md.

    python tools/nmsa_rate.py [--reps R] [--out FILE] [--skip-config5]

1. Cost of the correction at equal work: MSA against NMSA(0.8125, 0) with LDPC_FLAG_NO_EARLY_EXIT through ldpc_simulate -- config 2
   (1200_3_6_rand_ldpc_1, 65 536 frames, 50 sweeps) in fp64 and fp32, config 4 (irregular n = 10 000, 131 072 frames, 50 sweeps) in
   fp32, config 5 ((3,6)-regular n = 64 800, 32 768 frames, 10 sweeps, streaming kernels) in fp32.  Both algorithms interleaved in one
   process, median of R timed launches each (HIP events).
2. Word / bit error rate, mean sweeps and frames per second WITH early exit at 1.5 / 2.0 / 2.5 dB on config 2 for MSA, NMSA(0.875),
   NMSA(0.8125), NMSA(0.75), NMSA(1, 0.5), fp32 and fp64.
3. Registers, spills and scratch bytes of every corrected Monte-Carlo kernel beside its min-sum sibling (tools/kernel_resources.py:
   code-object metadata, no GPU needed)."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED_OF_GENERATED_CODES = 20261002  # bench.py load_code: the same ensemble members as its configs 4 and 5


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def equal_work(reps, skip5):
    import numpy as np
    import torch

    from ldpc_decoders_amd import _lib, codes
    from ldpc_decoders_amd._device import DecoderHandle

    rows = []
    cases = [("config 2", lambda: codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, "1200_3_6_rand_ldpc_1.txt")), "f64", 65536, 50, 2.0),
             ("config 2", lambda: codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, "1200_3_6_rand_ldpc_1.txt")), "f32", 65536, 50, 2.0),
             ("config 4", lambda: codes.rand_irregular_ldpc(10000, codes.LAMBDA_RHO_X5_HALF_RATE, 6, np.random.RandomState(SEED_OF_GENERATED_CODES)),
              "f32", 131072, 50, 1.2)]
    if not skip5:
        cases.append(("config 5", lambda: codes.rand_reg_ldpc(64800, 3, 6, np.random.RandomState(SEED_OF_GENERATED_CODES)), "f32", 32768, 10, 2.0))
    for what, make, prec, B, sweeps, snr in cases:
        code = make()
        hs = {"MSA": DecoderHandle(code, "MSA", prec), "NMSA": DecoderHandle(code, "NMSA", prec)}
        hs["NMSA"].set_correction(0.8125, 0.0)
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        ms = {k: [] for k in hs}
        for k, h in hs.items():  # warm-up: plan, workspace, first launch
            h.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, cnt, flags=_lib.FLAG_NO_EARLY_EXIT)
        torch.cuda.synchronize()
        for _ in range(reps):  # interleaved: clock and temperature drift hit both alike
            for k, h in hs.items():
                ms[k].append(_timed(lambda: h.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, cnt, flags=_lib.FLAG_NO_EARLY_EXIT)))
        med = {k: statistics.median(v) for k, v in ms.items()}
        kern = hs["NMSA"].kernel_name(True) or "streaming: k_cn<float, 3, ...> + k_vn<float, 0, ...>"
        rows.append((what, code.n, prec, B, sweeps, hs["NMSA"].last_stats()[0], kern, med["MSA"], med["NMSA"], med["MSA"] / med["NMSA"],
                     min(ms["MSA"]), max(ms["MSA"]), min(ms["NMSA"]), max(ms["NMSA"])))
        print(rows[-1], flush=True)
        del hs
    return rows


def with_early_exit(reps):
    import torch

    from ldpc_decoders_amd import codes
    from ldpc_decoders_amd._device import DecoderHandle

    code = codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, "1200_3_6_rand_ldpc_1.txt"))
    B, rows = 65536, []
    rules = [("MSA", None), ("NMSA(0.875)", (0.875, 0.0)), ("NMSA(0.8125)", (0.8125, 0.0)), ("NMSA(0.75)", (0.75, 0.0)), ("NMSA(1, 0.5)", (1.0, 0.5))]
    for prec in ("f32", "f64"):
        hs = {}
        for name, corr in rules:
            hs[name] = DecoderHandle(code, "MSA" if corr is None else "NMSA", prec)
            if corr is not None:
                hs[name].set_correction(*corr)
        for snr in (1.5, 2.0, 2.5):
            for name, h in hs.items():
                cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
                h.simulate("biawgn", snr, 0, 2024, 0, 0, B, 50, cnt)  # the counted round (also the warm-up of this operating point)
                torch.cuda.synchronize()
                tot, wec, bec, its = cnt.cpu().tolist()
                scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
                ms = statistics.median(_timed(lambda: h.simulate("biawgn", snr, 0, 2024, 0, 0, B, 50, scratch)) for _ in range(reps))
                rows.append((prec, snr, name, tot, wec, wec / tot, bec / (tot * code.n), its / tot, ms, B / (ms * 1e-3)))
                print(rows[-1], flush=True)
    return rows


def resources():
    import kernel_resources

    ks = {k.split("(")[0]: v for k, v in kernel_resources.kernels_of().items()}
    rows = []
    for name in sorted(ks):
        m = re.match(r"(k_fused_bp|k_fused_f64)<3, (.*true.*)>$", name)
        if m:
            sib = "%s<0, %s>" % m.groups()
            a, b = ks[name], ks[sib]
            rows.append((name, a["vgpr"], a["spill"], a["scratch"], b["vgpr"], b["spill"], b["scratch"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_nmsa.md"))
    ap.add_argument("--skip-config5", action="store_true")
    a = ap.parse_args()
    import torch

    out = ["# Corrected min-sum (LDPC_ALG_NMSA): cost and worth", "",
           "Written by `tools/nmsa_rate.py` on %s; HIP-event times of `ldpc_simulate` launches, median of %d." % (torch.cuda.get_device_name(0), a.reps), "",
           "## 1. Cost of the correction at equal work (no early exit)", "",
           "`MSA` against `NMSA(0.8125, 0)`, interleaved in one process; ratio = MSA time / NMSA time (1.00 = free, the yardstick is 0.85).", "",
           "| workload | n | arithmetic | frames | sweeps | backend | corrected kernel | MSA ms (min-max) | NMSA ms (min-max) | NMSA rate / MSA rate |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for w, n, prec, B, sw, bk, kern, m0, m1, ratio, a0, a1, b0, b1 in equal_work(a.reps, a.skip_config5):
        out.append("| %s | %d | %s | %d | %d | %s | `%s` | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.3f |" % (w, n, prec, B, sw, bk, kern, m0, a0, a1, m1, b0, b1, ratio))
    out += ["", "## 2. With early exit: config 2, 65 536 frames of one seed per rule, 50 sweeps", "",
            "| arithmetic | dB | rule | frames | word errors | WER | BER | mean sweeps | ms | frames/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for prec, snr, name, tot, wec, wer, ber, its, ms, fps in with_early_exit(a.reps):
        out.append("| %s | %.1f | %s | %d | %d | %.3e | %.3e | %.2f | %.3f | %.3e |" % (prec, snr, name, tot, wec, wer, ber, its, ms, fps))
    out += ["", "## 3. Registers of the corrected Monte-Carlo kernels beside their min-sum siblings", "",
            "| kernel | VGPRs | spilled | scratch B | sibling VGPRs | sibling spilled | sibling scratch B |", "|---|---|---|---|---|---|---|"]
    for r in resources():
        out.append("| `%s` | %d | %d | %d | %d | %d | %d |" % r)
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""What the bits of fixed-point min-sum (LDPC_ALG_QMSA) are worth and what the rule costs, on one GPU; writes profiles/r10_qmsa.md.

    python tools/qmsa_bits.py [--frames N] [--reps R] [--out FILE]

1. Word length against error rate: 1200_3_6_rand_ldpc_1, BI-AWGN at 2.0 dB, all-zero word, 50 sweeps, N >= 2^20 device-noise frames per
   row (one seed for all rows) -- float64 plain min-sum, float64 NMSA(0.8125), then (bits, frac_bits, scale, offset) from 8 bits down to 3
   on the fp32 LDS kernel; the peak |marginal| in levels comes from the soft outputs of 4 096 host-noise frames without early exit.
2. Cost of the rule at equal work: QMSA(6, 2, 0.8125, 0) against NMSA(0.8125, 0), LDPC_FLAG_NO_EARLY_EXIT, 50 sweeps, 65 536 frames of the
   same code through ldpc_simulate -- fp32 LDS kernel, fp64 LDS kernel, streaming fp32 and streaming fp16.  Both interleaved in one
   process, median of R timed launches each (HIP events).  The yardstick is the NMSA sibling in the same run.
3. Registers, spills and scratch bytes of every fixed-point Monte-Carlo kernel beside its NMSA sibling (tools/kernel_resources.py:
   code-object metadata, no GPU needed)."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CODE = "1200_3_6_rand_ldpc_1"
# (label, algorithm, precision, parameters)
ROWS = [("float64 plain min-sum", "MSA", "f64", None), ("float64 NMSA", "NMSA", "f64", (0.8125, 0.0)),
        ("8 4 0.8125 0", "QMSA", "f32", (8, 4, 0.8125, 0)), ("6 2 0.8125 0", "QMSA", "f32", (6, 2, 0.8125, 0)),
        ("5 1 1 1", "QMSA", "f32", (5, 1, 1.0, 1)), ("5 1 0.8125 0", "QMSA", "f32", (5, 1, 0.8125, 0)),
        ("4 1 0.75 0", "QMSA", "f32", (4, 1, 0.75, 0)), ("4 0 1 1", "QMSA", "f32", (4, 0, 1.0, 1)), ("4 0 0.75 0", "QMSA", "f32", (4, 0, 0.75, 0)),
        ("3 0 1 0", "QMSA", "f32", (3, 0, 1.0, 0)), ("3 0 0.75 0", "QMSA", "f32", (3, 0, 0.75, 0))]


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _make(code, alg, prec, params, backend="auto"):
    from ldpc_decoders_amd._device import DecoderHandle

    h = DecoderHandle(code, alg, prec, backend)
    if alg == "NMSA":
        h.set_correction(*params)
    if alg == "QMSA":
        h.set_fixed_point(*params)
    return h


def bits_table(code, frames):
    import numpy as np
    import torch

    from ldpc_decoders_amd import _lib

    rng = np.random.RandomState(11)
    var = 10 ** -0.2
    pri = torch.from_numpy((-2 * (-1 + rng.normal(0, np.sqrt(var), (4096, code.n))) / var).astype(np.float32)).cuda()
    rows, chunk = [], 1 << 18
    for label, alg, prec, params in ROWS:
        h = _make(code, alg, prec, params)
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        for f0 in range(0, frames, chunk):
            h.simulate("biawgn", 2.0, 0, 2026, 0, f0, min(chunk, frames - f0), 50, cnt)
        torch.cuda.synchronize()
        tot, wec, bec, its = cnt.cpu().tolist()
        peak = ""
        if alg == "QMSA":
            _, _, soft = h.decode_soft_device(pri, None, 50, flags=_lib.FLAG_NO_EARLY_EXIT)
            peak = "%d" % int(soft.abs().max().item())
        rows.append((label, prec, h.last_stats()[0], tot, wec, wec / tot, bec, bec / (tot * code.n), its / tot, peak))
        print(rows[-1], flush=True)
    return rows


def equal_work(code, reps):
    import torch

    from ldpc_decoders_amd import _lib

    rows, B, sweeps = [], 65536, 50
    for what, prec, backend in (("fp32 LDS kernel", "f32", "auto"), ("fp64 LDS kernel", "f64", "auto"), ("streaming fp32", "f32", "stream"),
                                ("streaming fp16", "f16", "stream")):
        hs = {"NMSA": _make(code, "NMSA", prec, (0.8125, 0.0), backend), "QMSA": _make(code, "QMSA", prec, (6, 2, 0.8125, 0), backend)}
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        ms = {k: [] for k in hs}
        for h in hs.values():  # warm-up: plan, workspace, first launch
            h.simulate("biawgn", 2.0, 0, 1, 0, 0, B, sweeps, cnt, flags=_lib.FLAG_NO_EARLY_EXIT)
        torch.cuda.synchronize()
        for _ in range(reps):  # interleaved: clock and temperature drift hit both alike
            for k, h in hs.items():
                ms[k].append(_timed(lambda: h.simulate("biawgn", 2.0, 0, 1, 0, 0, B, sweeps, cnt, flags=_lib.FLAG_NO_EARLY_EXIT)))
        med = {k: statistics.median(v) for k, v in ms.items()}
        kern = hs["QMSA"].kernel_name(True) if hs["QMSA"].last_stats()[0] == "fused" else "k_cn%s<.., 4, ..> + the min-sum variable pass" % ("16" if prec == "f16" else "")
        rows.append((what, hs["QMSA"].last_stats()[0], kern, med["NMSA"], min(ms["NMSA"]), max(ms["NMSA"]), med["QMSA"], min(ms["QMSA"]), max(ms["QMSA"]),
                     B / (med["NMSA"] * 1e-3), B / (med["QMSA"] * 1e-3), med["NMSA"] / med["QMSA"]))
        print(rows[-1], flush=True)
        del hs
    return rows


def resources():
    import kernel_resources

    ks = {k.split("(")[0]: v for k, v in kernel_resources.kernels_of().items()}
    rows = []
    for name in sorted(ks):
        m = re.match(r"(k_fused_bp|k_fused_f64)<4, (.*true.*)>$", name)
        if m:
            a, b = ks[name], ks["%s<3, %s>" % m.groups()]
            rows.append((name, a["vgpr"], a["spill"], a["scratch"], b["vgpr"], b["spill"], b["scratch"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_qmsa.md"))
    a = ap.parse_args()
    import torch

    from ldpc_decoders_amd import codes

    code = codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, CODE + ".txt"))
    out = ["# Fixed-point min-sum (LDPC_ALG_QMSA): what the bits are worth, what the rule costs", "",
           "Written by `tools/qmsa_bits.py` on %s." % torch.cuda.get_device_name(0), "",
           "## 1. Word length against error rate", "",
           "`%s`, BI-AWGN at 2.0 dB, all-zero word, 50 sweeps, device noise, %d frames per row (the same frames in every row of one arithmetic). "
           "Peak |marginal|: levels, 4 096 frames without early exit." % (CODE, a.frames), "",
           "| bits frac scale offset | arithmetic | backend | frames | word errors | WER | bit errors | BER | mean sweeps | peak \\|marginal\\| |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in bits_table(code, a.frames):
        out.append("| %s | %s | %s | %d | %d | %.3e | %d | %.3e | %.2f | %s |" % r)
    out += ["", "## 2. Cost of the rule at equal work (no early exit)", "",
            "`NMSA(0.8125, 0)` against `QMSA(6, 2, 0.8125, 0)`, 65 536 frames, 50 sweeps, `ldpc_simulate`, interleaved in one process, median of %d "
            "HIP-event times; ratio = QMSA rate / NMSA rate (1.00 = the same)." % a.reps, "",
            "| workload | backend | fixed-point kernel | NMSA ms (min-max) | QMSA ms (min-max) | NMSA frames/s | QMSA frames/s | QMSA rate / NMSA rate |",
            "|---|---|---|---|---|---|---|---|"]
    for w, bk, kern, m0, a0, a1, m1, b0, b1, f0, f1, ratio in equal_work(code, a.reps):
        out.append("| %s | %s | `%s` | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.3e | %.3e | %.3f |" % (w, bk, kern, m0, a0, a1, m1, b0, b1, f0, f1, ratio))
    out += ["", "## 3. Registers of the fixed-point Monte-Carlo kernels beside their NMSA siblings", "",
            "| kernel | VGPRs | spilled | scratch B | sibling VGPRs | sibling spilled | sibling scratch B |", "|---|---|---|---|---|---|---|"]
    for r in resources():
        out.append("| `%s` | %d | %d | %d | %d | %d | %d |" % r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

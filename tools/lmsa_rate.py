"""What the layered schedule (LDPC_ALG_LMSA) buys on the streaming kernels, on one GPU; writes profiles/r12_lmsa.md.

    python tools/lmsa_rate.py [--reps R] [--out FILE] [--parent-lib PATH] [--skip-config5]

1. With early exit, fp32, scale 0.8125, cap 50, device noise through ldpc_simulate: frames/s, mean executed sweeps and WER of LMSA against
   NMSA on the streaming kernels of the SAME build, interleaved in one process (median of R timed launches, HIP events) -- the (3,6)
   n = 64 800 code at 2.0 dB with 32 768 frames, the n = 10 000 irregular ensemble at 1.2 dB, 1200_3_6_rand_ldpc_1 at 2.0 dB -- and, with
   --parent-lib, against NMSA on the library of the parent commit (tools/build_commit_variant.sh), in a child process of its own.
2. Achieved bytes/s of the layer passes and of the whole layered sweep against the model s (4E + n) bytes per frame-sweep: ten sweeps
   without early exit under ldpc_decoder_profile ([0] layer passes, [1] decision pass)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_OF_GENERATED_CODES = 20261002  # bench.py load_code: the same ensemble members as its configs 4 and 5
SCALE, CAP = 0.8125, 50


def cases(skip5):
    import numpy as np

    from ldpc_decoders_amd import codes

    out = [("1200_3_6_rand_ldpc_1", lambda: codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, "1200_3_6_rand_ldpc_1.txt")), 65536, 2.0),
           ("irregular n = 10 000", lambda: codes.rand_irregular_ldpc(10000, codes.LAMBDA_RHO_X5_HALF_RATE, 6, np.random.RandomState(SEED_OF_GENERATED_CODES)), 131072, 1.2)]
    if not skip5:
        out.append(("(3,6) n = 64 800", lambda: codes.rand_reg_ldpc(64800, 3, 6, np.random.RandomState(SEED_OF_GENERATED_CODES)), 32768, 2.0))
    return out


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def early_exit_rows(algs, reps, skip5):
    """-> rows (case, n, alg, layers, frames, word errors, mean sweeps, median ms, min ms, max ms)"""
    import torch

    from ldpc_decoders_amd._device import DecoderHandle

    rows = []
    for what, make, B, snr in cases(skip5):
        code = make()
        hs = {}
        for alg in algs:
            hs[alg] = DecoderHandle(code, alg, "f32", "stream")
            hs[alg].set_correction(SCALE, 0.0)
        counted, ms = {}, {alg: [] for alg in algs}
        for alg, h in hs.items():  # the counted round is the warm-up of the operating point
            cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, cnt)
            torch.cuda.synchronize()
            counted[alg] = cnt.cpu().tolist()
        scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
        for _ in range(reps):  # interleaved: clock and temperature drift hit both alike
            for alg, h in hs.items():
                ms[alg].append(_timed(lambda: h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, scratch)))
        for alg, h in hs.items():
            tot, wec, _, its = counted[alg]
            layers = h.layers()[0] if alg == "LMSA" else 0
            rows.append([what, code.n, alg, layers, tot, wec, its / tot, statistics.median(ms[alg]), min(ms[alg]), max(ms[alg])])
            print(rows[-1], flush=True)
        del hs
    return rows


def bytes_rows(skip5):
    """-> rows (case, layers, frames, sweeps, layer-pass ms, decision ms, model bytes of the layer passes, of the sweep)"""
    import torch

    from ldpc_decoders_amd import _lib
    from ldpc_decoders_amd._device import DecoderHandle

    rows, sweeps = [], 10
    for what, make, B, snr in cases(skip5):
        code = make()
        h = DecoderHandle(code, "LMSA", "f32", "stream")
        h.set_correction(SCALE, 0.0)
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        h.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, cnt, flags=_lib.FLAG_NO_EARLY_EXIT)  # warm-up
        torch.cuda.synchronize()
        h.set_profiling(True)
        h.read_profile(reset=True)
        h.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, cnt, flags=_lib.FLAG_NO_EARLY_EXIT)
        torch.cuda.synchronize()
        prof = h.read_profile(reset=True)
        h.set_profiling(False)
        s, E, n = 4, code.E, code.n
        layer_bytes = s * B * (4 * E * sweeps - E)  # the first sweep reads no old messages
        rows.append([what, h.layers()[0], B, sweeps, prof["stream_check_pass"][0], prof["stream_variable_pass"][0], layer_bytes, layer_bytes + s * B * n * sweeps])
        print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_lmsa.md"))
    ap.add_argument("--parent-lib", default=None, help="libldpc_hip.so of the parent commit (tools/build_commit_variant.sh)")
    ap.add_argument("--skip-config5", action="store_true")
    ap.add_argument("--child", action="store_true", help="internal: NMSA rows of the library LDPC_LIB_PATH names, as JSON")
    a = ap.parse_args()
    if a.child:
        print("ROWS " + json.dumps(early_exit_rows(["NMSA"], a.reps, a.skip_config5)))
        return
    import torch

    parent = []
    if a.parent_lib:
        # (a library outside the package does not find the shipped layout plans by itself: tools/ab_sim.sh)
        env = dict(os.environ, LDPC_LIB_PATH=os.path.abspath(a.parent_lib), LDPC_LIB_ALLOW_OLDER_ABI="1",
                   LDPC_FUSED_PLAN_DIR=os.path.join(ROOT, "ldpc_decoders_amd", "plans"))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--skip-config5"] if a.skip_config5 else [])
        res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=900)
        parent = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("ROWS ")][-1][5:])
    rows = early_exit_rows(["NMSA", "LMSA"], a.reps, a.skip_config5)
    out = ["# Layered min-sum (LDPC_ALG_LMSA) on the streaming kernels", "",
           "Written by `tools/lmsa_rate.py` on %s; HIP-event times of `ldpc_simulate` launches, median of %d (min-max)." % (torch.cuda.get_device_name(0), a.reps), "",
           "## 1. With early exit: fp32, scale %s, cap %d, streaming kernels, one seed per point" % (SCALE, CAP), "",
           "| code | n | decoder | layers | frames | word errors | WER | mean sweeps | ms (min-max) | frames/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for tag, rs in (("", rows), (" (parent commit's library)", parent)):
        for what, n, alg, layers, tot, wec, its, med, lo, hi in rs:
            out.append("| %s | %d | %s%s | %s | %d | %d | %.3e | %.2f | %.2f (%.2f-%.2f) | %.3e |" % (what, n, alg, tag, layers or "-", tot, wec, wec / tot, its, med, lo, hi,
                                                                                                  tot / (med * 1e-3)))
    by = {(r[0], r[2]): r for r in rows}
    out += ["", "| code | LMSA sweeps / NMSA sweeps | LMSA rate / NMSA rate (same build) |", "|---|---|---|"]
    for what in dict.fromkeys(r[0] for r in rows):
        l, f = by[(what, "LMSA")], by[(what, "NMSA")]
        out.append("| %s | %.3f | %.3f |" % (what, l[6] / f[6], f[7] / l[7]))
    out += ["", "## 2. Bytes per second against the model s (4E + n) per frame-sweep", "",
            "Ten sweeps without early exit under `ldpc_decoder_profile`; model bytes over event time (the first sweep reads no old messages).", "",
            "| code | layers | frames | layer passes ms | decision pass ms | layer passes TB/s | whole sweep TB/s |", "|---|---|---|---|---|---|---|"]
    for what, layers, B, sweeps, t0, t1, b0, b1 in bytes_rows(a.skip_config5):
        out.append("| %s | %d | %d | %.2f | %.2f | %.2f | %.2f |" % (what, layers, B, t0, t1, b0 / (t0 * 1e-3) / 1e12, b1 / ((t0 + t1) * 1e-3) / 1e12))
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

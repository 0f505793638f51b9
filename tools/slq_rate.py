"""What the streaming layered fixed-point decoder (SLQMSA, ldpc_slq_*) reaches on one GPU; writes profiles/r16_slqmsa.md.

    python tools/slq_rate.py [--reps R] [--out FILE] [--parent-lib PATH] [--skip-config5] [--bench-steps K]

1. With early exit, cap 50, the same Philox frames for every decoder (seed 2024, stream 0, frame 0), one process, launches interleaved, the
   median of R timed launches after a counted warm-up: frames/s, mean sweeps and word errors of SLQMSA (6, 2, 0.8125, 0) and of fp32 LMSA
   (scale 0.8125) on the streaming kernels, both on the greedy layering -- 1200_3_6_rand_ldpc_1 at 2.0 dB, the irregular n = 10 000
   ensemble at 1.8 dB, (3,6) n = 64 800 at 2.0 dB with 32 768 frames -- and LQMSA (the LDS kernel) where it takes the code.  The counters
   of SLQMSA and LQMSA are asserted identical: one contract.
2. Model bytes per second: ten sweeps without early exit under ldpc_slq_profile; the layer passes move 6 E bytes per frame-sweep (the
   first sweep reads no messages: 5 E), the decision pass 2 n; beside fp32 LMSA under ldpc_decoder_profile with its model 4 (4 E + n).
3. With --parent-lib (tools/build_commit_variant.sh parent HEAD~1): streaming LMSA on the three rows, and with --bench-steps the headline
   line of bench.py, on this build and on the parent commit's library, each in a child process of its own."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_OF_GENERATED_CODES = 20261002  # bench.py load_code: the same ensemble members as its configs 4 and 5
FIXED, SCALE, CAP = (6, 2, 0.8125, 0), 0.8125, 50


def cases(skip5):
    import numpy as np

    from ldpc_decoders_amd import codes

    out = [("1200_3_6_rand_ldpc_1", lambda: codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, "1200_3_6_rand_ldpc_1.txt")), 65536, 2.0, True),
           ("irregular n = 10 000", lambda: codes.rand_irregular_ldpc(10000, codes.LAMBDA_RHO_X5_HALF_RATE, 6, np.random.RandomState(SEED_OF_GENERATED_CODES)), 131072, 1.8, True)]
    if not skip5:
        out.append(("(3,6) n = 64 800", lambda: codes.rand_reg_ldpc(64800, 3, 6, np.random.RandomState(SEED_OF_GENERATED_CODES)), 32768, 2.0, False))
    return out


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _lmsa(code):
    from ldpc_decoders_amd._device import DecoderHandle

    h = DecoderHandle(code, "LMSA", "f32", "stream")
    h.set_correction(SCALE, 0.0)
    return h


def rate_rows(names, reps, skip5):
    """-> rows (case, n, decoder, layers, frames, word errors, mean sweeps, median ms, min ms, max ms)"""
    import torch

    from ldpc_decoders_amd._device import LqmsaHandle, SlqHandle

    rows = []
    for what, make, B, snr, lds in cases(skip5):
        code = make()
        hs = {}
        if "SLQMSA" in names:
            hs["SLQMSA"] = SlqHandle(code, None, *FIXED)
        if "LMSA" in names:
            hs["LMSA fp32"] = _lmsa(code)
        if "LQMSA" in names and lds:
            hs["LQMSA"] = LqmsaHandle(code, None, *FIXED)
        counted, ms = {}, {k: [] for k in hs}
        for k, h in hs.items():  # the counted round is the warm-up of the operating point
            cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, cnt)
            torch.cuda.synchronize()
            counted[k] = cnt.cpu().tolist()
        if "SLQMSA" in counted and "LQMSA" in counted:
            assert counted["SLQMSA"] == counted["LQMSA"], (what, counted["SLQMSA"], counted["LQMSA"])  # one layering, one integer rule
        scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
        for _ in range(reps):  # interleaved: clock and temperature drift hit all alike
            for k, h in hs.items():
                ms[k].append(_timed(lambda: h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, scratch)))
        for k, h in hs.items():
            tot, wec, _, its = counted[k]
            rows.append([what, code.n, k, h.layers()[0], tot, wec, its / tot, statistics.median(ms[k]), min(ms[k]), max(ms[k])])
            print(rows[-1], flush=True)
        del hs
    return rows


def bytes_rows(skip5):
    """-> rows (case, decoder, layers, frames, sweeps, layer-pass ms, decision ms, model bytes of the layer passes, of the sweeps)"""
    import torch

    from ldpc_decoders_amd import _lib
    from ldpc_decoders_amd._device import SlqHandle

    rows, sweeps = [], 10
    for what, make, B, snr, _ in cases(skip5):
        code = make()
        E, n = code.E, code.n
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        for name in ("SLQMSA", "LMSA fp32"):
            h = SlqHandle(code, None, *FIXED) if name == "SLQMSA" else _lmsa(code)
            run = lambda: h.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, cnt, flags=_lib.FLAG_NO_EARLY_EXIT)  # noqa: E731
            run()  # warm-up
            torch.cuda.synchronize()
            if name == "SLQMSA":
                h.profile(True)
                h.read_profile(reset=True)
                run()
                prof = h.read_profile(reset=True)
                t0, t1 = prof["layer_passes"][0], prof["decision_pass"][0]
                layer_bytes, node_bytes = B * (6 * E * sweeps - E), 2 * B * n * sweeps  # the first sweep reads no old messages
            else:
                h.set_profiling(True)
                h.read_profile(reset=True)
                run()
                torch.cuda.synchronize()
                prof = h.read_profile(reset=True)
                t0, t1 = prof["stream_check_pass"][0], prof["stream_variable_pass"][0]
                layer_bytes, node_bytes = 4 * B * (4 * E * sweeps - E), 4 * B * n * sweeps
            rows.append([what, name, h.layers()[0], B, sweeps, t0, t1, layer_bytes, layer_bytes + node_bytes])
            print(rows[-1], flush=True)
            del h
    return rows


def _child(lib, args, timeout=1500):
    """stdout of a child process of this build's Python on the library `lib` (None: this build's)"""
    env = dict(os.environ)
    if lib:  # (a library outside the package does not find the shipped layout plans by itself: tools/ab_sim.sh)
        env.update(LDPC_LIB_PATH=os.path.abspath(lib), LDPC_LIB_ALLOW_OLDER_ABI="1", LDPC_FUSED_PLAN_DIR=os.path.join(ROOT, "ldpc_decoders_amd", "plans"))
    return subprocess.run([sys.executable] + args, env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=timeout, cwd=ROOT).stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_slqmsa.md"))
    ap.add_argument("--parent-lib", default=None, help="libldpc_hip.so of the parent commit (tools/build_commit_variant.sh)")
    ap.add_argument("--bench-steps", type=int, default=0, help="with --parent-lib: also bench.py --gpus 1 --steps K --warmup 3 --no-profile on both libraries")
    ap.add_argument("--skip-config5", action="store_true")
    ap.add_argument("--child", action="store_true", help="internal: the streaming LMSA rows of the library LDPC_LIB_PATH names, as JSON")
    a = ap.parse_args()
    if a.child:
        print("ROWS " + json.dumps(rate_rows(["LMSA"], a.reps, a.skip_config5)))
        return
    import torch

    rows = rate_rows(["SLQMSA", "LMSA", "LQMSA"], a.reps, a.skip_config5)
    brows = bytes_rows(a.skip_config5)
    out = ["# Streaming layered fixed-point min-sum (SLQMSA, ldpc_slq_*)", "",
           "Written by `python tools/slq_rate.py --reps %d` on %s; HIP-event times of whole simulate launches (channel kernel + decode + count), "
           "median of %d (min-max) after a counted warm-up; seed 2024, cap %d, early exit; SLQMSA and LQMSA (%d, %d, %s, %d), LMSA fp32 scale %s on the "
           "streaming kernels, all on the greedy layering." % ((a.reps, torch.cuda.get_device_name(0), a.reps, CAP) + FIXED + (SCALE,)), "",
           "## 1. With early exit", "",
           "| code | n | decoder | layers | frames | word errors | mean sweeps | ms (min-max) | frames/s |", "|---|---|---|---|---|---|---|---|---|"]
    for what, n, name, layers, tot, wec, its, med, lo, hi in rows:
        out.append("| %s | %d | %s | %d | %d | %d | %.2f | %.2f (%.2f-%.2f) | %.3e |" % (what, n, name, layers, tot, wec, its, med, lo, hi, tot / (med * 1e-3)))
    by = {(r[0], r[2]): r for r in rows}
    out += ["", "Sweep counts and word errors of SLQMSA and LQMSA were asserted identical.  The byte model (20 n against 52 n per frame-sweep at E = 3 n) says 2.6 "
            "for the ratio to LMSA; the measured ratios of the frame rates:", "",
            "| code | SLQMSA rate / LMSA rate | SLQMSA sweeps / LMSA sweeps | SLQMSA rate / LQMSA rate |", "|---|---|---|---|"]
    for what in dict.fromkeys(r[0] for r in rows):
        s, l, q = by[(what, "SLQMSA")], by[(what, "LMSA fp32")], by.get((what, "LQMSA"))
        out.append("| %s | %.3f | %.3f | %s |" % (what, l[7] / s[7], s[6] / l[6], "%.3f" % (q[7] / s[7]) if q else "- (LQMSA refuses the code)"))
    out += ["", "## 2. Model bytes per second", "",
            "Ten sweeps without early exit under the profile slots; model bytes over event time.  SLQMSA: 6 E per frame-sweep in the layer passes (the first "
            "sweep reads no messages), 2 n in the decision pass; LMSA fp32: 16 E and 4 n.", "",
            "| code | decoder | layers | frames | layer passes ms | decision pass ms | layer passes TB/s | with the decision pass TB/s |", "|---|---|---|---|---|---|---|---|"]
    for what, name, layers, B, sweeps, t0, t1, b0, b1 in brows:
        out.append("| %s | %s | %d | %d | %.2f | %.2f | %.2f | %.2f |" % (what, name, layers, B, t0, t1, b0 / (t0 * 1e-3) / 1e12, b1 / ((t0 + t1) * 1e-3) / 1e12))
    if a.parent_lib:
        flags = ["--reps", str(a.reps)] + (["--skip-config5"] if a.skip_config5 else [])
        out += ["", "## 3. Nothing existing moved: this build against the parent commit's library", "",
                "Streaming LMSA, the launches of section 1, each library in a child process of its own.", "",
                "| code | library | word errors | mean sweeps | ms (min-max) |", "|---|---|---|---|---|"]
        for tag, lib in (("this build", None), ("parent commit", a.parent_lib)):
            res = _child(lib, [os.path.abspath(__file__), "--child"] + flags)
            for what, n, name, layers, tot, wec, its, med, lo, hi in json.loads([ln for ln in res.splitlines() if ln.startswith("ROWS ")][-1][5:]):
                out.append("| %s | %s | %d | %.2f | %.2f (%.2f-%.2f) |" % (what, tag, wec, its, med, lo, hi))
        if a.bench_steps > 0:
            out += ["", "`python bench.py --gpus 1 --steps %d --warmup 3 --no-profile`:" % a.bench_steps, ""]
            for tag, lib in (("this build", None), ("parent commit", a.parent_lib)):
                res = _child(lib, [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "3", "--no-profile"])
                line = json.loads([ln for ln in res.splitlines() if ln.startswith("{")][-1])
                keep = {k: line[k] for k in ("value", "unit", "ms_per_step", "ms_per_step_min", "ms_per_step_max", "mean_sweeps", "word_errors") if k in line}
                out.append("- %s: `%s`" % (tag, json.dumps(keep)))
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""The host loop of the streaming decoders (csrc/ldpc_tiles.hpp) against another build of the library, on one GPU.

    python tools/stream_loop_ab.py --parent-lib LIB      parent / this build / parent, one child process each (LDPC_LIB_PATH): wall time of one
                                                         decode, stream synchronised, median (min-max) in ms per driver and batch, as a table
    python tools/stream_loop_ab.py --one DRIVER          one decode of case 1 of tests/test_gpu_sweep_loop.py, for `rocprofv3 --kernel-trace -- ...`
    python tools/stream_loop_ab.py --names DIR OUT       the library's kernels of the trace under DIR, in launch order with their grids -> OUT

Drivers and batches are those of tests/test_gpu_sweep_loop.py (fp32 MSA and LMSA on the streaming backend, fp16 storage MSA, SLQMSA;
1200_3_6_rand_ldpc_1).  A row is `within` if this build's median lies in the span of the parent's two medians widened by their difference."""
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIS = os.path.join(ROOT, "ldpc_decoders_amd", "csrc", "libldpc_hip.so")


def _tests():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import test_gpu_sweep_loop as T

    return T


def one(driver):
    os.environ["LDPC_STREAM_REPACK_FILL"] = "0.95"
    T = _tests()
    x, it, sweeps, repacks = T._decode(T._handle(driver), T._mixed(), 200)
    print(driver, "sweeps", sweeps, "repacks", repacks, "iters sum", int(it.sum()), "ones", int(x.sum()))


def names(trace_dir, out):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], r.get("Grid_Size") or "%sx%sx%s" % (r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"])))
    rows.sort()
    with open(out, "w") as fp:
        for _, n, g in rows:
            if "ldpc::" in n:
                fp.write("%s grid=%s\n" % (n.replace("ldpc::(anonymous namespace)::", "").replace("ldpc::", "").replace("void ", "").split("(")[0], g))
    print(out, sum(1 for _ in open(out)), "kernels")


def child():
    T = _tests()
    import numpy as np
    import torch

    import bp_oracle as O

    g = T._code()[0]
    rng = np.random.RandomState(3)

    def awgn(B, snr):
        return torch.from_numpy(O.biawgn_priors(-1 + rng.normal(0, np.sqrt(O.biawgn_noise_var(snr)), (B, g.n)), snr).astype(np.float32)).cuda()

    cases = [("one tile (64 frames), 2.0 dB, cap 50", awgn(64, 2.0), 50, 200),
             ("case 1 of test_gpu_sweep_loop (771 frames, cap 200)", torch.from_numpy(T._pool()[T._mixed()]).cuda(), 200, 60),
             ("16384 frames, 2.0 dB, cap 50", awgn(16384, 2.0), 50, 30)]
    out = {}
    for drv in T.DRIVERS:
        h = T._handle(drv)
        for name, pri, cap, reps in cases:
            for _ in range(3):
                h.decode_device(pri, None, cap)
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t = time.perf_counter()
                h.decode_device(pri, None, cap)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t) * 1e3)
            ts.sort()
            out["%s | %s" % (drv, name)] = (ts[len(ts) // 2], ts[0], ts[-1])
    print("JSON" + json.dumps(out))


def main(parent):
    runs = []
    for label, lib in (("parent 1", parent), ("this build", THIS), ("parent 2", parent)):
        env = dict(os.environ, LDPC_LIB_PATH=os.path.abspath(lib), LDPC_FUSED_PLAN_DIR=os.path.join(ROOT, "ldpc_decoders_amd", "plans"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            print(label, "failed", r.returncode, r.stderr[-2000:])
            sys.exit(1)
        runs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("JSON")][0][4:]))
    print("| driver, batch | parent, first run: median ms (min-max) | this build | parent, second run | parents' medians, widened by their difference | verdict |")
    print("|---|---|---|---|---|---|")
    for k in runs[0]:
        a, b, c = runs[0][k], runs[1][k], runs[2][k]
        lo, hi = min(a[0], c[0]), max(a[0], c[0])
        d = hi - lo
        verdict = "within" if lo - d <= b[0] <= hi + d else ("faster" if b[0] < lo - d else "SLOWER")
        print("| %s | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.3f-%.3f | %s |" % ((k,) + tuple(a) + tuple(b) + tuple(c) + (lo - d, hi + d, verdict)))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    elif "--one" in sys.argv:
        one(sys.argv[sys.argv.index("--one") + 1])
    elif "--names" in sys.argv:
        i = sys.argv.index("--names")
        names(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main(sys.argv[sys.argv.index("--parent-lib") + 1])

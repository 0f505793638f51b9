"""Whole `simulate` calls of the handle families on two builds of the library, for changes to their host side; writes a markdown table.

    python tools/sim_pass_ab.py --parent-lib LIB [--reps R] [--out FILE]

One child process per run (`LDPC_LIB_PATH`): the parent's library, this build, the parent's library again, and the parent's library once
more in the place of this build (how often the criterion calls a build slower than itself).  A row is one operating point of the family's
rate tool (tools/galb_rate.py, bec_ml_rate.py, osd_gain.py, lqmsa_rate.py, qc_rate.py, slq_rate.py) at 65 536 frames, and the smallest shipped
code beside it, where a launch takes about a millisecond and the host side weighs most: HIP-event time of the whole call, median of R
(min-max) after a counted warm-up call.  `--child` prints the rows of the library LDPC_LIB_PATH names as one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, FIXED, SCALE = 65536, (6, 2, 0.8125, 0), 0.8125


def _rows():
    """-> [(label, make handle, channel, param, max_iter)]"""
    import numpy as np

    from ldpc_decoders_amd import _device as D
    from ldpc_decoders_amd import codes, qc

    def shipped(name):
        return codes.load_parity_mtx(os.path.join(codes.PACKAGE_CODES_DIR, name + ".txt"))

    def osd(name):
        bp = D.DecoderHandle(shipped(name), "NMSA", "f32")
        bp.set_correction(SCALE, 0.0)
        return D.OsdHandle(bp, 0, 64)

    dense = np.ones((3, 6), dtype=bool)
    small, big = "512_3_6_rand_ldpc_1", "1200_3_6_rand_ldpc_1"
    return [("GALB, LDS kernel, %s, bsc 0.03" % small, lambda: D.HardHandle(shipped(small), "fused"), "bsc", 0.03, 20),
            ("GALB, LDS kernel, %s, bsc 0.03" % big, lambda: D.HardHandle(shipped(big), "fused"), "bsc", 0.03, 20),
            ("GALB, streaming kernels, %s, bsc 0.03" % big, lambda: D.HardHandle(shipped(big), "stream"), "bsc", 0.03, 20),
            ("GALB, LDS kernel, %s, biawgn 6 dB" % big, lambda: D.HardHandle(shipped(big), "fused"), "biawgn", 6.0, 20),
            ("BEC-ML, %s, eps 0.40" % small, lambda: D.BecMlHandle(shipped(small)), "bec", 0.40, 0),
            ("BEC-ML, %s, eps 0.45" % big, lambda: D.BecMlHandle(shipped(big)), "bec", 0.45, 0),
            ("OSD-0 behind NMSA, %s, 2.0 dB" % small, lambda: osd(small), "biawgn", 2.0, 20),
            ("OSD-0 behind NMSA, %s, 1.5 dB" % big, lambda: osd(big), "biawgn", 1.5, 50),
            ("LQMSA, %s, 2.5 dB" % small, lambda: D.LqmsaHandle(shipped(small), None, *FIXED), "biawgn", 2.5, 50),
            ("LQMSA, %s, 2.0 dB" % big, lambda: D.LqmsaHandle(shipped(big), None, *FIXED), "biawgn", 2.0, 50),
            ("LQMSA, %s, bsc 0.05" % big, lambda: D.LqmsaHandle(shipped(big), None, *FIXED), "bsc", 0.05, 50),
            ("QCMSA, dense 3 x 6, Z = 32, 3.5 dB", lambda: D.QcHandle(qc.rand_qc_ldpc(dense, 32, np.random.RandomState(1500)), 32, None, *FIXED), "biawgn", 3.5, 50),
            ("QCMSA, dense 3 x 6, Z = 200, 2.0 dB", lambda: D.QcHandle(qc.rand_qc_ldpc(dense, 200, np.random.RandomState(1501)), 200, None, *FIXED), "biawgn", 2.0, 50),
            ("SLQMSA, %s, 2.5 dB" % small, lambda: D.SlqHandle(shipped(small), None, *FIXED), "biawgn", 2.5, 50),
            ("SLQMSA, %s, 2.0 dB" % big, lambda: D.SlqHandle(shipped(big), None, *FIXED), "biawgn", 2.0, 50)]


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def child(reps):
    import torch

    out = []
    for label, make, channel, param, max_iter in _rows():
        h = make()
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        h.simulate(channel, param, 0, 2024, 0, 0, B, max_iter, cnt)  # the counted call is the warm-up of the operating point
        torch.cuda.synchronize()
        scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
        ms = [_timed(lambda: h.simulate(channel, param, 0, 2024, 0, 0, B, max_iter, scratch)) for _ in range(reps)]
        out.append(dict(row=label, counters=cnt.cpu().tolist(), median=statistics.median(ms), min=min(ms), max=max(ms)))
        del h
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libldpc_hip.so of the parent commit (tools/build_commit_variant.sh)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_sim_pass_shared.md"))
    ap.add_argument("--child", action="store_true", help="internal: the rows of the library LDPC_LIB_PATH names, as JSON")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    runs = []
    for lib in (a.parent_lib, None, a.parent_lib, a.parent_lib):
        env = dict(os.environ, LDPC_FUSED_PLAN_DIR=os.path.join(ROOT, "ldpc_decoders_amd", "plans"))  # a library elsewhere finds the shipped plans
        env.pop("LDPC_LIB_PATH", None)
        if lib:
            env["LDPC_LIB_PATH"] = os.path.abspath(lib)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=900)
        if res.returncode != 0:
            sys.exit("the child on %s failed (%d):\n%s" % (lib or "this build", res.returncode, res.stderr[-3000:]))
        runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
        print("ran", lib or "this build", flush=True)
    first, this, second, control = runs

    def cell(r):
        return "%.3f (%.3f-%.3f)" % (r["median"], r["min"], r["max"])

    out = ["| row | parent, first run: median ms (min-max) | parent, second run | parent's spread, both runs | this build | verdict | the parent in this build's place | verdict |",
           "|---|---|---|---|---|---|---|---|"]
    for p1, t, p2, c in zip(first, this, second, control):
        assert p1["counters"] == t["counters"] == p2["counters"] == c["counters"], (p1["row"], p1["counters"], t["counters"])
        lo, hi = min(p1["min"], p2["min"]), max(p1["max"], p2["max"])
        verdict = lambda r: "within" if lo <= r["median"] <= hi else ("faster" if r["median"] < lo else "slower")  # noqa: E731
        out.append("| %s | %s | %s | %.3f-%.3f | %s | %s | %s | %s |" % (p1["row"], cell(p1), cell(p2), lo, hi, cell(t), verdict(t), cell(c), verdict(c)))
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("\n".join(out))
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""What several frames per wave (ldpc_qcpack_set, k_qc_pack) give the quasi-cyclic decoder (QCMSA, ldpc_qc_*) at lifting sizes up to 32 on
one GPU; writes profiles/r17_qc_pack.md.

    python tools/qc_pack_rate.py [--reps R] [--out FILE]

Per code and operating point: P = 1 (k_qc, one frame per workgroup) and every P from 2 to floor(64 / Z) (k_qc_pack) on fresh handles,
interleaved in one process; 65 536 frames, cap 50, early exit, device noise, the same Philox frames for every P; whole simulate launches
timed with HIP events, median, minimum and maximum of R (>= 3) timed launches after a counted warm-up launch.  The counters of the warm-up
launches are asserted identical for every P: packing changes no result.  The last column says whether the rule's pick (ldpc_qc.hpp
qc_pack) is the fastest P by the median or overlaps the fastest's min-max spread.
The codes are generated here with fixed seeds (ldpc_decoders_amd/qc.py rand_qc_ldpc, girth >= 6); the masks are not a standard's."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP, FIXED, B, SNRS = 50, (6, 2, 0.8125, 0), 65536, (2.0, 3.5)


def cases():
    import numpy as np

    from ldpc_decoders_amd import qc

    out = [("12 x 24, dv = 3, Z = %d" % z, lambda z=z: qc.rand_qc_ldpc(qc.regular_mask(12, 24, 3), z, np.random.RandomState(1700 + z))) for z in (8, 16, 27, 32)]
    return out + [("dense 3 x 6, Z = 32", lambda: qc.rand_qc_ldpc(np.ones((3, 6), dtype=bool), 32, np.random.RandomState(1799)))]


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rows_of(reps):
    """-> rows (case, n, Z, dB, P, the rule's pick, stride, frames per CU, word errors, mean sweeps, median ms, min ms, max ms)"""
    import torch

    from ldpc_decoders_amd import qc
    from ldpc_decoders_amd._device import QcHandle

    rows = []
    for what, make in cases():
        code = make()
        Z = code.qc[1]
        hs = {P: QcHandle(code, Z, None, *FIXED, pack=P) for P in range(1, 64 // Z + 1)}
        pick = hs[1].pack()[1]
        need = hs[1].info()["lds_bytes_per_frame"]
        assert pick == qc.qc_pack(Z, need) and all(h.pack() == (P, pick) for P, h in hs.items())
        for snr in SNRS:
            counted, ms = {}, {P: [] for P in hs}
            for P, h in hs.items():  # the counted round is the warm-up of the operating point
                cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
                h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, cnt)
                torch.cuda.synchronize()
                counted[P] = cnt.cpu().tolist()
            assert all(c == counted[1] for c in counted.values()), (what, snr, counted)  # the same frames, the same integers
            scratch = torch.zeros(4, dtype=torch.int64, device="cuda")
            for _ in range(reps):  # interleaved: clock and temperature drift hit all alike
                for P, h in hs.items():
                    ms[P].append(_timed(lambda: h.simulate("biawgn", snr, 0, 2024, 0, 0, B, CAP, scratch)))
            tot, wec, _, its = counted[1]
            for P, h in hs.items():
                rows.append([what, code.n, Z, snr, P, pick, qc.qc_pack_stride(need, Z), h.info()["frames_per_cu"], wec, its / tot, statistics.median(ms[P]), min(ms[P]), max(ms[P])])
                print(rows[-1], flush=True)
        del hs
    return rows


def verdict(group, pick):
    """The rule's pick against the fastest P of one code and operating point: rows (P, median, min, max)"""
    best = min(group, key=lambda r: r[1])
    mine = next(r for r in group if r[0] == pick)
    if best[0] == pick:
        return "fastest"
    if mine[2] <= best[3]:
        return "within the spread of P = %d" % best[0]
    return "no: P = %d is %.1f %% faster" % (best[0], 100.0 * (mine[1] / best[1] - 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_qc_pack.md"))
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("--reps: at least 3 timed launches")
    import torch

    rows = rows_of(a.reps)
    out = ["# QCMSA: several frames per wave for lifting sizes up to 32 (ldpc_qcpack_set, k_qc_pack)", "",
           "Written by `python tools/qc_pack_rate.py --reps %d` on %s (%d CUs); HIP-event times of whole simulate launches (channel kernel + decode + "
           "count), median of %d (min-max) after a counted warm-up launch; %d frames over BI-AWGN, cap %d sweeps, early exit, all-zero word; the "
           "handles of a point -- P = 1 is `k_qc` with one frame per workgroup, P >= 2 is `k_qc_pack` -- are fresh, interleaved and see the same "
           "Philox frames; the tool asserts that their counters are identical.  The codes are generated by the tool with fixed seeds."
           % (a.reps, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.reps, B, CAP), "",
           "The stride from one frame slot's LDS image to the next is `qc_pack_stride`: the frame's bytes rounded up to 16 and then padded until it "
           "is congruent to 2 Z rounded up to 16 modulo 128.  Why: a slot's Z lanes read Z neighbouring int16 marginals of one block column, at "
           "most that many bytes; LDS conflicts are counted within a 32-lane group over 32 banks of 4 bytes, and the slots that share a group "
           "then start 2 Z bytes (rounded up) of banks apart instead of wherever the frame size happens to put them.  This was chosen from the "
           "bank arithmetic; the unpadded stride was not measured against it, and no hardware counter was collected.", "",
           "The slots a wave serves together draw their frames with one atomic on the dispenser.  A first form of `k_qc_pack` drew one frame per "
           "atomic, as `k_qc` does, and this tool measured it at 0.79 (Z = 8), 0.93 (Z = 16), 0.97 (Z = 27) and 0.93 (dense Z = 32) of P = 1 at "
           "3.5 dB, where a frame takes about two sweeps and the launch is bound by handing frames out (DESIGN section 22); P = 1 still pays one "
           "atomic per frame.", "",
           "| code | n | dB | word errors | mean sweeps | P | the rule's pick | stride B | frames per CU | ms (min-max) | frames/s | against P = 1 |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    groups = {}
    for r in rows:
        groups.setdefault((r[0], r[3]), []).append(r)
    for (what, snr), grp in groups.items():
        one = next(r for r in grp if r[4] == 1)
        for what, n, Z, snr, P, pick, stride, fpc, wec, its, med, lo, hi in grp:
            out.append("| %s | %d | %.1f | %d | %.2f | %d | %s | %d | %d | %.3f (%.3f-%.3f) | %.3e | %.2f |"
                       % (what, n, snr, wec, its, P, "yes" if P == pick else "", stride, fpc, med, lo, hi, B / (med * 1e-3), one[10] / med))
    out += ["", "## The rule's pick against the fastest P", "", "| code | dB | the rule's pick | fastest P by the median | pick / P = 1 | verdict |", "|---|---|---|---|---|---|"]
    for (what, snr), grp in groups.items():
        pick = grp[0][5]
        best = min(grp, key=lambda r: r[10])
        one = next(r for r in grp if r[4] == 1)
        mine = next(r for r in grp if r[4] == pick)
        out.append("| %s | %.1f | %d | %d | %.2f | %s |" % (what, snr, pick, best[4], one[10] / mine[10], verdict([(r[4], r[10], r[11], r[12]) for r in grp], pick)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

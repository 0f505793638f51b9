"""What ordered-statistics post-processing (csrc/ldpc_osd.hip) gains and costs: word error rates of NMSA, OSD-0 and OSD-1 (depth 64) on the
same frames, the rate of each whole Monte-Carlo step, and the solver's time per listed frame -- timed with HIP events.

    python tools/osd_gain.py [--reps R] [--frames B] [--code NAME ..] [--snr S ..]            one JSON line per (code, SNR)
    LDPC_LIB_PATH=<library of the parent commit> LDPC_LIB_ALLOW_OLDER_ABI=1 python tools/osd_gain.py --bp-only
                                                                                              the parent's ldpc_simulate at the same points
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/osd_gain.py --reps 1              BP / list / solve / count split

Codes 512_3_6_rand_ldpc_1 (20 sweeps; 1.5, 2.0, 2.5 dB) and 1200_3_6_rand_ldpc_1 (50 sweeps; 1.0, 1.5, 2.0 dB), NMSA 0.8125 in fp32, all-zero
word, Philox seed 1, 65 536 frames per round.  Every step (ldpc_simulate of NMSA; ldpc_osd_simulate with order 0 and with order 1, depth 64)
is warmed up once and timed `reps` times (best of).  The solver alone: ldpc_osd_solve (k_osd_list + k_osd_solve) on the soft outputs of
one round, divided by the frames it lists."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = {"512_3_6_rand_ldpc_1": (20, [1.5, 2.0, 2.5]), "1200_3_6_rand_ldpc_1": (50, [1.0, 1.5, 2.0])}


def _time(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def run(name, snr, sweeps, B, reps, bp_only):
    import torch

    from ldpc_decoders_amd import codes
    from ldpc_decoders_amd._device import DecoderHandle

    code = codes.get_code(name)
    bp = DecoderHandle(code, "NMSA", "f32")
    bp.set_correction(0.8125, 0.0)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = dict(code=name, snr=snr, sweeps=sweeps, frames=B)
    t = _time(lambda: bp.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, cnt), reps)
    c = torch.zeros(4, dtype=torch.int64, device="cuda")
    bp.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, c)
    out.update(bp_step_ms=round(t, 3), bp_frames_per_s=round(B / (t * 1e-3)), bp_wer=int(c[1]) / B)
    if bp_only:
        return out
    from ldpc_decoders_amd._device import OsdHandle

    osd = OsdHandle(bp)
    for tag, order, depth in (("osd0", 0, 0), ("osd1", 1, 64)):
        osd.order, osd.depth = order, depth
        t = _time(lambda: osd.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, cnt), reps)
        c = torch.zeros(4, dtype=torch.int64, device="cuda")
        osd.simulate("biawgn", snr, 0, 1, 0, 0, B, sweeps, c)
        out.update({tag + "_step_ms": round(t, 3), tag + "_frames_per_s": round(B / (t * 1e-3)), tag + "_wer": int(c[1]) / B})
    # the solver alone, on the soft outputs of the same round
    pri, _ = bp.channel_device("biawgn", snr, 0, 1, 0, 0, B)
    _, _, post = bp.decode_soft_device(pri, None, sweeps)
    for tag, order, depth in (("osd0", 0, 0), ("osd1", 1, 64)):
        t = _time(lambda: osd.solve(post, pri, order, depth, want_cost=False), reps)
        _, pick, _ = osd.solve(post, pri, order, depth, want_cost=False)
        listed = int((pick >= 0).sum())
        out.update({"listed": listed, tag + "_solve_ms": round(t, 3), tag + "_solve_us_per_listed": round(1e3 * t / max(listed, 1), 3)})
    t = _time(lambda: bp.decode_soft_device(pri, None, sweeps), reps)
    out.update(bp_soft_decode_ms=round(t, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", action="append")
    ap.add_argument("--snr", type=float, action="append")
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bp-only", action="store_true", help="only ldpc_simulate of NMSA (what a library of the parent commit can run)")
    a = ap.parse_args()
    for name in a.code or list(POINTS):
        sweeps, snrs = POINTS.get(name, (50, [1.5]))
        for snr in a.snr or snrs:
            print(json.dumps(run(name, snr, sweeps, a.frames, a.reps, a.bp_only)), flush=True)


if __name__ == "__main__":
    main()

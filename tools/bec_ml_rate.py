"""Rate of the ML erasure decoder (csrc/ldpc_bec_ml.hip) against the erasure decoder (BP) in the same process, timed with HIP events.

    python tools/bec_ml_rate.py [--reps R] [--frames B] [--eps E ..] [--code NAME ..]     one JSON line per (code, eps)
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bec_ml_rate.py --reps 1      peel / compaction / elimination / count split

Codes 1200_3_6_rand_ldpc_1 and 1200_rho_x5_rand_ldpc_1, eps in {0.40, 0.425, 0.45, 0.475, 0.50}, 65 536 frames per round.  Both Monte-Carlo
steps (ldpc_bec_ml_simulate: channel -> peel -> solve -> count; ldpc_simulate with max_iter 0: channel -> peel -> count) are warmed up once
and then timed `reps` times (best of).  Also reports how many frames keep erasures after peeling (the frames the solver lists), the mean
residual size and nullity of those frames, and how many needed the 160 KiB slab."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def run(name, eps, B, reps):
    import torch

    from ldpc_decoders_amd import codes
    from ldpc_decoders_amd._device import BecMlHandle, DecoderHandle

    code = codes.get_code(name)
    bp, ml = DecoderHandle(code, "BEC", "f32"), BecMlHandle(code)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    t_ml = _time(lambda: ml.simulate("bec", eps, 0, 1, 0, 0, B, 0, cnt), reps)
    t_bp = _time(lambda: bp.simulate("bec", eps, 0, 1, 0, 0, B, 0, cnt), reps)
    # what the solver saw on these frames
    _, y = bp.channel_device("bec", eps, 0, 1, 0, 0, B)
    bits, era, _ = bp.decode_device_bits(None, y, 0)
    _, nul = ml.solve_bits(bits, era, 1, 0, 0)
    sh = torch.arange(32, device=era.device, dtype=torch.int32)
    e = ((era[:, :, None] >> sh) & 1).reshape(B, -1)[:, :code.n].int()
    nc = e.sum(dim=1)
    touch = torch.zeros((B, code.m), dtype=torch.int32, device=era.device)
    touch.index_add_(1, torch.from_numpy(code.edge_chk.astype("int64")).cuda(), e[:, torch.from_numpy(code.edge_var.astype("int64")).cuda()])
    rows = (touch > 0).sum(dim=1)
    W, S, RP = (code.n + 31) // 32, (nc + 32) // 32, (rows + 63) // 64 * 64
    big = ((3 * W + 3 * S + S * RP) * 4 > 32 * 1024) & (nc > 0)  # frames the 32 KiB slab sets aside for the 160 KiB pass
    listed = nc > 0
    nl, nres = int(listed.sum()), int(nc.sum())
    c_ml, c_bp = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    ml.simulate("bec", eps, 0, 1, 0, 0, B, 0, c_ml)
    bp.simulate("bec", eps, 0, 1, 0, 0, B, 0, c_bp)
    return dict(code=name, eps=eps, frames=B, ml_step_ms=round(t_ml, 3), bp_step_ms=round(t_bp, 3),
                ml_frames_per_s=round(B / (t_ml * 1e-3)), bp_frames_per_s=round(B / (t_bp * 1e-3)),
                listed_frames=nl, mean_residual_listed=round(nres / max(nl, 1), 1),
                mean_nullity_listed=round(float(nul[listed].float().mean()) if nl else 0.0, 3),
                large_slab_frames=int(big.sum()), mean_rows_listed=round(float(rows[listed].float().mean()) if nl else 0.0, 1),
                ml_wer=int(c_ml[1]) / B, bp_wer=int(c_bp[1]) / B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", action="append")
    ap.add_argument("--eps", type=float, action="append")
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for name in a.code or ["1200_3_6_rand_ldpc_1", "1200_rho_x5_rand_ldpc_1"]:
        for eps in a.eps or [0.40, 0.425, 0.45, 0.475, 0.50]:
            print(json.dumps(run(name, eps, a.frames, a.reps)), flush=True)


if __name__ == "__main__":
    main()

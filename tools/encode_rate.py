"""Rate of the GF(2) encoder (csrc/ldpc_encode.hip) and of the random-codeword Monte-Carlo step, timed with HIP events.

    python tools/encode_rate.py [--config 2|4] [--reps R]            one JSON line per config
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/encode_rate.py --config 4 --reps 2    per-kernel times

Config 2: 1200_3_6_ldpc, 65 536 frames, fp64 min-sum over the BSC (p = 0.035, 50 sweeps).  Config 4: the irregular n = 10 000 ensemble
(rate 1/2, rho = x^5), 131 072 frames, fp32 min-sum over BI-AWGN at 1.5 dB, 50 sweeps.  Reports the encode kernel alone
(ldpc_encode_random), the whole random-codeword step (encode -> ldpc_channel_sent -> decode -> count) and the all-zero fused step
(ldpc_simulate) on the same frames."""
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


def run(config, reps):
    import numpy as np
    import torch

    from ldpc_decoders_amd import codes
    from ldpc_decoders_amd._device import DecoderHandle

    if config == 2:
        code, B, channel, param, prec = codes.get_code("1200_3_6_ldpc"), 65536, "bsc", 0.035, "f64"
    else:
        code = codes.rand_irregular_ldpc(10000, codes.LAMBDA_RHO_X5_HALF_RATE, 6, np.random.RandomState(1))
        B, channel, param, prec = 131072, "biawgn", 1.5, "f32"
    enc = code.encoder()
    h = DecoderHandle(code, "MSA", prec, "auto")
    out = torch.empty((B, code.n), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    t_enc = _time(lambda: enc.random_words(1, 0, 0, B, out=out), reps)
    t_rand = _time(lambda: h.simulate(channel, param, -1, 1, 0, 0, B, 50, cnt), reps)
    t_zero = _time(lambda: h.simulate(channel, param, 0, 1, 0, 0, B, 50, cnt), reps)
    macs = float(B) * enc.k * enc.rank
    return dict(config=config, n=code.n, k=enc.k, r=enc.rank, frames=B, channel=channel, param=param, precision=prec,
                encode_ms=round(t_enc, 4), encode_tops=round(2 * macs / (t_enc * 1e-3) / 1e12, 1),
                random_step_ms=round(t_rand, 3), zero_step_ms=round(t_zero, 3),
                random_frames_per_s=round(B / (t_rand * 1e-3)), zero_frames_per_s=round(B / (t_zero * 1e-3)),
                encode_share_of_random_step=round(t_enc / t_rand, 4), backend=h.last_stats()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=[2, 4], action="append")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for c in a.config or [2, 4]:
        print(json.dumps(run(c, a.reps)), flush=True)


if __name__ == "__main__":
    main()

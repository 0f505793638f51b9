// The layered fixed-point min-sum, stated once for its three decoders: LQMSA (ldpc_lqmsa.hip, the frame in the LDS, index tables), QCMSA
// (ldpc_qc.hip, the frame in the LDS, shift-addressed) and SLQMSA (ldpc_slq.hip, the state in HBM tiles).  They differ in where a check's
// values come from and where its messages go; what is done with them is here.
//
// The contract is the ldpc_lqmsa_* block of include/ldpc_hip.h, steps 1-4.  Everything after the quantiser is an
// integer, in levels, with V = 2^(bits-1) - 1:
//     1. level_v = quantise_prior(prior_v, 2^frac_bits, V) (ldpc_cn.hpp: LDPC_ALG_QMSA's quantiser); marg = level, every c2v = 0.
//     2. Before each sweep: stop at the cap, or when H x_hat = 0 -- from sweep 1 on with x_hat = (marg < 0), at sweep 0 only where the
//        received word y0 is given, which then is x_hat.  iters = sweeps executed.
//     3. One check, its edges j in H's row-major order: v_j = marg[var_j] - c2v_j; a_j = min(|v_j|, V); the new c2v_j has the sign of the
//        other edges' parity and the magnitude fx_mag(min over i != j of a_i); marg[var_j] = v_j + c2v_j (v_j itself is not clipped).
//        The checks of a layer share no variable.  |marg| <= V (1 + dv), so int16 holds it for every dv <= 255.
//     4. Outputs: the decisions as bytes and / or packed words, iters, optionally the int16 marginals of the last sweep; a frame that
//        never swept keeps the received word and reports 0 as its soft output.
// Device side: the rule (fx_mag, FxCheck, the two row forms of the LDS decoders), the frame prologue and epilogue of the LDS decoders and
// their frame hand-out and syndrome vote.  Host side: what the three handles hold and refuse in common.  Every message names the entry
// point it is raised for, so each routine takes that name.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "ldpc_cn.hpp"
#include "ldpc_common.hpp"
#include "ldpc_sim.hpp"

namespace ldpc {

// ---- device side: the rule ---------------------------------------------------------------------------------------------------------------
// |c2v| a minimum m <= V sends
__device__ __forceinline__ int fx_mag(int m, int scale64, int offset) {
    const int t = ((scale64 * m) >> 6) - offset;
    return t > 0 ? t : 0;
}

// One check in three steps: take(j, v_j, V) for every edge, finish(scale64, offset), then out(j, v_j) is the new message c2v_j.
struct FxCheck {
    int min1, min2, arg, f1, f2;
    uint32_t par;
    __device__ __forceinline__ explicit FxCheck(int V) : min1(V), min2(V), arg(-1), par(0) {}  // |v| enters as min(|v|, V), so V is the neutral element
    __device__ __forceinline__ void take(int j, int v, int V) {
        const int a = min(abs(v), V);
        par ^= (uint32_t)(v < 0);
        if (a < min1) {
            min2 = min1;
            min1 = a;
            arg = j;
        } else if (a < min2) {
            min2 = a;
        }
    }
    __device__ __forceinline__ void finish(int scale64, int offset) {
        f1 = fx_mag(min1, scale64, offset);
        f2 = fx_mag(min2, scale64, offset);
    }
    __device__ __forceinline__ int out(int j, int v) const {
        const int mag = j == arg ? f2 : f1;
        return (par ^ (uint32_t)(v < 0)) ? -mag : mag;
    }
};

// One check of an LDS-resident frame whose 8-byte message row `rowp` is held in registers: edges j < deg of at most D (deg == D where the
// degree is static), var(j) the variable of edge j.
template <int D, class Var>
__device__ __forceinline__ void fx_check_row8(int16_t* __restrict__ marg, uint2* __restrict__ rowp, int deg, Var var, int scale64, int offset, int V) {
    FxCheck k(V);
    const uint2 row = *rowp;
    const uint32_t rw[2] = {row.x, row.y};
    int v[D];
    decltype(var(0)) vi[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (j < deg) {
            vi[j] = var(j);
            v[j] = (int)marg[vi[j]] - (int)(int8_t)(rw[j >> 2] >> (8 * (j & 3)));
            k.take(j, v[j], V);
        }
    }
    k.finish(scale64, offset);
    uint32_t out[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (j < deg) {
            const int c = k.out(j, v[j]);
            marg[vi[j]] = (int16_t)(v[j] + c);
            out[j >> 2] |= (uint32_t)(uint8_t)(int8_t)c << (8 * (j & 3));
        }
    }
    *rowp = make_uint2(out[0], out[1]);
}

// The loop form, any degree: the row stays in the LDS and is read twice.
template <class Var>
__device__ __forceinline__ void fx_check_loop(int16_t* __restrict__ marg, uint8_t* __restrict__ row, int deg, Var var, int scale64, int offset, int V) {
    FxCheck k(V);
    for (int j = 0; j < deg; ++j) k.take(j, (int)marg[var(j)] - (int)(int8_t)row[j], V);
    k.finish(scale64, offset);
    for (int j = 0; j < deg; ++j) {
        const auto vi = var(j);
        const int v = (int)marg[vi] - (int)(int8_t)row[j];
        const int c = k.out(j, v);
        marg[vi] = (int16_t)(v + c);
        row[j] = (uint8_t)(int8_t)c;
    }
}

// ---- device side: a frame of the LDS decoders enters and leaves ----------------------------------------------------------------------------
// NT threads serve the frame: thread `tid`, lane `lane` of wave `w`.  Frame image: marg int16 [n], then the message rows.

// Step 1: the priors `pr` of the frame are quantised into marg, the `words` dwords of message rows at `rows` are zeroed.
template <int NT, typename T>
__device__ __forceinline__ void fx_load_frame(const T* __restrict__ pr, T step, T vmax, int16_t* marg, uint32_t* rows, int n, int words, int tid) {
    for (int v = tid; v < n; v += NT) marg[v] = (int16_t)(int)quantise_prior<T>(pr[v], step, vmax);
    for (int i = tid; i < words; i += NT) rows[i] = 0u;
}

// Step 4: frame f leaves after `it` sweeps.  it == 0: it left at the check of the received word and keeps it (cap >= 1, so y0 was given).
// The packed kernel k_qc_pack writes its frames with it (NT = 64, w = 0).  k_lqmsa and k_qc carry the same lines inline: routed through this
// function their sweeps changed speed by -2 to +1 % with the wave count (profiles/r18_layered_fx_shared.md), and this file was not to move any.
template <int NT, typename F>
__device__ __forceinline__ void fx_write_frame(const uint8_t* y0, uint8_t* xhat, int16_t* soft, uint32_t* bits, int32_t* iters, int n, const int16_t* marg,
                                               F f, int it, int tid, int lane, int w) {
    const int Wd = (n + 31) / 32;
    const uint8_t* __restrict__ yf = y0 ? y0 + (size_t)f * n : nullptr;
    if (tid == 0) iters[f] = it;
    if (xhat)
        for (int v = tid; v < n; v += NT) xhat[(size_t)f * n + v] = it == 0 ? yf[v] : (uint8_t)(marg[v] < 0);
    if (soft)
        for (int v = tid; v < n; v += NT) soft[(size_t)f * n + v] = it == 0 ? (int16_t)0 : marg[v];
    if (bits)
        for (int v0 = w * 64; v0 < n; v0 += NT) {
            const int v = v0 + lane;
            const bool bit = v < n && (it == 0 ? (yf[v] & 1u) != 0u : marg[v] < 0);
            const unsigned long long b = __ballot(bit);
            if (lane == 0) {
                uint32_t* out = bits + (size_t)f * Wd + (v0 >> 5);
                out[0] = (uint32_t)b;
                if ((v0 >> 5) + 1 < Wd) out[1] = (uint32_t)(b >> 32);
            }
        }
}

// The frame hand-out of a workgroup that owns one frame at a time.  ctl (LDS): frame index, two syndrome flags used by alternate sweeps,
// spare.  The first barrier: the frame before is written out.
__device__ __forceinline__ int64_t fx_draw_frame(uint32_t* dispenser, uint32_t* ctl, int tid) {
    __syncthreads();
    if (tid == 0) {
        ctl[0] = atomicAdd(dispenser, 1u);
        ctl[1] = 0u;
        ctl[2] = 0u;
    }
    __syncthreads();
    return ctl[0];
}

// Step 2 across the waves: `bad` (wave-uniform) says that this wave met an unsatisfied check before sweep `it`; does any wave say so?
__device__ __forceinline__ bool fx_any_unsatisfied(uint32_t* ctl, bool bad, int it, int tid, int lane) {
    if (bad && lane == 0) ctl[1 + (it & 1)] = 1u;
    __syncthreads();
    const bool any = ctl[1 + (it & 1)] != 0u;
    if (tid == 0) ctl[1 + ((it + 1) & 1)] = 0u;  // last read a sweep ago, next written a sweep (and a layer barrier) from now
    return any;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// The parameters of the rule as a handle holds them, and as a kernel takes them.
struct FixedPoint {
    int bits = 6, frac = 2, offset = 0;
    double scale = 0.8125;
    int set(const char* entry, int bits_, int frac_bits, double scale_, int offset_) {
        // (written so that a NaN scale fails; 64 * scale is exact, so the grid test is)
        if (bits_ < 2 || bits_ > 8 || frac_bits < -8 || frac_bits > 8 || !(scale_ > 0.0 && scale_ <= 1.0) ||
            64.0 * scale_ != (double)(long long)(64.0 * scale_) || offset_ < 0) {
            set_error("%s: 2 <= bits <= 8, -8 <= frac_bits <= 8, scale a multiple of 1/64 in (0, 1] and offset >= 0 are needed "
                      "(bits=%d frac_bits=%d scale=%g offset=%d)", entry, bits_, frac_bits, scale_, offset_);
            return LDPC_E_ARG;
        }
        bits = bits_;
        frac = frac_bits;
        scale = scale_;
        offset = offset_;
        return LDPC_OK;
    }
    void get(int* bits_, int* frac_bits, double* scale_, int* offset_) const {
        *bits_ = bits;
        *frac_bits = frac;
        *scale_ = scale;
        *offset_ = offset;
    }
    int32_t scale64() const { return (int32_t)(64.0 * scale); }
    int32_t clamped_offset() const { return std::min(offset, 1 << 20); }  // beyond V every message is 0 already
    int32_t vmax() const { return (1 << (bits - 1)) - 1; }
    double step() const { return std::ldexp(1.0, frac); }
};

// *_create: what the rule asks of the degrees; `rows` names what min_dc was taken over ("check", "block row"), dv_limit is the family's *_MAX_DV
inline int fx_check_degrees(const char* entry, const char* rows, int min_dc, int max_dv, int dv_limit) {
    if (min_dc < 2) {
        set_error("%s: a %s of degree %d: layered min-sum needs every check to have degree >= 2", entry, rows, min_dc);
        return LDPC_E_UNSUPPORTED;
    }
    if (max_dv > dv_limit) {
        set_error("%s: a variable of degree %d: the int16 marginals hold V (1 + dv) for dv <= %d", entry, max_dv, dv_limit);
        return LDPC_E_UNSUPPORTED;
    }
    return LDPC_OK;
}

// *_decode: the arguments every family refuses
inline int fx_check_decode(const char* entry, int dtype, uint32_t flags, int64_t B) {
    if (dtype != DT_F32 && dtype != DT_F64) {
        set_error("%s: the priors are LDPC_DTYPE_F32 or LDPC_DTYPE_F64 (got %d)", entry, dtype);
        return LDPC_E_ARG;
    }
    if (flags & ~FLAG_NO_EARLY_EXIT) {
        set_error("%s: the only flag is LDPC_FLAG_NO_EARLY_EXIT (got 0x%x)", entry, flags);
        return LDPC_E_UNSUPPORTED;
    }
    if (B > (int64_t)1 << 31) {
        set_error("%s: at most 2^31 frames per call (got %lld)", entry, (long long)B);
        return LDPC_E_ARG;
    }
    return LDPC_OK;
}

// *_simulate: the pass loop of ldpc_sim.hpp on fp32 priors, in passes of at most `cap` frames (the family's bound on the priors of one pass);
// decode(priors, y, frames, bits, iters) is the family's *_decode.
template <class Decode>
int fx_simulate(const char* entry, const Code* code, SimStage& s, int64_t cap, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id,
                uint64_t frame0, int64_t B, int32_t hist_bins, int64_t* counters, hipStream_t st, Decode&& decode) {
    const bool llr = channel == CH_BIAWGN || channel == CH_BSC;
    const bool bsc = channel == CH_BSC;  // over the BSC the received word takes the iteration-0 check, as upstream
    return sim_passes(
        SimCall{entry, code, codeword, frame0, B, hist_bins, counters, st},
        llr ? nullptr : "LDPC_CH_BIAWGN or LDPC_CH_BSC (min-sum has no magnitudes to work on over the erasure channel)", cap,
        [&](int64_t frames) -> int { return s.reserve(frames, (size_t)code->n, true, bsc); },
        [&](uint64_t first, int64_t nb, const uint32_t*& bits, const int32_t*& iters) -> int {
            uint8_t* y = bsc ? (uint8_t*)s.y.p : nullptr;
            LDPC_TRY(channel_generate(channel, DT_F32, param, codeword, seed, stream_id, first, nb, code->n, s.pri.p, y, st));
            bits = (const uint32_t*)s.bits.p;
            iters = (const int32_t*)s.iters.p;
            return decode(s.pri.p, y, nb, (uint32_t*)s.bits.p, (int32_t*)s.iters.p);
        });
}

// the LDS decoders' bound on one pass of fp32 priors: about 256 MiB
inline int64_t fx_lds_sim_cap(int32_t n) { return std::max<int64_t>((int64_t)(((size_t)256 << 20) / ((size_t)n * sizeof(float))), 1); }

// ---- host side, the LDS decoders: one workgroup of nw waves per frame ------------------------------------------------------------------------
// waves per frame: the family's rule, or what the environment variable `env_name` says (the tests reach every wave count with it)
inline int fx_waves(int rule, const char* env_name) {
    if (const char* env = std::getenv(env_name)) {
        const int v = std::atoi(env);
        if (v == 1 || v == 2 || v == 4 || v == 8) return v;
    }
    return rule;
}

// frames one CU works on at a time: what its LDS holds (`fit`), within its 32 waves
inline int fx_frames_per_cu(int64_t fit, int nw) { return (int)std::min<int64_t>(fit, 32 / nw); }

// above 64 KiB a workgroup's LDS has to be asked for, for the fp32 and the fp64 kernel
inline hipError_t fx_allow_lds(const void* k32, const void* k64, int64_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(k32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e != hipSuccess ? e : hipFuncSetAttribute(k64, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// the fields LqArgs and QcArgs have in common
template <class Args>
void fx_fill_args(Args& a, const Code* c, const FixedPoint& fx, int row_bytes, void* dispenser, const void* priors, const uint8_t* y0, int64_t B,
                  int32_t max_iter, uint32_t flags, uint8_t* xhat, uint32_t* bits, int32_t* iters, int16_t* soft) {
    a.priors = priors;
    a.y0 = y0;
    a.B = B;
    a.n = c->n;
    a.m = c->m;
    a.row_bytes = row_bytes;
    a.cap = max_iter > 0 ? max_iter : 100000;
    a.no_early = (flags & FLAG_NO_EARLY_EXIT) ? 1 : 0;
    a.scale64 = fx.scale64();
    a.offset = fx.clamped_offset();
    a.vmax = fx.vmax();
    a.step = fx.step();
    a.dispenser = (uint32_t*)dispenser;
    a.xhat = xhat;
    a.bits = bits;
    a.iters = iters;
    a.soft = soft;
}

}  // namespace ldpc

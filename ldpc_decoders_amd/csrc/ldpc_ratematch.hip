// Punctured and shortened transmission: the channel of a transmission pattern and the error tally that goes with it.
//
// A system rarely transmits the whole codeword of its mother code: it punctures bits (a codeword bit that is not sent: the decoder starts
// it from a prior of 0) and shortens bits (a filler bit known to be 0 and not sent: the decoder starts it from a large positive prior).
// kind [n], one byte per variable, says which (0 sent, 1 punctured, 2 shortened).  No decoder kernel changes; what changes is what the
// channel writes and what the tally counts.
//
//   sent        the draw of ldpc_channel_sent / ldpc_channel for the same (seed, stream, global frame, variable), bit for bit: the Philox
//               block and word of a variable are those of its index in the MOTHER code, so a pattern moves no other bit's noise
//   punctured   prior +0.0, y = 0
//   shortened   prior +short_llr (positive = bit 0, as -2y/sigma^2), y = 0; so reads every byte above 2, in the channel and in the tally
//   tally       the counters of k_count with a frame's errors taken over kind < 2: a punctured bit is a codeword bit and counts,
//               a shortened bit is known and does not
#include "ldpc_ratematch.hpp"

#include <cmath>
#include <vector>

#include "ldpc_rng.hpp"

namespace ldpc {
namespace {

// the four pattern bytes of variables 4j .. 4j+3 (VEC: one dword, n % 4 == 0; else bytes, a variable beyond n reads as punctured)
template <bool VEC>
__device__ __forceinline__ uint32_t kinds_of(const uint8_t* __restrict__ kind, int j, int n) {
    if constexpr (VEC) {
        return *reinterpret_cast<const uint32_t*>(kind + 4 * j);
    } else {
        uint32_t k4 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) k4 |= (uint32_t)(4 * j + q < n ? kind[4 * j + q] : (uint8_t)KIND_PUNCTURED) << (8 * q);
        return k4;
    }
}

// the four sent bits of variables 4j .. 4j+3 of frame f, as the bytes of a dword (sent == NULL: the all-`codeword` word)
template <bool VEC>
__device__ __forceinline__ uint32_t bits_of(const uint8_t* __restrict__ sent, int codeword, int64_t f, int j, int n) {
    if (!sent) return codeword ? 0x01010101u : 0u;
    const uint8_t* row = sent + f * n + 4 * j;
    if constexpr (VEC) {
        return *reinterpret_cast<const uint32_t*>(row);
    } else {
        uint32_t b4 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) b4 |= (uint32_t)(4 * j + q < n ? row[q] : (uint8_t)0) << (8 * q);
        return b4;
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void store4(T* __restrict__ dst, const T (&out)[4], int j, int n) {
    if constexpr (VEC) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float4*>(dst) = make_float4(out[0], out[1], out[2], out[3]);
        } else {
            *reinterpret_cast<double2*>(dst) = make_double2(out[0], out[1]);
            *reinterpret_cast<double2*>(dst + 2) = make_double2(out[2], out[3]);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * j + q < n) dst[q] = out[q];
    }
}

// one thread = 4 consecutive variables of one frame (one Philox block), as k_biawgn / k_biawgn_sent
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_biawgn_pattern(double sigma, double inv_var2, T short_llr, int codeword, uint64_t seed, uint32_t stream,
                                                        uint64_t frame0, int64_t B, int n, int blocks_per_frame, const uint8_t* __restrict__ sent,
                                                        const uint8_t* __restrict__ kind, T* __restrict__ priors) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t f = gid / blocks_per_frame;
    const int j = (int)(gid - f * blocks_per_frame);
    if (f >= B) return;
    const uint32_t k4 = kinds_of<VEC>(kind, j, n);
    T out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = ((k4 >> (8 * q)) & 0xffu) == KIND_PUNCTURED ? (T)0 : short_llr;
    // a block with no sent variable draws nothing, neither Philox nor Box-Muller: the test is "some byte of k4 is zero"
    if (((k4 - 0x01010101u) & ~k4 & 0x80808080u) != 0) {
        const uint32_t b4 = bits_of<VEC>(sent, codeword, f, j, n);
        const Philox4 p = philox_word_block(seed, stream, frame0 + (uint64_t)f, (uint32_t)j);
        T z[4];
        box_muller<T>(p.w[0], p.w[1], z[0], z[1]);
        box_muller<T>(p.w[2], p.w[3], z[2], z[3]);
        const T sg = (T)sigma, kk = (T)inv_var2;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const T yv = (T)(2 * (int)((b4 >> (8 * q)) & 1u) - 1) + sg * z[q];
            if (((k4 >> (8 * q)) & 0xffu) == KIND_SENT) out[q] = -(kk * yv);  // -2y/sigma^2 with kk = 2/sigma^2
        }
    }
    store4<T, VEC>(priors + f * n + 4 * j, out, j, n);
}

// BSC: one word per variable; flip <=> (w + 0.5) * 2^-32 < p <=> w < thr, as k_discrete / k_discrete_sent
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_bsc_pattern(uint64_t thr, double llr, T short_llr, int codeword, uint64_t seed, uint32_t stream, uint64_t frame0,
                                                     int64_t B, int n, int blocks_per_frame, const uint8_t* __restrict__ sent,
                                                     const uint8_t* __restrict__ kind, T* __restrict__ priors, uint8_t* __restrict__ y) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t f = gid / blocks_per_frame;
    const int j = (int)(gid - f * blocks_per_frame);
    if (f >= B) return;
    const uint32_t k4 = kinds_of<VEC>(kind, j, n);
    const uint32_t b4 = bits_of<VEC>(sent, codeword, f, j, n);
    const Philox4 p = philox_word_block(seed, stream, frame0 + (uint64_t)f, (uint32_t)j);
    T out[4];
    uint32_t y4 = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t k = (k4 >> (8 * q)) & 0xffu;
        const uint32_t s = (((b4 >> (8 * q)) & 1u) ^ ((uint64_t)p.w[q] < thr ? 1u : 0u));
        if (k == KIND_SENT) {
            out[q] = (T)llr * (T)(1 - 2 * (int)s);
            y4 |= s << (8 * q);
        } else {
            out[q] = k == KIND_PUNCTURED ? (T)0 : short_llr;
        }
    }
    if (priors) store4<T, VEC>(priors + f * n + 4 * j, out, j, n);
    uint8_t* yd = y + f * n + 4 * j;
    if constexpr (VEC) {
        *reinterpret_cast<uint32_t*>(yd) = y4;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * j + q < n) yd[q] = (uint8_t)(y4 >> (8 * q));
    }
}

// k_count (ldpc_channel.hip) over the variables with kind < 2: one wavefront per frame, grid-stride; counters combined per block (LDS)
// before the global atomics; `sent` is one word PER FRAME [B, n] or null for the all-`codeword` word.  A byte above 2 reads as shortened
// here as in the channel kernels.  The body is k_count's with one more term -- k_count keeps its machine code, so it is not shared: a
// change to the counters or the histogram rule of either kernel belongs in both.
__global__ __launch_bounds__(256) void k_count_pattern(const uint8_t* __restrict__ xhat, const uint8_t* __restrict__ sent, int codeword,
                                                       const uint8_t* __restrict__ kind, const int32_t* __restrict__ iters, int64_t B, int n,
                                                       int hist_bins, unsigned long long* __restrict__ counters) {
    extern __shared__ unsigned int s_hist[];  // [hist_bins]
    __shared__ unsigned long long s_cnt[4];
    for (int i = threadIdx.x; i < hist_bins; i += 256) s_hist[i] = 0;
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long tot = 0, wec = 0, bec = 0, itsum = 0;  // meaningful on lane 0 of each wave
    for (int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); f < B; f += (int64_t)gridDim.x * 4) {
        int err = 0;
        const uint8_t* row = xhat + f * n;
        for (int v = lane; v < n; v += 64) {
            const uint8_t want = sent ? sent[f * n + v] : (uint8_t)codeword;
            err += kind[v] < KIND_SHORTENED && row[v] != want;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) err += __shfl_xor(err, off, 64);
        if (lane == 0) {
            tot += 1;
            wec += err > 0;
            bec += (unsigned long long)err;
            if (iters) {
                const int it = iters[f];
                itsum += (unsigned long long)it;
                if (hist_bins > 0) atomicAdd(&s_hist[it < 0 ? 0 : (it < hist_bins ? it : hist_bins - 1)], 1u);
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&s_cnt[0], tot);
        atomicAdd(&s_cnt[1], wec);
        atomicAdd(&s_cnt[2], bec);
        atomicAdd(&s_cnt[3], itsum);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], s_cnt[threadIdx.x]);
    for (int i = threadIdx.x; i < hist_bins; i += 256)
        if (s_hist[i]) atomicAdd(&counters[4 + i], (unsigned long long)s_hist[i]);
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

int channel_pattern(int channel, int dtype, double param, const uint8_t* sent, int codeword, const uint8_t* kind, double short_llr, uint64_t seed,
                    uint64_t stream_id, uint64_t frame0, int64_t B, int32_t n, void* priors, uint8_t* y, hipStream_t st) {
    if (!kind || B < 0 || n <= 0 || dtype < 0 || dtype > 1) {
        set_error("ldpc_channel_pattern: bad arguments");
        return LDPC_E_ARG;
    }
    if ((channel & CH_RAW_OBSERVATION) != 0 || LDPC_CH_PRIOR_GRID_OF(channel) >= 0) {
        set_error("ldpc_channel_pattern: the raw-observation and prior-grid flags are not taken here; a pattern writes LLRs, off any grid but short_llr");
        return LDPC_E_ARG;
    }
    if (channel == CH_BEC) {
        set_error("ldpc_channel_pattern: the erasure channel has no pattern (LDPC_CH_BIAWGN and LDPC_CH_BSC)");
        return LDPC_E_ARG;
    }
    if (channel != CH_BIAWGN && channel != CH_BSC) {
        set_error("ldpc_channel_pattern: unknown channel id %d (plain LDPC_CH_BIAWGN / LDPC_CH_BSC only)", channel);
        return LDPC_E_ARG;
    }
    if (!(short_llr > 0.0) || !std::isfinite(short_llr)) {
        set_error("ldpc_channel_pattern: short_llr must be finite and > 0 (got %g)", short_llr);
        return LDPC_E_ARG;
    }
    if (!sent && codeword != 0 && codeword != 1) {
        set_error("ldpc_channel_pattern: without sent words the all-zero (0) or all-one (1) word is sent; got codeword=%d", codeword);
        return LDPC_E_ARG;
    }
    if (!sent && codeword == 1) {  // (the one case that reads the pattern back and waits for `st`; a caller that has checked sends words of ones)
        std::vector<uint8_t> host((size_t)n);
        LDPC_HIP_TRY(hipMemcpyAsync(host.data(), kind, (size_t)n, hipMemcpyDeviceToHost, st));
        LDPC_HIP_TRY(hipStreamSynchronize(st));
        for (int32_t v = 0; v < n; ++v)
            if (host[(size_t)v] == KIND_SHORTENED) {
                set_error("ldpc_channel_pattern: the all-one word is no codeword of the shortened code (variable %d is shortened)", v);
                return LDPC_E_ARG;
            }
    }
    if (channel == CH_BIAWGN ? !priors : !y) {
        set_error(channel == CH_BIAWGN ? "ldpc_channel_pattern: biawgn needs a priors output buffer" : "ldpc_channel_pattern: the bsc needs the y output buffer");
        return LDPC_E_ARG;
    }
    if (B == 0) return LDPC_OK;
    const int bpf = (n + 3) / 4;
    const int64_t threads = B * bpf;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    // the dword / float4 / double2 path: n a multiple of 4 and every buffer on its natural boundary (rows then are too)
    const bool vec = (n & 3) == 0 && aligned(kind, 4) && aligned(sent, 4) && aligned(priors, 16) && aligned(y, 4);
    if (channel == CH_BIAWGN) {
        const double var = pow(10.0, -param / 10.0);  // src/biawgn.py:10, as channel_generate_words
        const double sigma = sqrt(var), kk = 2.0 / var;
        if (dtype == DT_F64) {
            if (vec) hipLaunchKernelGGL((k_biawgn_pattern<double, true>), grid, block, 0, st, sigma, kk, short_llr, codeword, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, kind, (double*)priors);
            else hipLaunchKernelGGL((k_biawgn_pattern<double, false>), grid, block, 0, st, sigma, kk, short_llr, codeword, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, kind, (double*)priors);
        } else {
            if (vec) hipLaunchKernelGGL((k_biawgn_pattern<float, true>), grid, block, 0, st, sigma, kk, (float)short_llr, codeword, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, kind, (float*)priors);
            else hipLaunchKernelGGL((k_biawgn_pattern<float, false>), grid, block, 0, st, sigma, kk, (float)short_llr, codeword, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, kind, (float*)priors);
        }
    } else {
        if (!(param >= 0.0 && param <= 1.0)) {
            set_error("ldpc_channel_pattern: channel probability %g outside [0,1]", param);
            return LDPC_E_ARG;
        }
        double t = ceil(param * 4294967296.0 - 0.5);  // (w + 0.5) * 2^-32 < p  <=>  w < ceil(p * 2^32 - 0.5)
        if (t < 0) t = 0;
        const uint64_t thr = (uint64_t)t;
        const double llr = log(1.0 - param) - log(param);  // src/bsc.py:21
        if (dtype == DT_F64) {
            if (vec) hipLaunchKernelGGL((k_bsc_pattern<double, true>), grid, block, 0, st, thr, llr, short_llr, codeword, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, kind, (double*)priors, y);
            else hipLaunchKernelGGL((k_bsc_pattern<double, false>), grid, block, 0, st, thr, llr, short_llr, codeword, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, kind, (double*)priors, y);
        } else {
            if (vec) hipLaunchKernelGGL((k_bsc_pattern<float, true>), grid, block, 0, st, thr, llr, (float)short_llr, codeword, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, kind, (float*)priors, y);
            else hipLaunchKernelGGL((k_bsc_pattern<float, false>), grid, block, 0, st, thr, llr, (float)short_llr, codeword, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, kind, (float*)priors, y);
        }
    }
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int count_errors_pattern(const uint8_t* xhat, const uint8_t* sent, int codeword, const uint8_t* kind, const int32_t* iters, int64_t B, int32_t n,
                         int32_t hist_bins, int64_t* counters, hipStream_t st) {
    if (!xhat || !kind || !counters || B < 0 || n <= 0 || hist_bins < 0) {
        set_error("ldpc_count_errors_pattern: bad arguments");
        return LDPC_E_ARG;
    }
    if (hist_bins > 8192) {
        set_error("ldpc_count_errors_pattern: at most 8192 histogram bins");
        return LDPC_E_ARG;
    }
    if (B == 0) return LDPC_OK;
    const int64_t want = (B + 3) / 4;
    const unsigned grid = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(k_count_pattern, dim3(grid), dim3(256), (size_t)hist_bins * sizeof(unsigned int), st, xhat, sent, codeword, kind, iters, B, n,
                       hist_bins, (unsigned long long*)counters);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

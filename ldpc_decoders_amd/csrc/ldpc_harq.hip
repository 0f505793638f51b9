// Incremental-redundancy HARQ: what a retransmission loop needs beside the decoders, none of which changes.
//
// The schedule is made on the host (ratematch.Harq): the circular buffer is the variables of kind 0 of a transmission pattern in ascending
// index, transmission t sends E_t buffer positions from its start k_t, wrapping (E_t > Ncb repeats).  What reaches the device is two bytes
// per variable and transmission: cnt[v], how many copies of v this transmission sends, and first[v], how many copies every earlier
// transmission sent -- the ordinal of this transmission's first copy.
//
//   transmit   row i of the new soft buffer = row src[i] of the old one + the LLRs of this transmission's copies, added in ascending
//              ordinal r, one addition each.  Copy r of variable v of global frame g draws word v % 4 of Philox block v / 4 of stream word
//              stream_id + (r << 16): r = 0 is the draw of ldpc_channel_pattern bit for bit, every later copy is independent of it and
//              still a function of (seed, stream, global frame) alone.  The two buffers ping-pong, so the gather of the frames that go on
//              rides inside the transmission.
//   syndrome   fail[f] = some check of the code is not satisfied by xhat[f]: the acknowledgement of a system without a CRC
//   tally      the counters of k_count_pattern for the rows that LEAVE (acknowledged, or the last transmission), the iteration counters
//              for every attempt, and behind them ack[t], undetected, sym
#include "ldpc_harq.hpp"

#include <cmath>
#include <vector>

#include "ldpc_ratematch.hpp"
#include "ldpc_rng.hpp"

namespace ldpc {
namespace {

// four bytes of a per-variable table (or of a sent word) at variables 4j .. 4j+3 (VEC: one dword, n % 4 == 0; else bytes, `beyond` past n)
template <bool VEC>
__device__ __forceinline__ uint32_t bytes4(const uint8_t* __restrict__ p, int j, int n, uint32_t beyond) {
    if constexpr (VEC) {
        return *reinterpret_cast<const uint32_t*>(p + 4 * j);
    } else {
        uint32_t b4 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) b4 |= (4 * j + q < n ? (uint32_t)p[4 * j + q] : beyond) << (8 * q);
        return b4;
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void load4(const T* __restrict__ srcp, T (&acc)[4], int j, int n) {
    if constexpr (VEC) {
        if constexpr (sizeof(T) == 4) {
            const float4 a = *reinterpret_cast<const float4*>(srcp);
            acc[0] = a.x, acc[1] = a.y, acc[2] = a.z, acc[3] = a.w;
        } else {
            const double2 a = *reinterpret_cast<const double2*>(srcp), b = *reinterpret_cast<const double2*>(srcp + 2);
            acc[0] = a.x, acc[1] = a.y, acc[2] = b.x, acc[3] = b.y;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = 4 * j + q < n ? srcp[q] : (T)0;
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

// what every transmit kernel reads before it draws: the row's place in the old buffer and in the sent words, the copies of its four
// variables, and the values it starts from.  false: the row's src or orig lies outside its buffer -- nothing is read or written for it.
struct HarqRow {
    int64_t frame;      // orig[i]: the row of the sent words, and the offset of the global frame
    uint32_t c[4], f[4];  // copies in this transmission (0 for a variable outside the buffer) and the ordinal of the first of them
    uint32_t lo, hi;    // ordinals [lo, hi) are those at which some variable of the block has a copy
};

template <typename T, bool VEC>
__device__ __forceinline__ bool harq_row(int64_t i, int j, int n, T short_llr, const uint8_t* __restrict__ kind, const uint8_t* __restrict__ cnt,
                                         const uint8_t* __restrict__ first, const int64_t* __restrict__ src, const int64_t* __restrict__ orig,
                                         const T* __restrict__ soft_old, int64_t old_rows, bool has_sent, int64_t sent_rows, HarqRow& row, T (&acc)[4]) {
    row.frame = orig ? orig[i] : i;
    if (has_sent && (row.frame < 0 || row.frame >= sent_rows)) return false;
    const uint32_t k4 = bytes4<VEC>(kind, j, n, KIND_PUNCTURED), c4 = bytes4<VEC>(cnt, j, n, 0), f4 = bytes4<VEC>(first, j, n, 0);
    if (soft_old) {
        const int64_t s = src ? src[i] : i;
        if (s < 0 || s >= old_rows) return false;
        load4<T, VEC>(soft_old + s * n + 4 * j, acc, j, n);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = ((k4 >> (8 * q)) & 0xffu) < KIND_SHORTENED ? (T)0 : short_llr;
    }
    row.lo = 256, row.hi = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        row.c[q] = ((k4 >> (8 * q)) & 0xffu) == KIND_SENT ? (c4 >> (8 * q)) & 0xffu : 0u;  // (a shortened value never changes)
        row.f[q] = (f4 >> (8 * q)) & 0xffu;
        if (row.c[q]) {
            row.lo = row.f[q] < row.lo ? row.f[q] : row.lo;
            row.hi = row.f[q] + row.c[q] > row.hi ? row.f[q] + row.c[q] : row.hi;
        }
    }
    return true;
}

// variable q of the block has a copy at ordinal r  <=>  f <= r < f + c  (unsigned: r < f wraps beyond any c)
__device__ __forceinline__ bool harq_on(const HarqRow& row, int q, uint32_t r) { return r - row.f[q] < row.c[q]; }
__device__ __forceinline__ bool harq_any(const HarqRow& row, uint32_t r) {
    return harq_on(row, 0, r) || harq_on(row, 1, r) || harq_on(row, 2, r) || harq_on(row, 3, r);
}

// one thread = 4 consecutive variables of one output row (one Philox block per copy ordinal), as k_biawgn_pattern; the Box-Muller pairing
// and the -(kk * y) form are that kernel's, so ordinal 0 is its draw bit for bit
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_harq_biawgn(double sigma, double inv_var2, T short_llr, int codeword, uint64_t seed, uint32_t stream,
                                                     uint64_t frame0, int64_t B_out, int n, int blocks_per_frame, const uint8_t* __restrict__ sent,
                                                     int64_t sent_rows, const uint8_t* __restrict__ kind, const uint8_t* __restrict__ cnt,
                                                     const uint8_t* __restrict__ first, const int64_t* __restrict__ src,
                                                     const int64_t* __restrict__ orig, const T* __restrict__ soft_old, int64_t old_rows,
                                                     T* __restrict__ soft_new) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = gid / blocks_per_frame;
    const int j = (int)(gid - i * blocks_per_frame);
    if (i >= B_out) return;
    HarqRow row;
    T acc[4];
    if (!harq_row<T, VEC>(i, j, n, short_llr, kind, cnt, first, src, orig, soft_old, old_rows, sent != nullptr, sent_rows, row, acc)) return;
    if (row.lo < row.hi) {
        const uint32_t b4 = sent ? bytes4<VEC>(sent + row.frame * n, j, n, 0) : (codeword ? 0x01010101u : 0u);
        const T sg = (T)sigma, kk = (T)inv_var2;
        for (uint32_t r = row.lo; r < row.hi; ++r) {
            if (!harq_any(row, r)) continue;  // a block without a copy at this ordinal draws nothing for it
            const Philox4 p = philox_word_block(seed, stream + (r << 16), frame0 + (uint64_t)row.frame, (uint32_t)j);
            T z[4];
            box_muller<T>(p.w[0], p.w[1], z[0], z[1]);
            box_muller<T>(p.w[2], p.w[3], z[2], z[3]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const T yv = (T)(2 * (int)((b4 >> (8 * q)) & 1u) - 1) + sg * z[q];
                const T llr = -(kk * yv);  // -2y/sigma^2 with kk = 2/sigma^2
                if (harq_on(row, q, r)) acc[q] = acc[q] + llr;
            }
        }
    }
    store4<T, VEC>(soft_new + i * n + 4 * j, acc, j, n);
}

// BSC: one word per copy; flip <=> w < thr and the LLR +-llr, as k_bsc_pattern
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_harq_bsc(uint64_t thr, double llr, T short_llr, int codeword, uint64_t seed, uint32_t stream, uint64_t frame0,
                                                  int64_t B_out, int n, int blocks_per_frame, const uint8_t* __restrict__ sent, int64_t sent_rows,
                                                  const uint8_t* __restrict__ kind, const uint8_t* __restrict__ cnt, const uint8_t* __restrict__ first,
                                                  const int64_t* __restrict__ src, const int64_t* __restrict__ orig, const T* __restrict__ soft_old,
                                                  int64_t old_rows, T* __restrict__ soft_new) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = gid / blocks_per_frame;
    const int j = (int)(gid - i * blocks_per_frame);
    if (i >= B_out) return;
    HarqRow row;
    T acc[4];
    if (!harq_row<T, VEC>(i, j, n, short_llr, kind, cnt, first, src, orig, soft_old, old_rows, sent != nullptr, sent_rows, row, acc)) return;
    if (row.lo < row.hi) {
        const uint32_t b4 = sent ? bytes4<VEC>(sent + row.frame * n, j, n, 0) : (codeword ? 0x01010101u : 0u);
        for (uint32_t r = row.lo; r < row.hi; ++r) {
            if (!harq_any(row, r)) continue;
            const Philox4 p = philox_word_block(seed, stream + (r << 16), frame0 + (uint64_t)row.frame, (uint32_t)j);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t s = (((b4 >> (8 * q)) & 1u) ^ ((uint64_t)p.w[q] < thr ? 1u : 0u));
                const T v = (T)llr * (T)(1 - 2 * (int)s);
                if (harq_on(row, q, r)) acc[q] = acc[q] + v;
            }
        }
    }
    store4<T, VEC>(soft_new + i * n + 4 * j, acc, j, n);
}

// one wavefront per frame, grid-stride; lanes stride over the checks; a check XORs the bytes of its row, the wave ORs the results
__global__ __launch_bounds__(256) void k_harq_syndrome(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var,
                                                       const uint8_t* __restrict__ xhat, int64_t B, int m, int n, uint8_t* __restrict__ fail) {
    const int lane = threadIdx.x & 63;
    for (int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); f < B; f += (int64_t)gridDim.x * 4) {
        const uint8_t* row = xhat + f * n;
        int bad = 0;
        for (int c = lane; c < m; c += 64) {
            uint32_t x = 0;
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) x ^= row[edge_var[e]];
            bad |= (int)x;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) bad |= __shfl_xor(bad, off, 64);
        if (lane == 0) fail[f] = bad != 0;
    }
}

// k_count_pattern (ldpc_ratematch.hip) for a retransmission loop: one wavefront per row, grid-stride; counters combined per block (LDS)
// before the global atomics.  Every row is one decode attempt (ITER_SUM, histogram, sym); a row that leaves -- acknowledged, or the last
// transmission -- is one frame (TOT, WEC, BEC over kind < 2 against sent[orig[i]]).  The body is k_count's with these terms -- k_count and
// k_count_pattern keep their machine code, so it is not shared: a change to the counters or the histogram rule of one kernel belongs in
// all three.
__global__ __launch_bounds__(256) void k_harq_tally(const uint8_t* __restrict__ xhat, const uint8_t* __restrict__ sent, int64_t sent_rows, int codeword,
                                                    const uint8_t* __restrict__ kind, const int32_t* __restrict__ iters,
                                                    const uint8_t* __restrict__ fail, const int64_t* __restrict__ orig, int64_t B, int n,
                                                    int hist_bins, int t, int T, unsigned long long tx_bits,
                                                    unsigned long long* __restrict__ counters) {
    extern __shared__ unsigned int s_hist[];  // [hist_bins]
    __shared__ unsigned long long s_cnt[7];
    for (int i = threadIdx.x; i < hist_bins; i += 256) s_hist[i] = 0;
    if (threadIdx.x < 7) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long tot = 0, wec = 0, bec = 0, itsum = 0, ack = 0, und = 0, sym = 0;  // meaningful on lane 0 of each wave
    for (int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); f < B; f += (int64_t)gridDim.x * 4) {
        int err = 0;
        const uint8_t* row = xhat + f * n;
        const int64_t o = orig ? orig[f] : f;
        const bool have = !sent || (o >= 0 && o < sent_rows);  // (a row whose word lies outside the sent words counts against `codeword`)
        for (int v = lane; v < n; v += 64) {
            const uint8_t want = sent && have ? sent[o * n + v] : (uint8_t)codeword;
            err += kind[v] < KIND_SHORTENED && row[v] != want;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) err += __shfl_xor(err, off, 64);
        if (lane == 0) {
            const bool acked = fail[f] == 0;
            sym += tx_bits;
            if (acked || t == T - 1) {
                tot += 1;
                wec += err > 0;
                bec += (unsigned long long)err;
            }
            if (acked) {
                ack += 1;
                und += err > 0;
            }
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
        atomicAdd(&s_cnt[4], ack);
        atomicAdd(&s_cnt[5], und);
        atomicAdd(&s_cnt[6], sym);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], s_cnt[threadIdx.x]);
    for (int i = threadIdx.x; i < hist_bins; i += 256)
        if (s_hist[i]) atomicAdd(&counters[4 + i], (unsigned long long)s_hist[i]);
    unsigned long long* extra = counters + 4 + hist_bins;  // ack[T], undetected, sym
    if (threadIdx.x == 4 && s_cnt[4]) atomicAdd(&extra[t], s_cnt[4]);
    if (threadIdx.x == 5 && s_cnt[5]) atomicAdd(&extra[T], s_cnt[5]);
    if (threadIdx.x == 6 && s_cnt[6]) atomicAdd(&extra[T + 1], s_cnt[6]);
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <typename T>
void launch_transmit(int channel, bool vec, dim3 grid, hipStream_t st, double a, double b, uint64_t thr, double short_llr, int codeword, uint64_t seed,
                     uint32_t stream, uint64_t frame0, int64_t B_out, int n, int bpf, const uint8_t* sent, int64_t sent_rows, const uint8_t* kind,
                     const uint8_t* cnt, const uint8_t* first, const int64_t* src, const int64_t* orig, const void* soft_old, int64_t old_rows,
                     void* soft_new) {
    const dim3 block(256);
    const T sl = (T)short_llr;
    const T* so = (const T*)soft_old;
    T* sn = (T*)soft_new;
    if (channel == CH_BIAWGN) {
        if (vec) hipLaunchKernelGGL((k_harq_biawgn<T, true>), grid, block, 0, st, a, b, sl, codeword, seed, stream, frame0, B_out, n, bpf, sent, sent_rows, kind, cnt, first, src, orig, so, old_rows, sn);
        else hipLaunchKernelGGL((k_harq_biawgn<T, false>), grid, block, 0, st, a, b, sl, codeword, seed, stream, frame0, B_out, n, bpf, sent, sent_rows, kind, cnt, first, src, orig, so, old_rows, sn);
    } else {
        if (vec) hipLaunchKernelGGL((k_harq_bsc<T, true>), grid, block, 0, st, thr, a, sl, codeword, seed, stream, frame0, B_out, n, bpf, sent, sent_rows, kind, cnt, first, src, orig, so, old_rows, sn);
        else hipLaunchKernelGGL((k_harq_bsc<T, false>), grid, block, 0, st, thr, a, sl, codeword, seed, stream, frame0, B_out, n, bpf, sent, sent_rows, kind, cnt, first, src, orig, so, old_rows, sn);
    }
}

}  // namespace

int harq_transmit(int channel, int dtype, double param, const uint8_t* sent, int64_t sent_rows, int codeword, const uint8_t* kind, const uint8_t* cnt,
                  const uint8_t* first, double short_llr, uint64_t seed, uint64_t stream_id, uint64_t frame0, const int64_t* src, const int64_t* orig,
                  const void* soft_old, int64_t old_rows, int64_t B_out, int32_t n, void* soft_new, hipStream_t st) {
    if (!kind || !cnt || !first || !soft_new || B_out < 0 || n <= 0 || dtype < 0 || dtype > 1 || (sent && sent_rows < 0) || (soft_old && old_rows < 0)) {
        set_error("ldpc_harq_transmit: bad arguments");
        return LDPC_E_ARG;
    }
    if (soft_old == soft_new) {
        set_error("ldpc_harq_transmit: the two soft buffers ping-pong; a transmission cannot gather rows inside the buffer it writes");
        return LDPC_E_ARG;
    }
    if (stream_id >= 65536) {
        set_error("ldpc_harq_transmit: stream_id %llu: the copy ordinal lives in bits 16 and up of the stream word, so stream_id < 65536",
                  (unsigned long long)stream_id);
        return LDPC_E_ARG;
    }
    if ((channel & CH_RAW_OBSERVATION) != 0 || LDPC_CH_PRIOR_GRID_OF(channel) >= 0) {
        set_error("ldpc_harq_transmit: the raw-observation and prior-grid flags are not taken here; a soft buffer holds sums of LLRs, off any grid");
        return LDPC_E_ARG;
    }
    if (channel == CH_BEC) {
        set_error("ldpc_harq_transmit: the erasure channel has no soft buffer (LDPC_CH_BIAWGN and LDPC_CH_BSC)");
        return LDPC_E_ARG;
    }
    if (channel != CH_BIAWGN && channel != CH_BSC) {
        set_error("ldpc_harq_transmit: unknown channel id %d (plain LDPC_CH_BIAWGN / LDPC_CH_BSC only)", channel);
        return LDPC_E_ARG;
    }
    if (!(short_llr > 0.0) || !std::isfinite(short_llr)) {
        set_error("ldpc_harq_transmit: short_llr must be finite and > 0 (got %g)", short_llr);
        return LDPC_E_ARG;
    }
    if (!sent && codeword != 0 && codeword != 1) {
        set_error("ldpc_harq_transmit: without sent words the all-zero (0) or all-one (1) word is sent; got codeword=%d", codeword);
        return LDPC_E_ARG;
    }
    if (channel == CH_BSC && !(param >= 0.0 && param <= 1.0)) {
        set_error("ldpc_harq_transmit: channel probability %g outside [0,1]", param);
        return LDPC_E_ARG;
    }
    if (!sent && codeword == 1) {  // (reads the pattern back and waits for `st`, as ldpc_channel_pattern; a caller that has checked sends words of ones)
        std::vector<uint8_t> host((size_t)n);
        LDPC_HIP_TRY(hipMemcpyAsync(host.data(), kind, (size_t)n, hipMemcpyDeviceToHost, st));
        LDPC_HIP_TRY(hipStreamSynchronize(st));
        for (int32_t v = 0; v < n; ++v)
            if (host[(size_t)v] >= KIND_SHORTENED) {
                set_error("ldpc_harq_transmit: the all-one word is no codeword of the shortened code (variable %d is shortened)", v);
                return LDPC_E_ARG;
            }
    }
    if (B_out == 0) return LDPC_OK;
    const int bpf = (n + 3) / 4;
    const int64_t blocks = (B_out * bpf + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        set_error("ldpc_harq_transmit: %lld rows of %d variables are more than one launch takes", (long long)B_out, n);
        return LDPC_E_ARG;
    }
    // the dword / float4 / double2 path: n a multiple of 4 and every buffer on its natural boundary (rows then are too)
    const bool vec = (n & 3) == 0 && aligned(kind, 4) && aligned(cnt, 4) && aligned(first, 4) && aligned(sent, 4) && aligned(soft_old, 16) && aligned(soft_new, 16);
    const dim3 grid((unsigned)blocks);
    double a, b = 0.0;
    uint64_t thr = 0;
    if (channel == CH_BIAWGN) {
        const double var = pow(10.0, -param / 10.0);  // src/biawgn.py:10, as channel_pattern
        a = sqrt(var), b = 2.0 / var;
    } else {
        double t = ceil(param * 4294967296.0 - 0.5);  // (w + 0.5) * 2^-32 < p  <=>  w < ceil(p * 2^32 - 0.5)
        if (t < 0) t = 0;
        thr = (uint64_t)t;
        a = log(1.0 - param) - log(param);  // src/bsc.py:21
    }
    if (dtype == DT_F64)
        launch_transmit<double>(channel, vec, grid, st, a, b, thr, short_llr, codeword, seed, (uint32_t)stream_id, frame0, B_out, n, bpf, sent, sent_rows, kind, cnt, first, src, orig, soft_old, old_rows, soft_new);
    else
        launch_transmit<float>(channel, vec, grid, st, a, b, thr, short_llr, codeword, seed, (uint32_t)stream_id, frame0, B_out, n, bpf, sent, sent_rows, kind, cnt, first, src, orig, soft_old, old_rows, soft_new);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int harq_syndrome(const Code* c, const uint8_t* xhat, int64_t B, uint8_t* fail, hipStream_t st) {
    if (!c || !xhat || !fail || B < 0) {
        set_error("ldpc_harq_syndrome: bad arguments");
        return LDPC_E_ARG;
    }
    if (B == 0) return LDPC_OK;
    const int64_t want = (B + 3) / 4;
    const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
    hipLaunchKernelGGL(k_harq_syndrome, dim3(grid), dim3(256), 0, st, c->d_row_ptr, c->d_edge_var, xhat, B, c->m, c->n, fail);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int harq_tally(const uint8_t* xhat, const uint8_t* sent, int64_t sent_rows, int codeword, const uint8_t* kind, const int32_t* iters, const uint8_t* fail,
               const int64_t* orig, int64_t B, int32_t n, int32_t hist_bins, int32_t t, int32_t T, int64_t tx_bits, int64_t* counters, hipStream_t st) {
    if (!xhat || !kind || !fail || !counters || B < 0 || n <= 0 || hist_bins < 0 || tx_bits < 0 || (sent && sent_rows < 0)) {
        set_error("ldpc_harq_tally: bad arguments");
        return LDPC_E_ARG;
    }
    if (T < 1 || T > HARQ_MAX_TX || t < 0 || t >= T) {
        set_error("ldpc_harq_tally: transmission %d of %d (1 <= T <= %d, 0 <= t < T)", t, T, HARQ_MAX_TX);
        return LDPC_E_ARG;
    }
    if (hist_bins > 8192) {
        set_error("ldpc_harq_tally: at most 8192 histogram bins");
        return LDPC_E_ARG;
    }
    if (B == 0) return LDPC_OK;
    const int64_t want = (B + 3) / 4;
    const unsigned grid = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(k_harq_tally, dim3(grid), dim3(256), (size_t)hist_bins * sizeof(unsigned int), st, xhat, sent, sent_rows, codeword, kind, iters,
                       fail, orig, B, n, hist_bins, t, T, (unsigned long long)tx_bits, (unsigned long long*)counters);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

// Systematic GF(2) encoder (--codeword -1 for every code) and the channel of a given word per frame.
//
// The host (ldpc_decoders_amd/encoder.py) brings H to reduced row echelon form over GF(2): r = rank pivot columns par_pos, k' = n - r
// information columns info_pos, and P (k' x r bits) with  c[par_pos] = u . P mod 2,  c[info_pos] = u.  Encoding B frames is the 0/1
// integer GEMM  [B x k'] . [k' x r], done here on the i8 matrix cores (v_mfma_i32_32x32x32_i8): 0/1 bytes in, int32 accumulation
// (exact for k' < 2^31), & 1 out.  No tolerance anywhere.
//
// Data layout:
//   * P lives in HBM as BITS, in the order its MFMA fragments consume them: for column tile t (32 parity columns), k-group g (4 k-steps of
//     32 information bits) and lane l (c = l & 31, h = l >> 5), one uint64 holds four 16-bit pieces, piece q = bits e = 0..15 of
//     P[128 g + 32 q + 16 h + e][32 t + c].  A wave loads one uint64 per lane per (tile, k-group): 512 coalesced bytes.  Rows >= k' and
//     columns >= r are zero.  3.2 MB for n = 10 000: the whole matrix stays in one XCD's L2.
//   * A 16-bit piece becomes the 16-byte MFMA operand in registers: nibble d -> dword d via (x * 0x00204081) & 0x01010101.  The A operand
//     (information bits) is expanded the same way, so A and B agree on the k order inside a fragment whatever the hardware's lane map
//     of k is; only the documented row (A) / column (B) lane maps and the C/D map are relied on.
//   * Random mode: the information bits of frame f are Philox4x32-10 keyed like every other draw (seed, stream id, global frame index),
//     blocks 0x80000000 + j: bit t of word w of block j is information bit 128 j + 32 w + t.  One block = one k-group, computed in
//     registers by the lane that owns the frame's A row: A never exists in memory.  Disjoint from the noise blocks 0 .. n/4, the
//     code-book pick 0xFFFFFFFE and the ML tie-break 0xFFFFFFFF; a frame's word does not depend on how frames are batched.
//   * Output: sent [B, n] bytes, information bits at info_pos, parity bits at par_pos -- what ldpc_count_errors_words reads.
#include <new>

#include "ldpc_common.hpp"
#include "ldpc_encode.hpp"
#include "ldpc_rng.hpp"

namespace ldpc {

struct Encoder {
    int device = 0;
    int32_t n = 0, k = 0, r = 0;
    int32_t kgroups = 0;  // ceil(k / 128): k-groups of 4 MFMA k-steps (= Philox blocks)
    int32_t nt = 1;       // 32-column tiles per wave (template parameter of k_encode)
    int32_t cgroups = 0;  // column groups of nt tiles
    int32_t* d_info = nullptr;   // [k]
    int32_t* d_par = nullptr;    // [cgroups * nt * 32], -1 beyond r
    uint64_t* d_P = nullptr;     // [cgroups * nt][kgroups][64]
    DevBuf words;                // user-supplied mode: packed information words [B][4 * kgroups]
};

namespace {

constexpr uint32_t INFO_BLOCK0 = 0x80000000u;
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// 16 bits -> 16 bytes in {0,1}: bit 4d + b -> byte b of dword d
__device__ __forceinline__ v4i expand16(uint32_t x) {
    v4i o;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = (int)((((x >> (4 * d)) & 0xFu) * 0x00204081u) & 0x01010101u);
    return o;
}

// One wave = 32 frames x (NT x 32) parity columns, the whole k loop; block = 4 waves on consecutive frame groups, blockIdx.y = column
// group (consecutive blocks share one slice of P: it stays in L2).  RANDOM: information words from Philox; else from `words`.
template <int NT, bool RANDOM>
__global__ __launch_bounds__(256) void k_encode(const uint64_t* __restrict__ P, const int32_t* __restrict__ par, int kgroups, int n,
                                                uint64_t seed, uint32_t stream, uint64_t frame0, int64_t B,
                                                const uint32_t* __restrict__ words, uint8_t* __restrict__ sent) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int64_t fbase = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (fbase >= B) return;
    const int64_t f = fbase + (lane & 31);  // this lane's A row
    const bool live = f < B;
    const int tile0 = blockIdx.y * NT;
    v16i acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v16i{};
    for (int g = 0; g < kgroups; ++g) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (live) {
            if constexpr (RANDOM) {
                const Philox4 p = philox_word_block(seed, stream, frame0 + (uint64_t)f, INFO_BLOCK0 + (uint32_t)g);
                w[0] = p.w[0], w[1] = p.w[1], w[2] = p.w[2], w[3] = p.w[3];
            } else {
                const uint4 q = *reinterpret_cast<const uint4*>(words + (f * kgroups + g) * 4);
                w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
            }
        }
        uint64_t b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) b[t] = P[((int64_t)(tile0 + t) * kgroups + g) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4i a = expand16(w[q] >> (16 * h));
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const v4i bf = expand16((uint32_t)(b[t] >> (16 * q)));
                acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bf, acc[t], 0, 0, 0);
            }
        }
    }
    // C/D map of the 32x32 MFMA: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 h for accumulator register i
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pos = par[(tile0 + t) * 32 + (lane & 31)];
        if (pos < 0) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t fr = fbase + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (fr < B) sent[fr * n + pos] = (uint8_t)(acc[t][i] & 1);
        }
    }
}

// Information bits into sent[f, info_pos[.]]: one wave per (frame, chunk of 8192 bits); lane l of iteration i owns bit 8192 c + 64 i + l.
// RANDOM: lane j of the wave computes Philox block 64 c + j once, the bits travel by ds_bpermute.  Else the bits are read from u [B, k]
// bytes, and the packed words [B][4 kgroups] that k_encode reads are written as well (two ballots' worth per iteration).
template <bool RANDOM>
__global__ __launch_bounds__(256) void k_info(const int32_t* __restrict__ info, int k, int kgroups, int n, uint64_t seed, uint32_t stream,
                                              uint64_t frame0, int64_t B, const uint8_t* __restrict__ u, uint32_t* __restrict__ words,
                                              uint8_t* __restrict__ sent) {
    const int lane = threadIdx.x & 63;
    const int chunks = (kgroups + 63) / 64;
    const int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t f = task / chunks;
    if (f >= B) return;
    const int c = (int)(task - f * chunks);
    const int kbits = kgroups * 128;
    Philox4 p{{0u, 0u, 0u, 0u}};
    if constexpr (RANDOM) {
        if (64 * c + lane < kgroups) p = philox_word_block(seed, stream, frame0 + (uint64_t)f, INFO_BLOCK0 + (uint32_t)(64 * c + lane));
    }
    const int iters = min(128, (kbits - 8192 * c) / 64);
    for (int i = 0; i < iters; ++i) {
        const int idx = 8192 * c + 64 * i + lane;
        uint32_t bit;
        if constexpr (RANDOM) {
            // bit idx = bit (idx & 31) of word ((idx >> 5) & 3) of block idx >> 7, held by lane (i >> 1) of this wave
            // (the word, 2 (i & 1) + (lane >> 5), differs between the two lane halves: both candidates travel, each half keeps its own)
            const int src = i >> 1;
            const uint32_t lo = (uint32_t)__shfl((int)(i & 1 ? p.w[2] : p.w[0]), src, 64);
            const uint32_t hi = (uint32_t)__shfl((int)(i & 1 ? p.w[3] : p.w[1]), src, 64);
            bit = ((lane >> 5 ? hi : lo) >> (idx & 31)) & 1u;
        } else {
            bit = idx < k ? (uint32_t)(u[f * k + idx] & 1) : 0u;
            const unsigned long long m = __ballot(bit != 0);
            if (lane < 2) words[f * (int64_t)(kgroups * 4) + ((8192 * c + 64 * i) >> 5) + lane] = (uint32_t)(lane ? m >> 32 : m);
        }
        if (idx < k) sent[f * n + info[idx]] = (uint8_t)bit;
    }
}

// Channel.send + LLR for a GIVEN word per frame, sent [B, n]: the noise of ldpc_channel, draw for draw (Philox block j of the frame =
// variables 4j .. 4j+3), so that for an all-zero `sent` the output is exactly ldpc_channel(codeword = 0)'s.
template <typename T>
__global__ __launch_bounds__(256) void k_biawgn_sent(double sigma, double inv_var2, uint64_t seed, uint32_t stream, uint64_t frame0, int64_t B,
                                                     int n, int blocks_per_frame, const uint8_t* __restrict__ sent, T* __restrict__ priors) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t f = gid / blocks_per_frame;
    const int j = (int)(gid - f * blocks_per_frame);
    if (f >= B) return;
    const Philox4 p = philox_word_block(seed, stream, frame0 + (uint64_t)f, (uint32_t)j);
    T z[4];
    box_muller<T>(p.w[0], p.w[1], z[0], z[1]);
    box_muller<T>(p.w[2], p.w[3], z[2], z[3]);
    const T sg = (T)sigma, kk = (T)inv_var2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int v = 4 * j + q;
        if (v < n) {
            const T y = (T)(2 * (int)sent[f * n + v] - 1) + sg * z[q];
            priors[f * n + v] = -(kk * y);
        }
    }
}

template <typename T, int CH>
__global__ __launch_bounds__(256) void k_discrete_sent(uint64_t thr, double llr, uint64_t seed, uint32_t stream, uint64_t frame0, int64_t B, int n,
                                                       int blocks_per_frame, const uint8_t* __restrict__ sent, T* __restrict__ priors,
                                                       uint8_t* __restrict__ y) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t f = gid / blocks_per_frame;
    const int j = (int)(gid - f * blocks_per_frame);
    if (f >= B) return;
    const Philox4 p = philox_word_block(seed, stream, frame0 + (uint64_t)f, (uint32_t)j);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int v = 4 * j + q;
        if (v < n) {
            const bool hit = (uint64_t)p.w[q] < thr;
            const int bit = sent[f * n + v];
            uint8_t s;
            if constexpr (CH == CH_BSC) {
                s = (uint8_t)(bit ^ (hit ? 1 : 0));
                if (priors) priors[f * n + v] = (T)llr * (T)(1 - 2 * (int)s);
            } else {
                s = hit ? (uint8_t)2 : (uint8_t)bit;
            }
            y[f * n + v] = s;
        }
    }
}

template <int NT>
void launch_encode(const Encoder* e, bool random, uint64_t seed, uint32_t stream, uint64_t frame0, int64_t B, const uint32_t* words,
                   uint8_t* sent, hipStream_t st) {
    const dim3 grid((unsigned)((B + 127) / 128), (unsigned)e->cgroups), block(256);
    if (random)
        hipLaunchKernelGGL((k_encode<NT, true>), grid, block, 0, st, e->d_P, e->d_par, e->kgroups, e->n, seed, stream, frame0, B, words, sent);
    else
        hipLaunchKernelGGL((k_encode<NT, false>), grid, block, 0, st, e->d_P, e->d_par, e->kgroups, e->n, seed, stream, frame0, B, words, sent);
}

int encode_impl(Encoder* e, bool random, const uint8_t* u, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, uint8_t* sent,
                hipStream_t st) {
    if (B <= 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(e->device));
    uint32_t* words = nullptr;
    const int chunks = (e->kgroups + 63) / 64;
    if (e->k > 0) {
        if (!random) {
            LDPC_TRY(e->words.reserve((size_t)B * e->kgroups * 16));
            words = (uint32_t*)e->words.p;
        }
        const int64_t waves = B * chunks;
        const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
        if (random)
            hipLaunchKernelGGL((k_info<true>), grid, block, 0, st, e->d_info, e->k, e->kgroups, e->n, seed, (uint32_t)stream_id, frame0, B, u, words, sent);
        else
            hipLaunchKernelGGL((k_info<false>), grid, block, 0, st, e->d_info, e->k, e->kgroups, e->n, seed, (uint32_t)stream_id, frame0, B, u, words, sent);
        LDPC_HIP_TRY(hipGetLastError());
    }
    if (e->r > 0) {
        if (e->k == 0) {  // rank n: the zero word is the only codeword
            LDPC_HIP_TRY(hipMemsetAsync(sent, 0, (size_t)B * (size_t)e->n, st));
            return LDPC_OK;
        }
        switch (e->nt) {
            case 1: launch_encode<1>(e, random, seed, (uint32_t)stream_id, frame0, B, words, sent, st); break;
            case 2: launch_encode<2>(e, random, seed, (uint32_t)stream_id, frame0, B, words, sent, st); break;
            case 4: launch_encode<4>(e, random, seed, (uint32_t)stream_id, frame0, B, words, sent, st); break;
            default: launch_encode<8>(e, random, seed, (uint32_t)stream_id, frame0, B, words, sent, st); break;
        }
        LDPC_HIP_TRY(hipGetLastError());
    }
    return LDPC_OK;
}

template <class V>
int upload_vec(const V& v, void** dst) {
    if (v.empty()) return LDPC_OK;
    const size_t bytes = v.size() * sizeof(v[0]);
    LDPC_HIP_TRY(hipMalloc(dst, bytes));
    LDPC_HIP_TRY(hipMemcpy(*dst, v.data(), bytes, hipMemcpyHostToDevice));
    return LDPC_OK;
}

}  // namespace

void encoder_destroy(Encoder* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->d_info) (void)hipFree(e->d_info);
    if (e->d_par) (void)hipFree(e->d_par);
    if (e->d_P) (void)hipFree(e->d_P);
    e->words.release();
    delete e;
}

int encoder_create(int device, int32_t n, int32_t k, int32_t r, const int32_t* info_pos, const int32_t* par_pos, const uint8_t* P, Encoder** out) {
    if (!out || n <= 0 || k < 0 || r < 0 || (int64_t)k + r != n || (k > 0 && !info_pos) || (r > 0 && !par_pos) || (k > 0 && r > 0 && !P)) {
        set_error("ldpc_encoder_create: bad arguments (need n = k + r > 0 and the position / P arrays)");
        return LDPC_E_ARG;
    }
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int32_t i = 0; i < k; ++i) {
        if (info_pos[i] < 0 || info_pos[i] >= n || seen[info_pos[i]]++) {
            set_error("ldpc_encoder_create: info_pos / par_pos must partition 0 .. n-1");
            return LDPC_E_ARG;
        }
    }
    for (int32_t i = 0; i < r; ++i) {
        if (par_pos[i] < 0 || par_pos[i] >= n || seen[par_pos[i]]++) {
            set_error("ldpc_encoder_create: info_pos / par_pos must partition 0 .. n-1");
            return LDPC_E_ARG;
        }
    }
    Encoder* e = new Encoder();
    e->device = device, e->n = n, e->k = k, e->r = r;
    e->kgroups = (k + 127) / 128;
    // tiles per wave: the fewest padded tiles weighed against how often a frame's information words are drawn again (once per group)
    const int tiles = (r + 31) / 32;
    int best = 8;
    long best_cost = -1;
    for (int nt : {8, 4, 2, 1}) {
        const long groups = (tiles + nt - 1) / nt, cost = groups * (nt + 2);
        if (best_cost < 0 || cost < best_cost) best = nt, best_cost = cost;
    }
    e->nt = best;
    e->cgroups = (tiles + best - 1) / best;
    const int64_t ptiles = (int64_t)e->cgroups * best;
    std::vector<int32_t> par((size_t)(ptiles * 32), -1);
    for (int32_t i = 0; i < r; ++i) par[i] = par_pos[i];
    std::vector<uint64_t> Pf((size_t)(ptiles * e->kgroups * 64), 0);
    for (int64_t j = 0; j < k; ++j) {  // information bit j = 128 g + 32 q + 16 h + b
        const int g = (int)(j >> 7), q = (int)((j >> 5) & 3), hh = (int)((j >> 4) & 1), b = (int)(j & 15);
        const uint8_t* row = P + j * r;
        for (int32_t col = 0; col < r; ++col) {
            if (!row[col]) continue;
            const int64_t t = col >> 5, lane = (col & 31) + 32 * hh;
            Pf[(size_t)((t * e->kgroups + g) * 64 + lane)] |= 1ull << (16 * q + b);
        }
    }
    int rc = LDPC_OK;
    hipError_t he = hipSetDevice(device);
    if (he != hipSuccess) {
        set_error("hipSetDevice(%d) failed: %s", device, hipGetErrorString(he));
        delete e;
        return LDPC_E_HIP;
    }
    std::vector<int32_t> info(info_pos, info_pos + k);
    if ((rc = upload_vec(info, (void**)&e->d_info)) || (rc = upload_vec(par, (void**)&e->d_par)) || (rc = upload_vec(Pf, (void**)&e->d_P))) {
        encoder_destroy(e);
        return rc;
    }
    *out = e;
    return LDPC_OK;
}

int encoder_info(const Encoder* e, int32_t out[4]) {
    if (!e || !out) {
        set_error("ldpc_encoder_info: bad arguments");
        return LDPC_E_ARG;
    }
    out[0] = e->nt, out[1] = e->cgroups, out[2] = e->kgroups, out[3] = (e->kgroups + 63) / 64;
    return LDPC_OK;
}

int encode(Encoder* e, const uint8_t* u, int64_t B, uint8_t* sent, hipStream_t st) {
    if (!e || !sent || B < 0 || (B > 0 && e->k > 0 && !u)) {
        set_error("ldpc_encode: bad arguments");
        return LDPC_E_ARG;
    }
    return encode_impl(e, false, u, 0, 0, 0, B, sent, st);
}

int encode_random(Encoder* e, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, uint8_t* sent, hipStream_t st) {
    if (!e || !sent || B < 0) {
        set_error("ldpc_encode_random: bad arguments");
        return LDPC_E_ARG;
    }
    return encode_impl(e, true, nullptr, seed, stream_id, frame0, B, sent, st);
}

int channel_sent(int channel, int dtype, double param, const uint8_t* sent, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                 int32_t n, void* priors, uint8_t* y, hipStream_t st) {
    if (!sent || B < 0 || n <= 0 || dtype < 0 || dtype > 1) {
        set_error("ldpc_channel_sent: bad arguments");
        return LDPC_E_ARG;
    }
    if (B == 0) return LDPC_OK;
    const int bpf = (n + 3) / 4;
    const int64_t threads = B * bpf;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    if (channel == CH_BIAWGN) {
        if (!priors) {
            set_error("ldpc_channel_sent: biawgn needs a priors output buffer");
            return LDPC_E_ARG;
        }
        const double var = pow(10.0, -param / 10.0);  // src/biawgn.py:10, as channel_generate_words
        const double sigma = sqrt(var), kk = 2.0 / var;
        if (dtype == DT_F64) hipLaunchKernelGGL((k_biawgn_sent<double>), grid, block, 0, st, sigma, kk, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, (double*)priors);
        else hipLaunchKernelGGL((k_biawgn_sent<float>), grid, block, 0, st, sigma, kk, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, (float*)priors);
    } else if (channel == CH_BSC || channel == CH_BEC) {
        if (!y) {
            set_error("ldpc_channel_sent: discrete channels need the y output buffer");
            return LDPC_E_ARG;
        }
        if (!(param >= 0.0 && param <= 1.0)) {
            set_error("channel probability %g outside [0,1]", param);
            return LDPC_E_ARG;
        }
        double t = ceil(param * 4294967296.0 - 0.5);  // (w + 0.5) * 2^-32 < p  <=>  w < ceil(p * 2^32 - 0.5)
        if (t < 0) t = 0;
        const uint64_t thr = (uint64_t)t;
        const double llr = log(1.0 - param) - log(param);  // src/bsc.py:21
        if (channel == CH_BSC) {
            if (dtype == DT_F64) hipLaunchKernelGGL((k_discrete_sent<double, CH_BSC>), grid, block, 0, st, thr, llr, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, (double*)priors, y);
            else hipLaunchKernelGGL((k_discrete_sent<float, CH_BSC>), grid, block, 0, st, thr, llr, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, (float*)priors, y);
        } else {
            hipLaunchKernelGGL((k_discrete_sent<float, CH_BEC>), grid, block, 0, st, thr, 0.0, seed, (uint32_t)stream_id, frame0, B, n, bpf, sent, (float*)nullptr, y);
        }
    } else {
        set_error("ldpc_channel_sent: unknown channel id %d (plain LDPC_CH_* only)", channel);
        return LDPC_E_ARG;
    }
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace ldpc

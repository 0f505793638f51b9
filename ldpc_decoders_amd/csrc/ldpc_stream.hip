// Streaming backend: flooding BP with the message state resident in HBM.
//
// Layout per tile of 64 frames (lane == frame):
//     c2v  [tile][E][64]   T     check -> variable messages, row-major edge order (the order of np.where(H), src/bpa.py:12)
//     marg [tile][n][64]   T     marginals  prior + ordered sum of c2v  (src/bpa.py:35); also the soft output
//     prior[tile][n][64]   T
//     xbits[tile/8][n][8]  u64   hard decision of variable v for the 64 frames of a tile (bit f == frame f); the words of EIGHT
//                                consecutive tiles sit in one 64-byte sector, which is what the syndrome kernel fetches per variable
//     live [tile]          u64   frames that are still iterating
// Every H index is wave-uniform (scalar loads); every message access is one contiguous 64-element line.
//
// One sweep = two passes (round 3: the variable -> check messages are no longer stored):
//   check pass     per check: stream its old c2v lines in, gather the marginal lines of its variables, v2c = marg - c2v_old
//                  (src/bpa.py:37 -- the same subtraction on the same operands, so the same bits), apply the rule, stream c2v out.
//                  Every store of the sweep's E-sized traffic is a contiguous stream; the only random accesses are READS of
//                  marginal lines, each used by dv checks (re-reads are served by the L2 / Infinity Cache).
//   variable pass  per variable: gather its c2v lines (read only), marg = prior + (((0 + c_a) + c_b) + ...), stream marg out,
//                  decision bit-plane.
// HBM bytes per frame-sweep: check pass reads E + n..E, writes E; variable pass reads E + n, writes n  --  3E + 3n when the marginal
// re-reads hit on chip, against the s(4E + n) of SURVEY.md section 8(d) (v2c written and read back); bench.py prices the kernels
// with the section-8(d) ALGORITHMIC bytes and reports the PMC traffic beside it.
//
// Layered min-sum (ALG_LMSA, no upstream counterpart) keeps the same c2v / marg state but no prior tiles and updates the marginals in place:
// one layer pass per layer of checks (k_layer) and a decision pass (k_decide) instead of the two passes above -- s(4E + n) bytes per frame-sweep.
//
// Reference semantics reproduced (file:line relative to thadikari/ldpc_decoders):
//   flooding loop, max_iter and syndrome exits, x_hat = (marginal < 0) ...... src/bpa.py:17-63
//   iteration-0 check of the received word (BSC) ............................ src/bpa.py:20,29
//   variable update: prior + (((0 + c_a) + c_b) + ...) in ascending edge order  src/bpa.py:35, src/math_utils.py:7
// (The erasure decoder of src/bec.py:83-122 has its own bit-sliced streaming kernels: ldpc_bec_stream.hip.)
#include <hip/hip_fp16.h>

#include <cstdlib>
#include <string>
#include <type_traits>

#include "ldpc_cn.hpp"
#include "ldpc_common.hpp"
#include "ldpc_repack.hpp"
#include "ldpc_rng.hpp"
#include "ldpc_tiles.hpp"

namespace ldpc {

namespace {

// streaming (non-temporal) access, selectable per pass and per direction (measured): the check pass streams
// its c2v lines through with non-temporal loads AND stores so that they do not push the marginal lines (re-used dv times) out of
// the caches
constexpr bool CN_NTL = true, CN_NTS = true, VN_NTL = false, VN_NTS = false;
template <bool NT, typename T> __device__ __forceinline__ T msg_ld(const T* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p); else return *p;
}
template <bool NT, typename T> __device__ __forceinline__ void msg_st(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

// ---------------------------------------------------------------------------------------------------
// priors [B,n] (frame-major, as numpy hands them over) -> prior tile [n][64]; optional hard word y0 -> planes.
template <typename T>
__global__ __launch_bounds__(256) void k_load_tile(const T* __restrict__ priors, const uint8_t* __restrict__ y0, int64_t B,
                                                   int n, T* __restrict__ prior_t, u64* __restrict__ xbits) {
    __shared__ T sp[64][65];
    __shared__ uint8_t sy[64][68];
    const int tile = blockIdx.y, v0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int f = ty; f < 64; f += 4) {
        const int64_t fr = (int64_t)tile * 64 + f;
        const int v = v0 + tx;
        T val = T(0);
        uint8_t yy = 0;
        if (fr < B && v < n) {
            if (y0) yy = y0[fr * n + v];
            val = priors[fr * n + v];
        }
        sp[f][tx] = val;
        sy[f][tx] = yy;
    }
    __syncthreads();
    for (int vv = ty; vv < 64; vv += 4) {
        const int v = v0 + vv;
        if (v < n) {
            prior_t[((int64_t)tile * n + v) * 64 + tx] = sp[tx][vv];
            if (y0) {
                const u64 one = __ballot(sy[tx][vv] != 0);
                if (tx == 0) xbits[plane_at(tile, v, n)] = one;
            }
        }
    }
}

// BI-AWGN channel + LLR written STRAIGHT into the prior tiles (ldpc_simulate on the streaming kernels): the Philox block, Box-Muller and
// LLR expressions of k_biawgn (ldpc_channel.hip; src/biawgn.py:10-28) -- bit-identical priors -- without the [B,n] staging array and the
// transposing tile load.  Lane == frame: one Philox block (4 consecutive variables) per lane and step, four coalesced lines per wave.
struct SimSource {
    double sigma, inv_var2;
    int codeword;
    uint64_t seed, frame0;
    uint32_t stream;
};
template <typename T>
__global__ __launch_bounds__(256) void k_biawgn_tile(SimSource s, int64_t B, int n, int bpf, int blocks_per_wave, T* __restrict__ prior_t) {
    const int lane = threadIdx.x, tile = blockIdx.y;
    const int64_t fr = (int64_t)tile * 64 + lane;
    if (fr >= B) return;
    const int j0 = (blockIdx.x * 4 + threadIdx.y) * blocks_per_wave;
    const T sg = (T)s.sigma, k = (T)s.inv_var2, mean = (T)(2 * s.codeword - 1);
    T* pt = prior_t + (int64_t)tile * n * 64 + lane;
    for (int j = j0; j < min(bpf, j0 + blocks_per_wave); ++j) {
        const Philox4 p = philox_word_block(s.seed, s.stream, s.frame0 + (uint64_t)fr, (uint32_t)j);
        T z[4];
        box_muller<T>(p.w[0], p.w[1], z[0], z[1]);
        box_muller<T>(p.w[2], p.w[3], z[2], z[3]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const T y = mean + sg * z[q];
            if (4 * j + q < n) pt[(int64_t)(4 * j + q) * 64] = -(k * y);  // -2y/sigma^2 with k = 2/sigma^2
        }
    }
}

// Fixed-point min-sum (ALG_QMSA): the decoder's input stage, in place on the prior tiles of the decoder's workspace (never the caller's
// buffer) -- level = clamp(rint(prior * 2^k), -V, +V), ldpc_cn.hpp quantise_prior.  One element per thread; `count` covers whole tiles
// (lanes beyond the batch hold zeros or unread noise).  The fp16-storage mode passes its float2 pair-tiles as 2 * count floats.
template <typename T>
__global__ __launch_bounds__(256) void k_quantise_tile(T* __restrict__ prior_t, int64_t count, T step, T vmax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) prior_t[i] = quantise_prior(prior_t[i], step, vmax);
}
template <typename T>
void launch_quantise(const RuleParams& r, T* prior_t, int64_t count, hipStream_t st) {
    hipLaunchKernelGGL((k_quantise_tile<T>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, prior_t, count, (T)r.step, (T)r.vmax);
}

__global__ void k_init_live(u64* __restrict__ live, int64_t B, int tiles) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tiles) return;
    const int64_t rem = B - (int64_t)t * 64;
    live[t] = rem >= 64 ? ~0ull : (rem <= 0 ? 0ull : ((1ull << rem) - 1ull));
}

// ---------------------------------------------------------------------------------------------------
// Check pass.  One wavefront = (tile, contiguous run of checks); UNR checks are in flight together: UNR*dc old-message lines (a
// stream) and UNR*dc marginal lines (gathers) outstanding per wave.  `src` = the marginals, or the priors in the first sweep, when
// the reference's v2c is the prior itself (src/bpa.py:19) and there is no old message to subtract.
template <typename T, int ALG>
__device__ __forceinline__ T v2c_of(T marg, T c_old) {
    return marg - c_old;  // src/bpa.py:37
}

// GATHER (the frame repack folded into the sweep that follows it, see run()): `tile` is a tile of the DENSE destination tiling; lane j
// reads its old messages and marginals from the (source tile, source lane) of the j-th live frame (srcmap) -- `c2v_in` / `src` are the
// SOURCE set -- and the new messages are stored as whole lines of the destination set `c2v`.  The lanes of a destination tile cover a
// contiguous run of source positions, so every source sector is fetched by one destination tile (two at a run's ends).
template <typename T, int ALG, int DCMAX, int FIXED_DC, int UNR, bool GATHER = false>
__global__ __launch_bounds__(256) void k_cn(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var,
                                            T* __restrict__ c2v, const T* __restrict__ src,
                                            const u64* __restrict__ live, int m, int n, int64_t E, int tiles, int chunks,
                                            int cpw, int first, int xcd_aware, typename last_int_arg<T, ALG>::type freeze_arg,
                                            const T* __restrict__ c2v_in = nullptr, const int32_t* __restrict__ srcmap = nullptr) {
    const int freeze = last_int_arg<T, ALG>::value(freeze_arg);  // (corrected min-sum: scale and offset ride behind it, ldpc_cn.hpp)
    const int lane = threadIdx.x;
    int tile, chunk;
    if (!task_of(tiles, chunks, xcd_aware, &tile, &chunk)) return;
    const u64 lv = live[tile];
    if (lv == 0) return;
    // A tile with a live frame is processed by ALL its lanes: the messages of a frame that has left are never looked at again, and a
    // store that skips some lanes is a partial line -- sub-sector writes, measured 47 % slower passes at 90 % live lanes (n = 64 800:
    // 16.6 against 11.3 ms per check pass, profiles/r05_config5_timeline.txt).  Only a decode that returns the soft output freezes the
    // lanes of departed frames (`freeze`): their marginals must stay those of their own last sweep.
    const bool on = freeze ? (bool)((lv >> lane) & 1ull) : true;
    const bool dense = E * 4 >= (int64_t)m * DCMAX * 3;  // average row length at least three quarters of DCMAX (wave-uniform)
    T* ct = c2v + (int64_t)tile * E * 64 + lane;
    const T* ci = ct;                                    // old messages in
    const T* st = src + (int64_t)tile * n * 64 + lane;
    if constexpr (GATHER) {
        int sm = srcmap[(int64_t)tile * 64 + lane];
        if (sm < 0) sm = srcmap[(int64_t)tile * 64];      // a lane beyond the live frames (tail of the last tile) shadows lane 0: defined values, never looked at
        ci = c2v_in + (int64_t)(sm >> 6) * E * 64 + (sm & 63);
        st = src + (int64_t)(sm >> 6) * n * 64 + (sm & 63);
    }
    const int c_end = min(m, (chunk + 1) * cpw);
    for (int c = chunk * cpw; c < c_end; c += UNR) {
        T v[UNR][DCMAX], o[UNR][DCMAX];
        int k0[UNR], deg[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int cc = c + u;
            if (cc < c_end) {
                if constexpr (FIXED_DC > 0) {
                    k0[u] = cc * FIXED_DC;
                    deg[u] = FIXED_DC;
                } else {
                    k0[u] = row_ptr[cc];
                    deg[u] = row_ptr[cc + 1] - k0[u];
                }
            } else {
                k0[u] = 0;
                deg[u] = 0;
            }
        }
        if (on) {
            // irregular rows, `dense` (most rows nearly DCMAX long): every line is fetched unconditionally (a short row re-reads its
            // last edge, an empty row edge 0) -- a branch per line keeps the loads of a group of checks from being issued together;
            // with widely spread row lengths the branch stays
            if (FIXED_DC > 0 || dense) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
#pragma unroll
                    for (int j = 0; j < DCMAX; ++j) {
                        const int kk = FIXED_DC > 0 ? k0[u] + j : (deg[u] > 0 ? k0[u] + (j < deg[u] ? j : deg[u] - 1) : 0);
                        v[u][j] = st[(int64_t)edge_var[kk] * 64];
                        if (!first) o[u][j] = msg_ld<CN_NTL>(ci + (int64_t)kk * 64);
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
#pragma unroll
                    for (int j = 0; j < DCMAX; ++j) {
                        if (j < deg[u]) {
                            v[u][j] = st[(int64_t)edge_var[k0[u] + j] * 64];
                            if (!first) o[u][j] = msg_ld<CN_NTL>(ci + (int64_t)(k0[u] + j) * 64);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (!first) {
#pragma unroll
                    for (int j = 0; j < DCMAX; ++j) v[u][j] = v2c_of<T, ALG>(v[u][j], o[u][j]);
                }
                cn_rule<T, ALG, DCMAX>(v[u], deg[u], last_int_arg<T, ALG>::correction(freeze_arg), last_int_arg<T, ALG>::cap(freeze_arg));
#pragma unroll
                for (int j = 0; j < DCMAX; ++j) {
                    if (j < deg[u]) msg_st<CN_NTS>(ct + (int64_t)(k0[u] + j) * 64, v[u][j]);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Variable pass: marginal = prior + ordered sum of c2v (c2v is only read) ; decision bit.
// FIXED_DV > 0: every variable has exactly that many edges (edge list of variable v at v * FIXED_DV): no col_ptr loads and no branch
// per line, so the lines of a group of variables are fetched together
// GATHER (second half of the folded repack): messages, marginals and decision words are those of the destination tiling already; the
// priors are still read from the source position of each lane's frame (srcmap) and copied into the destination set on the way.
template <typename T, int ALG, int DVMAX, int UNR, int FIXED_DV, bool GATHER = false>
__global__ __launch_bounds__(256) void k_vn(const int32_t* __restrict__ col_ptr, const int32_t* __restrict__ col_edge,
                                            const T* __restrict__ c2v, const T* __restrict__ prior_t, T* __restrict__ marg_t,
                                            const u64* __restrict__ live, u64* __restrict__ xbits,
                                            int n, int64_t E, int tiles, int chunks, int vpw, int xcd_aware, int freeze,
                                            T* __restrict__ prior_out = nullptr, const int32_t* __restrict__ srcmap = nullptr) {
    const int lane = threadIdx.x;
    int tile, chunk;
    if (!task_of(tiles, chunks, xcd_aware, &tile, &chunk)) return;
    const u64 lv = live[tile];
    if (lv == 0) return;
    const bool on = freeze ? (bool)((lv >> lane) & 1ull) : true;  // (see k_cn; the decision words below keep the bits of departed frames either way)
    const T* ct = c2v + (int64_t)tile * E * 64 + lane;
    const T* pt = prior_t + (int64_t)tile * n * 64 + lane;
    T* po = nullptr;
    if constexpr (GATHER) {
        int sm = srcmap[(int64_t)tile * 64 + lane];
        if (sm < 0) sm = srcmap[(int64_t)tile * 64];
        pt = prior_t + (int64_t)(sm >> 6) * n * 64 + (sm & 63);
        po = prior_out + (int64_t)tile * n * 64 + lane;
    }
    T* mt = marg_t + (int64_t)tile * n * 64 + lane;
    u64* xb = xbits + plane_at(tile, 0, n);  // word of variable v at xb[8 * v]
    const int v_end = min(n, (chunk + 1) * vpw);
    for (int vbase = chunk * vpw; vbase < v_end; vbase += UNR) {
        T c[UNR][DVMAX];
        T pr[UNR];
        u64 old[UNR];
        int p0[UNR], deg[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int vv = vbase + u;
            // decisions of frames that have left, read ahead of the lines (a read behind this variable's marginal store would wait for it)
            if (lv != ~0ull) old[u] = GATHER ? 0ull : uniform_ld64(xb + 8 * (vv < v_end ? vv : v_end - 1));  // (GATHER: the destination words hold nothing yet)
            if constexpr (FIXED_DV > 0) {
                p0[u] = (vv < v_end ? vv : v_end - 1) * FIXED_DV;  // past the end: the last variable's lines once more, result unused
                deg[u] = vv < v_end ? FIXED_DV : -1;
            } else if (vv < v_end) {
                p0[u] = col_ptr[vv];
                deg[u] = col_ptr[vv + 1] - p0[u];
            } else {
                p0[u] = 0;
                deg[u] = -1;
            }
        }
        if (on) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if constexpr (FIXED_DV > 0) {
                    pr[u] = pt[(int64_t)(vbase + u < v_end ? vbase + u : v_end - 1) * 64];
#pragma unroll
                    for (int j = 0; j < FIXED_DV; ++j) c[u][j] = msg_ld<VN_NTL>(ct + (int64_t)col_edge[p0[u] + j] * 64);
                } else {
                    if (deg[u] >= 0) pr[u] = pt[(int64_t)(vbase + u) * 64];
#pragma unroll
                    for (int j = 0; j < DVMAX; ++j) {
                        if (j < deg[u]) c[u][j] = msg_ld<VN_NTL>(ct + (int64_t)col_edge[p0[u] + j] * 64);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (deg[u] < 0) continue;  // wave-uniform
            const int du = FIXED_DV > 0 ? FIXED_DV : deg[u];
            bool b_one = false;
            if (on) {
                T s = T(0);
#pragma unroll
                for (int j = 0; j < DVMAX; ++j)
                    if (j < du) s += c[u][j];
                const T marg = pr[u] + s;
                msg_st<VN_NTS>(mt + (int64_t)(vbase + u) * 64, marg);
                if constexpr (GATHER) po[(int64_t)(vbase + u) * 64] = pr[u];
                b_one = marg < T(0);  // NaN marginal -> 0 (src/bpa.py:38,62)
            }
            const u64 one = __ballot(b_one);
            const int vv = vbase + u;
            u64 merged = one;
            if (lv != ~0ull) merged = (old[u] & ~lv) | (one & lv);
            if (lane == 0) xb[8 * vv] = merged;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Layered min-sum (ALG_LMSA; the contract is in include/ldpc_hip.h).  The state is the flooding state -- c2v[tile][E][64] and
// marg[tile][n][64], lane == frame -- but the marginals are updated IN PLACE, check by check: v = marg - c2v_old, the corrected min-sum
// rule on the row, c2v = the new message, marg = v + c2v.  The checks of one LAYER share no variable, so they touch disjoint marginal rows
// and run in any order and in parallel: one launch per layer, the launches ordered on the stream.  A wave takes (tile, run of the layer's
// checks) out of `order`, the checks sorted by (layer, index); `c0` .. `c1` is the layer's range in that list.  UNR checks are in flight
// together (all of one layer, hence independent).  Per edge: one marginal row and one message row read, one each written.  FIRST: the
// first sweep, where every old message is +0 and x - (+0) == x bit for bit: nothing is read.  `freeze` as in k_cn: a soft-output decode
// keeps the marginals of a frame that has left.
template <typename T, int DCMAX, int FIXED_DC, int UNR, bool FIRST>
__global__ __launch_bounds__(256) void k_layer(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var,
                                               const int32_t* __restrict__ order, T* c2v, T* marg, const u64* __restrict__ live, int m, int n,
                                               int64_t E, int tiles, int chunks, int cpw, int c0, int c1, int xcd_aware, int freeze, T scale,
                                               T offset) {
    const int lane = threadIdx.x;
    int tile, chunk;
    if (!task_of(tiles, chunks, xcd_aware, &tile, &chunk)) return;
    const u64 lv = live[tile];
    if (lv == 0) return;
    const bool on = freeze ? (bool)((lv >> lane) & 1ull) : true;
    if (!on) return;  // (no wave-wide operation below)
    // irregular rows: as in k_cn, where most rows are nearly DCMAX long every line is fetched unconditionally (a short row re-reads its
    // last edge) -- a branch per line keeps the loads of a group of checks from being issued together
    // (degree classes up to 8, the ensembles this form was measured on; both forms in one kernel cost the wide classes their registers)
    const bool dense = FIXED_DC > 0 || (DCMAX <= 8 && E * 4 >= (int64_t)m * DCMAX * 3);  // (wave-uniform)
    T* ct = c2v + (int64_t)tile * E * 64 + lane;
    T* mt = marg + (int64_t)tile * n * 64 + lane;
    const int i_end = min(c1, c0 + (chunk + 1) * cpw);
    for (int i = c0 + chunk * cpw; i < i_end; i += UNR) {
        T v[UNR][DCMAX], w[UNR][DCMAX];
        int k0[UNR], deg[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (i + u < i_end) {
                const int cc = order[i + u];
                k0[u] = FIXED_DC > 0 ? cc * FIXED_DC : row_ptr[cc];
                deg[u] = FIXED_DC > 0 ? FIXED_DC : row_ptr[cc + 1] - k0[u];
            } else {
                k0[u] = 0;
                deg[u] = 0;
            }
        }
        if (dense) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
#pragma unroll
                for (int j = 0; j < DCMAX; ++j) {
                    const int kk = FIXED_DC > 0 ? k0[u] + j : (deg[u] > 0 ? k0[u] + (j < deg[u] ? j : deg[u] - 1) : 0);
                    v[u][j] = mt[(int64_t)edge_var[kk] * 64];
                    if constexpr (!FIRST) w[u][j] = msg_ld<CN_NTL>(ct + (int64_t)kk * 64);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
#pragma unroll
                for (int j = 0; j < DCMAX; ++j) {
                    if (j < deg[u]) {
                        v[u][j] = mt[(int64_t)edge_var[k0[u] + j] * 64];
                        if constexpr (!FIRST) w[u][j] = msg_ld<CN_NTL>(ct + (int64_t)(k0[u] + j) * 64);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
#pragma unroll
            for (int j = 0; j < DCMAX; ++j) {
                if constexpr (!FIRST) v[u][j] = v[u][j] - w[u][j];
                w[u][j] = v[u][j];
            }
            cn_msa<T, DCMAX, MSA_CORRECTED>(w[u], deg[u], Correction<T>{scale, offset});
#pragma unroll
            for (int j = 0; j < DCMAX; ++j) {
                if (j < deg[u]) {
                    msg_st<CN_NTS>(ct + (int64_t)(k0[u] + j) * 64, w[u][j]);
                    mt[(int64_t)edge_var[k0[u] + j] * 64] = v[u][j] + w[u][j];
                }
            }
        }
    }
}

// Decision pass of the layered decoder: marginals -> decision bit planes, behind the last layer of a sweep.  The words keep the bits of the
// frames that have left (as k_vn's do).
template <typename T>
__global__ __launch_bounds__(256) void k_decide(const T* __restrict__ marg, const u64* __restrict__ live, u64* __restrict__ xbits, int n, int tiles,
                                                int chunks, int vpw, int xcd_aware) {
    const int lane = threadIdx.x;
    int tile, chunk;
    if (!task_of(tiles, chunks, xcd_aware, &tile, &chunk)) return;
    const u64 lv = live[tile];
    if (lv == 0) return;
    const T* mt = marg + (int64_t)tile * n * 64 + lane;
    u64* xb = xbits + plane_at(tile, 0, n);  // word of variable v at xb[8 * v]
    const int v_end = min(n, (chunk + 1) * vpw);
    for (int v = chunk * vpw; v < v_end; ++v) {
        const u64 one = __ballot(mt[(int64_t)v * 64] < T(0));  // NaN marginal -> 0, as k_vn
        u64 merged = one;
        if (lv != ~0ull) merged = (uniform_ld64(xb + 8 * v) & ~lv) | (one & lv);
        if (lane == 0) xb[8 * v] = merged;
    }
}

// soft output of the layered decoder: the marginal tiles start as the priors, so a frame that never swept (iters == 0: it left at the
// iteration-0 check) reports 0 as it does everywhere else
template <typename T>
__global__ void k_soft_out_swept(const T* __restrict__ soft_t, const int32_t* __restrict__ iters, T* __restrict__ out, int64_t B, int n) {
    const int tile = blockIdx.y, lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t fr = (int64_t)tile * 64 + lane;
    if (v < n && fr < B) out[fr * n + v] = iters[fr] > 0 ? soft_t[((int64_t)tile * n + v) * 64 + lane] : T(0);
}

// ---------------------------------------------------------------------------------------------------
// Syndrome of the current hard decisions; frames whose syndrome is zero leave (iters = sweeps run so far).
// Two kernels: k_syndrome_part -- a block takes a GROUP of eight tiles and a chunk of the checks; a thread fetches, per edge of its
// check, the one 64-byte sector that holds the decision words of the variable for all eight tiles (per-tile 8-byte gathers made this
// kernel L2-bound: 0.92 ms per sweep at n = 64 800, 6 % of the sweep), XORs them into eight parities, and the block merges the OR of
// its checks into the tiles' words -- and k_syndrome_fin, one wave per tile, which retires the frames.
__global__ __launch_bounds__(256) void k_syndrome_part(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var,
                                                       const u64* __restrict__ xbits, const u64* __restrict__ live,
                                                       u64* __restrict__ unsat_acc, int m, int n, int tiles, int checks_per_block) {
    const int grp = blockIdx.y, t = threadIdx.x;
    const int t0 = grp * 8, nt = min(8, tiles - t0);
    u64 any_live = 0;
    for (int i = 0; i < nt; ++i) any_live |= live[t0 + i];
    if (any_live == 0) return;
    const ulonglong2* xb = reinterpret_cast<const ulonglong2*>(xbits + (int64_t)grp * n * 8);  // variable v: xb[4 v .. 4 v + 3]
    const int c0 = blockIdx.x * checks_per_block, c1 = min(m, c0 + checks_per_block);
    u64 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = c0 + t; c < c1; c += 256) {
        u64 par[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = row_ptr[c]; k < row_ptr[c + 1]; ++k) {
            const ulonglong2* w = xb + (int64_t)edge_var[k] * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const ulonglong2 x = w[q];
                par[2 * q] ^= x.x;
                par[2 * q + 1] ^= x.y;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] |= par[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u64 a = wave_or(acc[i]);
        if ((t & 63) == 0 && a && i < nt) atomicOr(&unsat_acc[2 * (t0 + i)], a);
    }
}

__global__ __launch_bounds__(64) void k_syndrome_fin(u64* __restrict__ unsat_acc, u64* __restrict__ live, int32_t* __restrict__ iters,
                                                     int* __restrict__ live_tiles, int64_t B, int sweeps,
                                                     const int32_t* __restrict__ frame_of) {
    const int tile = blockIdx.x, t = threadIdx.x;
    const u64 lv = live[tile];
    if (lv == 0) return;
    const u64 unsat = unsat_acc[2 * tile];
    const u64 stay = lv & unsat, leave = lv & ~unsat;
    __syncthreads();  // every lane has read the word before lane 0 clears it for the next sweep
    if (t == 0) {
        unsat_acc[2 * tile] = 0;
        live[tile] = stay;
        if (stay && live_tiles) {
            atomicAdd(live_tiles, 1);                    // tiles that still hold a live frame
            atomicAdd(live_tiles + 1, __popcll(stay));   // live frames
        }
    }
    if ((leave >> t) & 1ull) {
        const int64_t fr = frame_of ? (int64_t)frame_of[(int64_t)tile * 64 + t] : (int64_t)tile * 64 + t;
        if (fr >= 0 && fr < B) iters[fr] = sweeps;
    }
}

// ---------------------------------------------------------------------------------------------------
// Frame repack (early termination, ldpc_repack.hpp): when many tiles hold only a few live frames, the live frames are gathered
// into dense tiles.  k_repack moves
// message lines, marginals, priors and decision bit-planes: destination lane j reads (source tile, source lane) of the j-th live
// frame; lanes that share a source tile share the 256-byte line, so a line of a source tile is fetched once per destination tile
// that draws from it.  The decisions of every frame of the old tiles are written out before (k_unpack), the moved frames
// overwrite theirs at the end.
// (PRIOR false: the layered decoder keeps no prior tiles)
template <typename T, bool PRIOR = true>
__global__ __launch_bounds__(256) void k_repack(const T* __restrict__ msg_src, T* __restrict__ msg_dst, const T* __restrict__ marg_src,
                                                T* __restrict__ marg_dst, const T* __restrict__ prior_src, T* __restrict__ prior_dst,
                                                const u64* __restrict__ xb_src, u64* __restrict__ xb_dst,
                                                const u64* __restrict__ live_src, u64* __restrict__ live_dst,
                                                const int32_t* __restrict__ base, const int32_t* __restrict__ frame_src,
                                                int32_t* __restrict__ frame_dst, int tiles_src, int n, int64_t E, int rows_per_wave) {
    const int lane = threadIdx.x;
    const int dt = blockIdx.y;  // destination tile
    int st, sl;
    const bool has = repack_source(base, live_src, tiles_src, dt * 64 + lane, &st, &sl);
    const int chunk = blockIdx.x * 4 + threadIdx.y;
    const int64_t rows = E + n;  // message lines, then per variable: marginal + prior line + one bit-plane word
    const int64_t r0 = (int64_t)chunk * rows_per_wave, r1 = min(rows, r0 + rows_per_wave);
    const T* ms = msg_src + (int64_t)st * E * 64 + sl;
    T* md = msg_dst + (int64_t)dt * E * 64 + lane;
    const int64_t so = (int64_t)st * n * 64 + sl, dof = (int64_t)dt * n * 64 + lane;
    for (int64_t r = r0; r < r1; ++r) {
        // lanes beyond the live frames (the tail of the last destination tile) get zeros, not whatever the buffer held: every lane of a
        // live tile computes and stores in the passes that follow, and whole-line stores are the cheaper ones anyway
        if (r < E) {
            md[r * 64] = has ? ms[r * 64] : T(0);
        } else {
            const int64_t v = r - E;
            if constexpr (PRIOR) prior_dst[dof + v * 64] = has ? prior_src[so + v * 64] : T(0);
            marg_dst[dof + v * 64] = has ? marg_src[so + v * 64] : T(0);
            const u64 w = has ? xb_src[plane_at(st, v, n)] : 0ull;
            const u64 plane = __ballot(has && ((w >> sl) & 1ull));
            if (lane == 0) xb_dst[plane_at(dt, v, n)] = plane;
        }
    }
    if (chunk == 0) {
        frame_dst[(int64_t)dt * 64 + lane] = has ? (frame_src ? frame_src[(int64_t)st * 64 + sl] : st * 64 + sl) : -1;
        const u64 lv = __ballot(has);
        if (lane == 0) live_dst[dt] = lv;
    }
}

// The repack FOLDED into the next sweep (LLR decoders, node degrees up to 8): instead of copying E + 2n lines per tile, only the map is
// built -- srcmap[dt][lane] = source tile * 64 + source lane of the frame that destination lane will hold (-1 beyond the live frames),
// the frame indices and the live words of the destination tiling -- and the sweep that follows runs the GATHER variants of the two passes:
// they read the old state through the map and write the new state densely into the other buffer set.  A separate repack read all of the
// source and wrote the live part (13.7 ms at n = 64 800 / 59 % live) before a sweep that read and wrote the live part again; folded, the
// sweep reads the source once and writes the live part once.
__global__ __launch_bounds__(64) void k_repack_map(const u64* __restrict__ live_src, u64* __restrict__ live_dst, const int32_t* __restrict__ base,
                                                   const int32_t* __restrict__ frame_src, int32_t* __restrict__ frame_dst,
                                                   int32_t* __restrict__ srcmap, int tiles_src) {
    const int lane = threadIdx.x, dt = blockIdx.x;
    int st, sl;
    const bool has = repack_source(base, live_src, tiles_src, dt * 64 + lane, &st, &sl);
    srcmap[(int64_t)dt * 64 + lane] = has ? st * 64 + sl : -1;
    frame_dst[(int64_t)dt * 64 + lane] = has ? (frame_src ? frame_src[(int64_t)st * 64 + sl] : st * 64 + sl) : -1;
    const u64 lv = __ballot(has);
    if (lane == 0) live_dst[dt] = lv;
}

// Frames that hit max_iter: iters = sweeps ; then planes -> x_hat bytes [B,n] in {0,1}.
__global__ void k_finish_iters(const u64* __restrict__ live, int32_t* __restrict__ iters, int64_t B, int sweeps,
                               const int32_t* __restrict__ frame_of) {
    const int tile = blockIdx.x, t = threadIdx.x;
    const u64 lv = live[tile];
    const int64_t fr = frame_of ? (int64_t)frame_of[(int64_t)tile * 64 + t] : (int64_t)tile * 64 + t;
    if (((lv >> t) & 1ull) && fr >= 0 && fr < B) iters[fr] = sweeps;
}

// marginal tile [n][64] -> [B,n] (diagnostic / soft-output path; not on the throughput path)
template <typename T>
__global__ void k_soft_out(const T* __restrict__ soft_t, T* __restrict__ out, int64_t B, int n) {
    const int tile = blockIdx.y, lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t fr = (int64_t)tile * 64 + lane;
    if (v < n && fr < B) out[fr * n + v] = soft_t[((int64_t)tile * n + v) * 64 + lane];
}

__global__ __launch_bounds__(256) void k_unpack(const u64* __restrict__ xbits, uint8_t* __restrict__ xhat, int64_t B, int n,
                                                const int32_t* __restrict__ frame_of) {
    const int tile = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const u64 one = xbits[plane_at(tile, v, n)];
    const int64_t f0 = (int64_t)tile * 64;
    if (frame_of) {  // repacked tiles: lane f holds frame frame_of[tile][f] (-1: none)
        for (int f = 0; f < 64; ++f) {
            const int64_t fr = frame_of[f0 + f];
            if (fr >= 0 && fr < B) xhat[fr * n + v] = (uint8_t)((one >> f) & 1ull);
        }
        return;
    }
    const int fmax = (int)min((int64_t)64, B - f0);
    for (int f = 0; f < fmax; ++f) xhat[(f0 + f) * n + v] = (uint8_t)((one >> f) & 1ull);
}

// planes -> PACKED decisions [B, W] u32 (bit v & 31 of word v >> 5 = decision of variable v; W = ceil(n / 32)): the form
// ldpc_decode_bits returns (SURVEY 8(a2) "packed x_hat bits").  One wave per (tile, 64 variables): the 64 x 64 bit block is
// transposed with 64 ballots (lane = variable on the way in, lane = frame on the way out).
__global__ __launch_bounds__(256) void k_unpack_bits(const u64* __restrict__ xbits, uint32_t* __restrict__ bits, int64_t B, int n, int W,
                                                     const int32_t* __restrict__ frame_of) {
    const int tile = blockIdx.y, lane = threadIdx.x;
    const int vb = blockIdx.x * 4 + threadIdx.y, v0 = vb * 64;
    if (v0 >= n) return;
    const u64 col = v0 + lane < n ? xbits[plane_at(tile, v0 + lane, n)] : 0ull;
    u64 row = 0;
    for (int f = 0; f < 64; ++f) {
        const u64 b = __ballot((col >> f) & 1ull);
        if (lane == f) row = b;
    }
    const int64_t fr = frame_of ? (int64_t)frame_of[(int64_t)tile * 64 + lane] : (int64_t)tile * 64 + lane;
    if (fr >= 0 && fr < B) {
        uint32_t* out = bits + fr * W + 2 * vb;
        out[0] = (uint32_t)row;
        if (2 * vb + 1 < W) out[1] = (uint32_t)(row >> 32);
    }
}

}  // namespace

// The launchers of the bookkeeping kernels above (ldpc_tiles.hpp), for this file's loops and SLQMSA's (ldpc_slq.hip).
void tiles_init_live(u64* live, int64_t B, int tiles, hipStream_t st) {
    hipLaunchKernelGGL(k_init_live, dim3((tiles + 255) / 256), dim3(256), 0, st, live, B, tiles);
}

void tiles_syndrome(const Code* c, const u64* xbits, u64* live, u64* tflags, int32_t* iters, int* poll_dev, int64_t B, int tiles, int sweeps,
                    const int32_t* fmap, hipStream_t st) {
    // groups of eight tiles x chunks of the checks: enough blocks to fill the chip (about 4 per CU), at least 1024 checks each
    const int groups = (tiles + 7) / 8;
    int sblocks = (1024 + groups - 1) / groups;
    const int smax = (c->m + 1023) / 1024;
    sblocks = sblocks < 1 ? 1 : (sblocks > smax ? smax : sblocks);
    const int cpb = (c->m + sblocks - 1) / sblocks;
    hipLaunchKernelGGL(k_syndrome_part, dim3(sblocks, groups), dim3(256), 0, st, c->d_row_ptr, c->d_edge_var, xbits, live, tflags, c->m, c->n, tiles, cpb);
    hipLaunchKernelGGL(k_syndrome_fin, dim3(tiles), dim3(64), 0, st, tflags, live, iters, poll_dev, B, sweeps, fmap);
}

void tiles_unpack(const u64* xbits, uint8_t* xhat, uint32_t* bits, int64_t B, int n, int tiles, const int32_t* fmap, hipStream_t st) {
    if (bits) hipLaunchKernelGGL(k_unpack_bits, dim3(((n + 63) / 64 + 3) / 4, tiles), dim3(64, 4), 0, st, xbits, bits, B, n, (n + 31) / 32, fmap);
    if (xhat) hipLaunchKernelGGL(k_unpack, dim3((n + 255) / 256, tiles), dim3(256), 0, st, xbits, xhat, B, n, fmap);
}

void tiles_finish_iters(const u64* live, int32_t* iters, int64_t B, int tiles, int sweeps, const int32_t* fmap, hipStream_t st) {
    hipLaunchKernelGGL(k_finish_iters, dim3(tiles), dim3(64), 0, st, live, iters, B, sweeps, fmap);
}

namespace {

// decisions in the form the caller asked for: packed words (ldpc_decode_bits) if set, else bytes [B,n] (ldpc_decode)
void launch_unpack(const DecodeCall& k, const u64* xbits, int n, int tiles, const int32_t* fmap) {
    tiles_unpack(xbits, k.bits ? nullptr : k.xhat, k.bits, k.B, n, tiles, fmap, k.stream);
}

// what every LLR decode ends with: iteration counts of the frames still live, decisions in the form the caller asked for
void launch_decisions(const DecodeCall& k, const u64* xbits, const u64* live, int n, int tiles, int sweeps, const int32_t* fmap) {
    tiles_finish_iters(live, k.iters, k.B, tiles, sweeps, fmap, k.stream);
    launch_unpack(k, xbits, n, tiles, fmap);
}

bool degrees_supported(const Code* c) {
    if (c->max_dc <= 64 && c->max_dv <= 64) return true;
    set_error("streaming backend supports node degrees up to 64 (max_dc=%d, max_dv=%d)", c->max_dc, c->max_dv);
    return false;
}

// Per-kernel timing of a decode when Decoder::profile is set (no-ops otherwise): event pairs around the two passes of every sweep
// (kinds 0 and 1) and, optionally, around the whole decode (kind 3).  `next`: first free entry of the decoder's event pool.
struct DecodeProf {
    Decoder* d;
    hipStream_t st;
    size_t next;
    hipEvent_t e[3] = {}, whole[2] = {};
    std::vector<ProfSpan> spans = {};
    int begin_decode() {
        if (!d->profile) return LDPC_OK;
        for (hipEvent_t& x : whole) LDPC_TRY(prof_event(d, next++, &x));
        LDPC_HIP_TRY(hipEventRecord(whole[0], st));
        return LDPC_OK;
    }
    int mark(int i) {  // 0: a sweep begins, 1: between its passes, 2: behind it
        if (!d->profile) return LDPC_OK;
        if (i == 0)
            for (hipEvent_t& x : e) LDPC_TRY(prof_event(d, next++, &x));
        LDPC_HIP_TRY(hipEventRecord(e[i], st));
        if (i == 2) spans.insert(spans.end(), {{0, e[0], e[1]}, {1, e[1], e[2]}});
        return LDPC_OK;
    }
    int collect() {
        if (!d->profile) return LDPC_OK;
        if (whole[0]) LDPC_HIP_TRY(hipEventRecord(whole[1], st));
        LDPC_HIP_TRY(hipStreamSynchronize(st));
        LDPC_TRY(prof_collect(d, spans));
        if (whole[0]) LDPC_TRY(prof_collect(d, {{3, whole[0], whole[1]}}));  // everything the decode enqueued: the two passes + load, syndrome, repack, unpack kernels
        return LDPC_OK;
    }
};

// the host side of every LLR decode ends here: launch errors, profile, statistics of the call
int end_decode(Decoder* d, DecodeProf& prof, int sweeps, int repacks) {
    LDPC_HIP_TRY(hipGetLastError());
    LDPC_TRY(prof.collect());
    d->last_repacks = repacks;
    d->last_sweeps = sweeps;
    d->last_backend = BK_STREAM;
    return LDPC_OK;
}

int pick_pow2_ge(int x, int lo, int hi) {
    int p = lo;
    while (p < x && p < hi) p <<= 1;
    return p;
}

// Degree classes of the pass kernels, handed to f as std::integral_constants (f is a generic lambda that launches the instantiation).
template <int V>
using int_c = std::integral_constant<int, V>;
template <class F>
void pow2_class(int deg, F&& f) {
    switch (pick_pow2_ge(deg, 4, 64)) {
        case 4: return f(int_c<4>{}, int_c<0>{});
        case 8: return f(int_c<8>{}, int_c<0>{});
        case 16: return f(int_c<16>{}, int_c<0>{});
        case 32: return f(int_c<32>{}, int_c<0>{});
        default: return f(int_c<64>{}, int_c<0>{});
    }
}
// checks -> f(DCMAX, FIXED_DC): regular dc = 6; degrees up to 6 (the rho = x^5 ensembles: no lines fetched for positions that never
// exist); else the next power of two
template <class F>
void check_class(const Code* c, F&& f) {
    if (c->min_dc == c->max_dc && c->max_dc == 6) return f(int_c<6>{}, int_c<6>{});
    if (c->max_dc > 4 && c->max_dc <= 6) return f(int_c<6>{}, int_c<0>{});
    pow2_class(c->max_dc, f);
}
// variables -> f(DVMAX, FIXED_DV): (3, r)-regular codes; regular dv = 4 where the pass has that form (FIXED4); else the next power of two
template <bool FIXED4, class F>
void var_class(const Code* c, F&& f) {
    const bool regular = c->min_dv == c->max_dv;
    if (regular && c->max_dv == 3) return f(int_c<3>{}, int_c<3>{});
    if constexpr (FIXED4)
        if (regular && c->max_dv == 4) return f(int_c<4>{}, int_c<4>{});
    pow2_class(c->max_dv, f);
}

// nodes kept in flight per wave: about 32 VGPRs (128 bytes per lane) of messages, at most 4 nodes
constexpr int unroll_for(int row_bytes) {
    int u = 128 / row_bytes;
    u = u > 4 ? 4 : u;
    return u >= 8 ? 8 : (u >= 4 ? 4 : (u >= 2 ? 2 : 1));
}

struct Geometry {
    int tiles, cn_chunks, cpw, vn_chunks, vpw, xcd_aware;
    int freeze = 0;  // lanes of departed frames do not compute or store (soft-output decodes)
    RuleParams rule;  // of the check rule, at the time of the call
};

// The two passes.  GATHER (c2v_in / prior_out + srcmap): the sweep that carries a folded repack; those forms are built for the node
// degrees the LDPC ensembles of the reference have (dc <= 8, dv <= 8).
inline bool gather_passes_built(const Code* c) { return c->max_dc <= 8 && c->max_dv <= 8; }
template <typename T, int ALG, bool GATHER = false>
void dispatch_cn(const Code* c, T* c2v, const T* src, const u64* live, const Geometry& g, int first, hipStream_t st, const T* c2v_in = nullptr,
                 const int32_t* srcmap = nullptr) {
    check_class(c, [&](auto dcm, auto fdc) {
        constexpr int DCMAX = decltype(dcm)::value, UNR = unroll_for(2 * DCMAX * (int)sizeof(T));  // old message + marginal line per edge
        if constexpr (!GATHER || DCMAX <= 8)
            hipLaunchKernelGGL((k_cn<T, ALG, DCMAX, decltype(fdc)::value, UNR, GATHER>), dim3(task_blocks(g.tiles, g.cn_chunks, g.xcd_aware)), dim3(64, 4), 0, st,
                               c->d_row_ptr, c->d_edge_var, c2v, src, live, c->m, c->n, c->E, g.tiles, g.cn_chunks, g.cpw, first, g.xcd_aware,
                               last_int_arg<T, ALG>::make(g.freeze, g.rule), c2v_in, srcmap);
    });
}
template <typename T, int ALG, bool GATHER = false>
void dispatch_vn(const Code* c, const T* c2v, const T* prior, T* marg, const u64* live, u64* xbits, const Geometry& g, hipStream_t st, T* prior_out = nullptr,
                 const int32_t* srcmap = nullptr) {
    var_class<true>(c, [&](auto dvm, auto fdv) {
        constexpr int DVMAX = decltype(dvm)::value, UNR = unroll_for((DVMAX + 1) * (int)sizeof(T));
        // (the variable pass does not depend on the check rule: corrected min-sum launches the min-sum instantiations)
        if constexpr (!GATHER || DVMAX <= 8)
            hipLaunchKernelGGL((k_vn<T, alg_family(ALG), DVMAX, UNR, decltype(fdv)::value, GATHER>), dim3(task_blocks(g.tiles, g.vn_chunks, g.xcd_aware)), dim3(64, 4), 0, st,
                               c->d_col_ptr, c->d_col_edge, c2v, prior, marg, live, xbits, c->n, c->E, g.tiles, g.vn_chunks, g.vpw, g.xcd_aware, g.freeze, prior_out, srcmap);
    });
}

// The layered sweep (ALG_LMSA): one layer pass per layer, in order on the stream, then the decision pass.  Degree classes of dispatch_cn.
template <typename T>
void dispatch_layers(const Decoder* d, T* c2v, T* marg, const u64* live, const Geometry& g, bool first, hipStream_t st) {
    const Code* c = d->code;
    check_class(c, [&](auto dcm, auto fdc) {
        constexpr int DCMAX = decltype(dcm)::value, FDC = decltype(fdc)::value, UNR = unroll_for(2 * DCMAX * (int)sizeof(T));
        const auto kern = first ? k_layer<T, DCMAX, FDC, UNR, true> : k_layer<T, DCMAX, FDC, UNR, false>;
        for (size_t l = 0; l + 1 < d->layer_start.size(); ++l) {
            const int c0 = d->layer_start[l], c1 = d->layer_start[l + 1];
            const int chunks = (c1 - c0 + g.cpw - 1) / g.cpw;
            hipLaunchKernelGGL(kern, dim3(task_blocks(g.tiles, chunks, g.xcd_aware)), dim3(64, 4), 0, st, c->d_row_ptr, c->d_edge_var,
                               (const int32_t*)d->layer_order.p, c2v, marg, live, c->m, c->n, c->E, g.tiles, chunks, g.cpw, c0, c1, g.xcd_aware, g.freeze,
                               (T)g.rule.scale, (T)g.rule.offset);
        }
    });
}
template <typename T>
void dispatch_decide(const Code* c, const T* marg, const u64* live, u64* xbits, const Geometry& g, hipStream_t st) {
    hipLaunchKernelGGL((k_decide<T>), dim3(task_blocks(g.tiles, g.vn_chunks, g.xcd_aware)), dim3(64, 4), 0, st, marg, live, xbits, c->n, g.tiles, g.vn_chunks, g.vpw,
                       g.xcd_aware);
}

int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e && *e ? atoi(e) : dflt;
}

template <typename T, int ALG>
int run(Decoder* d, const DecodeCall& k, const SimSource* sim = nullptr) {
    const Code* c = d->code;
    const int n = c->n, m = c->m;
    const int64_t E = c->E, B = k.B;
    const int32_t max_iter = k.max_iter;
    const uint8_t* const y0 = k.y0;
    int32_t* const iters = k.iters;
    const hipStream_t st = k.stream;
    const int tiles = (int)((B + 63) / 64);
    if (!degrees_supported(c)) return LDPC_E_UNSUPPORTED;
    // layered min-sum: the marginal tiles start as the priors and are updated in place -- no prior tiles, no variable pass
    constexpr bool LAYERED = ALG == ALG_LMSA;
    const bool early = !(k.flags & FLAG_NO_EARLY_EXIT);
    RepackPolicy repack(early && k.soft == nullptr && tiles >= 2);

    // every buffer of the decode is reserved here, before the first sweep (no allocation -- a device synchronisation -- in the loop)
    TileSet* const set = d->set;
    LDPC_TRY(set[0].edge.reserve((size_t)tiles * E * 64 * sizeof(T)));
    LDPC_TRY(set[0].node.reserve((size_t)tiles * n * 64 * sizeof(T)));
    if (!LAYERED) LDPC_TRY(set[0].prior.reserve((size_t)tiles * n * 64 * sizeof(T)));
    LDPC_TRY(set[0].planes.reserve(plane_words(tiles, n) * 8));
    LDPC_TRY(set[0].live.reserve((size_t)tiles * 8));
    LDPC_TRY(d->flags.reserve((size_t)tiles * 16 + 64 + POLL_RING_BYTES));
    if (repack.on) {
        // second state set: the first repack fires at <= fill * 64 live frames per tile, later ones only shrink
        const size_t nt = repack.target_tiles(tiles);
        if (set[1].edge.reserve(nt * E * 64 * sizeof(T)) || set[1].node.reserve(nt * n * 64 * sizeof(T)) ||
            (!LAYERED && set[1].prior.reserve(nt * n * 64 * sizeof(T))) || set[1].planes.reserve(plane_words((int)nt, n) * 8) || set[1].live.reserve(nt * 8) ||
            set[1].fmap.reserve(nt * 64 * sizeof(int32_t)) || set[0].fmap.reserve(nt * 64 * sizeof(int32_t)) ||
            d->rbase.reserve(((size_t)tiles + 1) * sizeof(int32_t)) || d->rmap.reserve(nt * 64 * sizeof(int32_t)))
            repack.on = false;  // no room for a second set: decode without repacking
    }
    // the repack folded into the sweep behind it (k_repack_map + GATHER passes) where those passes are built; LDPC_STREAM_REPACK_FOLD=0: the
    // separate copy kernel (k_repack), kept for the degrees beyond and as the A/B reference
    // (the layered decoder has no GATHER passes: its repack is the copy kernel, without the priors)
    const bool fold_repack = !LAYERED && gather_passes_built(c) && env_int("LDPC_STREAM_REPACK_FOLD", 1) != 0;
    int cur = 0;  // which set holds the state; the pointers below are re-read from it after a flip
    T *msg, *marg, *prior;
    u64 *xbits, *live;
    int32_t* fmap = nullptr;  // frame index of (tile, lane); null = identity (never repacked)
    auto use_set = [&](int s) {
        cur = s;
        msg = (T*)set[s].edge.p;
        marg = (T*)set[s].node.p;
        prior = (T*)set[s].prior.p;
        xbits = (u64*)set[s].planes.p;
        live = (u64*)set[s].live.p;
    };
    use_set(0);
    u64* tflags = (u64*)d->flags.p;  // [tiles][2], the device poll ring behind them
    hipEvent_t poll_ev[POLL_RING];
    for (int i = 0; i < POLL_RING; ++i) LDPC_TRY(prof_event(d, i, &poll_ev[i]));
    DecodeProf prof{d, st, POLL_RING};

    Geometry g;
    g.tiles = tiles;
    g.freeze = k.soft != nullptr ? 1 : 0;
    LDPC_TRY(rule_params(d, &g.rule));
    // Nodes per wave.  The marginal lines a check pass gathers are re-used dv times; the fewer tiles are in flight at once, the
    // more of those re-reads hit on chip -- so a tile is cut into MANY short wave tasks (tile-major task order).  Measured on one
    // MI355X (sweep of 32 768 frames of the (3,6) n = 64 800 shape, profiles/r03_stream_chunking.txt): 64 checks per wave 20.9 ms,
    // 16: 19.9, 8: 19.4, 2-4 with 16 variables per wave: 19.1-19.3 ms; n = 1200 and the n = 10 000 ensemble agree.  Longer runs only
    // beyond 2^22 tasks per launch.
    auto per_wave = [&](int nodes, int base) {
        long v = base < 1 ? 1 : base;
        while ((long)((nodes + v - 1) / v) * tiles > (1L << 22) && v < 256) v *= 2;
        return (int)(v > nodes ? ((nodes + 3) / 4 * 4) : v);
    };
    g.cpw = per_wave(m, 4);
    g.cn_chunks = (m + g.cpw - 1) / g.cpw;
    g.vpw = per_wave(n, 16);
    g.vn_chunks = (n + g.vpw - 1) / g.vpw;
    // XCD-aware task order (task_of) where a tile's marginal rows fit one XCD's 4 MB L2: measured (profiles/r03_stream_xcd.txt) the check
    // pass then fetches E + n lines per tile -- its compulsory minimum -- instead of ~2E (n = 1200: 1.78 -> 1.24 GB per launch of 65 536
    // frames, n = 10 000: 3.63 -> 2.68 GB), at unchanged time (the re-reads were being served by the Infinity Cache); at n = 64 800
    // (16.6 MB of marginals per tile) nothing is re-used either way and the plain order is 2.5 % faster
    g.xcd_aware = (size_t)n * 64 * sizeof(T) <= ((size_t)4 << 20) ? 1 : 0;

    LDPC_TRY(prof.begin_decode());
    LDPC_HIP_TRY(hipMemsetAsync(xbits, 0, plane_words(tiles, n) * 8, st));
    LDPC_HIP_TRY(hipMemsetAsync(tflags, 0, (size_t)tiles * 16 + 64 + POLL_RING_BYTES, st));
    LDPC_HIP_TRY(hipMemsetAsync(iters, 0, (size_t)B * sizeof(int32_t), st));
    if (k.soft && !LAYERED) LDPC_HIP_TRY(hipMemsetAsync(marg, 0, (size_t)tiles * n * 64 * sizeof(T), st));  // frames that never sweep report 0
    if (sim) {  // device Monte-Carlo over BI-AWGN: the noise goes straight into the tile layout
        const int bpf = (n + 3) / 4, bpw = 16;
        hipLaunchKernelGGL((k_biawgn_tile<T>), dim3(((bpf + bpw - 1) / bpw + 3) / 4, tiles), dim3(64, 4), 0, st, *sim, B, n, bpf, bpw, LAYERED ? marg : prior);
    }
    if (!sim)
        hipLaunchKernelGGL((k_load_tile<T>), dim3((n + 63) / 64, tiles), dim3(256), 0, st, (const T*)k.priors, y0, B, n, LAYERED ? marg : prior, xbits);
    if constexpr (ALG == ALG_QMSA) launch_quantise<T>(g.rule, prior, (int64_t)tiles * n * 64, st);  // priors -> levels, in the workspace
    tiles_init_live(live, B, tiles, st);

    const int cap = max_iter > 0 ? max_iter : 100000;  // max_iter <= 0 == unlimited upstream (src/bpa.py:28); bounded here
    const double bytes_per_frame = sizeof(T) * (4.0 * E + n);
    SweepPolls p{st, (int*)((char*)d->flags.p + (size_t)tiles * 16 + 64), (volatile int*)d->pinned, poll_ev, repack, cap, tiles, bytes_per_frame};
    p.poll_every = SweepPolls::poll_every_300us(tiles, bytes_per_frame);
    p.every_sweep = p.eager = max_iter <= 0;  // an unbounded run polls at every sweep and reads at once
    const T *gather_msg = nullptr, *gather_marg = nullptr, *gather_prior = nullptr;  // non-null: the next sweep carries a folded repack out of that set
    const auto syndrome = [&](int* slot_dev) { tiles_syndrome(c, xbits, live, tflags, iters, slot_dev, B, p.cur_tiles, p.sweeps, fmap, st); };
    const auto repack_into = [&](int nt) {
        const TileSet& to = set[1 - cur];
        // the decisions of every frame of the old tiles (those that left keep them; the moved ones overwrite theirs later)
        launch_unpack(k, xbits, n, p.cur_tiles, fmap);
        hipLaunchKernelGGL(k_repack_plan, dim3(1), dim3(1024), 0, st, live, p.cur_tiles, (int32_t*)d->rbase.p);
        if (fold_repack) {
            // only the map now; the sweep enqueued below moves the state (GATHER passes: old set in, new set out)
            hipLaunchKernelGGL(k_repack_map, dim3(nt), dim3(64), 0, st, live, (u64*)to.live.p, (const int32_t*)d->rbase.p, fmap, (int32_t*)to.fmap.p,
                               (int32_t*)d->rmap.p, p.cur_tiles);
            gather_msg = msg;
            gather_marg = marg;
            gather_prior = prior;
        } else {
            const int rows_per_wave = 128;
            const int chunks = (int)((E + n + rows_per_wave - 1) / rows_per_wave);
            hipLaunchKernelGGL((k_repack<T, !LAYERED>), dim3((chunks + 3) / 4, nt), dim3(64, 4), 0, st, msg, (T*)to.edge.p, marg, (T*)to.node.p, prior,
                               (T*)to.prior.p, xbits, (u64*)to.planes.p, live, (u64*)to.live.p, (const int32_t*)d->rbase.p, fmap, (int32_t*)to.fmap.p,
                               p.cur_tiles, n, E, rows_per_wave);
        }
        use_set(1 - cur);
        fmap = (int32_t*)to.fmap.p;
        g.tiles = nt;
        return nt;
    };
    for (int it = 0; it < cap && !p.all_left; ++it) {
        if (early && (it > 0 || y0 != nullptr)) {
            LDPC_TRY(p.check_point(it, syndrome, repack_into));
            if (p.all_left) break;
        }
        LDPC_TRY(prof.mark(0));
        if constexpr (LAYERED) {
            dispatch_layers<T>(d, msg, marg, live, g, it == 0, st);
            LDPC_TRY(prof.mark(1));
            dispatch_decide<T>(c, marg, live, xbits, g, st);
        } else if (gather_msg) {  // the sweep that carries a repack: state read from the old set through the map, written densely into the new one
            // (never the first sweep, never a soft-output decode: first == 0 and g.freeze == 0)
            dispatch_cn<T, ALG, true>(c, msg, gather_marg, live, g, 0, st, gather_msg, (const int32_t*)d->rmap.p);
            LDPC_TRY(prof.mark(1));
            dispatch_vn<T, ALG, true>(c, msg, gather_prior, marg, live, xbits, g, st, prior, (const int32_t*)d->rmap.p);
            gather_msg = gather_marg = gather_prior = nullptr;
        } else {
            dispatch_cn<T, ALG>(c, msg, it == 0 ? prior : marg, live, g, it == 0 ? 1 : 0, st);
            LDPC_TRY(prof.mark(1));
            dispatch_vn<T, ALG>(c, msg, prior, marg, live, xbits, g, st);
        }
        LDPC_TRY(prof.mark(2));
        ++p.sweeps;
    }
    launch_decisions(k, xbits, live, n, p.cur_tiles, p.sweeps, fmap);
    if (k.soft && LAYERED) hipLaunchKernelGGL(k_soft_out_swept<T>, dim3((n + 3) / 4, tiles), dim3(256), 0, st, marg, (const int32_t*)iters, (T*)k.soft, B, n);
    if (k.soft && !LAYERED) hipLaunchKernelGGL(k_soft_out<T>, dim3((n + 3) / 4, tiles), dim3(256), 0, st, marg, (T*)k.soft, B, n);
    LDPC_TRY(p.finish());
    return end_decode(d, prof, p.sweeps, p.repacks);
}

}  // namespace

// =====================================================================================================================================
// fp16 STORAGE mode (LDPC_DTYPE_F16): the check -> variable messages -- the E-sized part of the sweep's traffic -- are kept as fp16, all
// arithmetic and the marginals stay fp32.  A lane must still move at least 4 bytes per access to use the memory system (2-byte lanes
// would halve the bytes AND the rate), so this mode works on PAIR-TILES of 128 frames: lane l holds frames l and 64 + l of the pair
// (= the 64-frame tiles 2P and 2P + 1 of the planes / live words, which keep their layout), a message line is 64 x half2 = 256 B, a
// prior line 64 x float2 = 512 B.  The sweep is the two-array form SURVEY 8(d) prices (v2c written by the variable pass and read back by the
// check pass): with 2-byte messages every E-sized line is moved exactly once per pass and nothing is re-read -- the marginal-resident form
// of the fp32 passes would gather 4-byte marginal lines dv times each, which at half-size messages becomes half of the traffic.  Bytes
// per frame-sweep: check pass 2E + 2E, variable pass 2E + 2E + 4n: 8E + 4n = 1.81 MB at n = 64 800 against 12E + 12n = 3.11 MB in fp32
// (SURVEY 8(d)'s all-fp16 figure 2(4E + n) differs only by the fp32 priors).
// A throughput mode, NOT the parity mode: messages are rounded to 11 significant bits each sweep (and saturate at +-65504 where the fp32
// mode would carry larger finite values); tests hold it to a stated per-sweep tolerance against the fp32 kernels and to the published
// curves.  Frame repack on pair-tiles (k_repack16); with a soft output there is none, and the soft output is that of the last sweep of the
// BATCH (frames that have left keep evolving).
namespace {

// the load and the conversion are separate so that a kernel can issue all its line loads before it touches the first result
__device__ __forceinline__ uint32_t msg16_ld_raw(const __half2* p) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)); }
__device__ __forceinline__ float2 msg16_cvt(uint32_t raw) { return __half22float2(*reinterpret_cast<const __half2*>(&raw)); }
__device__ __forceinline__ float2 msg16_ld(const __half2* p) { return msg16_cvt(msg16_ld_raw(p)); }
template <int ALG>
__device__ __forceinline__ float sat16(float v) {
    // finite values beyond the fp16 range saturate (min-sum messages of a trapped frame grow without bound); sum-product keeps its +-inf
    // and NaN (src/bpa.py:38 relies on them)
    if constexpr (ALG == ALG_SPA) return (__builtin_fabsf(v) <= 65504.0f || !(__builtin_fabsf(v) < __builtin_huge_valf())) ? v : __builtin_copysignf(65504.0f, v);
    else return __builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f);
}
template <int ALG>
__device__ __forceinline__ void msg16_st(__half2* p, float x, float y) {
    const __half2 h = __floats2half2_rn(sat16<ALG>(x), sat16<ALG>(y));
    __builtin_nontemporal_store(*reinterpret_cast<const uint32_t*>(&h), reinterpret_cast<uint32_t*>(p));
}

// priors [B,n] fp32 -> pair-tile layout [P][n][64] float2; optional hard word y0 -> decision planes of the two 64-frame tiles
__global__ __launch_bounds__(256) void k_load_tile16(const float* __restrict__ priors, const uint8_t* __restrict__ y0, int64_t B, int n,
                                                     float2* __restrict__ prior_t, u64* __restrict__ xbits) {
    __shared__ float sp[64][65];
    __shared__ uint8_t sy[64][68];
    const int P = blockIdx.y, v0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int sub = 0; sub < 2; ++sub) {
        const int tile = 2 * P + sub;
        __syncthreads();
        for (int f = ty; f < 64; f += 4) {
            const int64_t fr = (int64_t)tile * 64 + f;
            const int v = v0 + tx;
            float val = 0.0f;
            uint8_t yy = 0;
            if (fr < B && v < n) {
                if (y0) yy = y0[fr * n + v];
                val = priors[fr * n + v];
            }
            sp[f][tx] = val;
            sy[f][tx] = yy;
        }
        __syncthreads();
        for (int vv = ty; vv < 64; vv += 4) {
            const int v = v0 + vv;
            if (v < n) {
                reinterpret_cast<float*>(prior_t + ((int64_t)P * n + v) * 64 + tx)[sub] = sp[tx][vv];
                if (y0) {
                    const u64 one = __ballot(sy[tx][vv] != 0);
                    if (tx == 0) xbits[plane_at(tile, v, n)] = one;
                }
            }
        }
    }
}

// BI-AWGN channel + LLR straight into the pair-tile layout: the expressions of k_biawgn<float> (bit-identical priors)
__global__ __launch_bounds__(256) void k_biawgn_tile16(SimSource s, int64_t B, int n, int bpf, int blocks_per_wave, float2* __restrict__ prior_t) {
    const int lane = threadIdx.x, P = blockIdx.y;
    const int64_t fa = (int64_t)P * 128 + lane, fb = fa + 64;
    if (fa >= B) return;
    const int j0 = (blockIdx.x * 4 + threadIdx.y) * blocks_per_wave;
    const float sg = (float)s.sigma, k = (float)s.inv_var2, mean = (float)(2 * s.codeword - 1);
    float2* pt = prior_t + (int64_t)P * n * 64 + lane;
    for (int j = j0; j < min(bpf, j0 + blocks_per_wave); ++j) {
        const Philox4 pa = philox_word_block(s.seed, s.stream, s.frame0 + (uint64_t)fa, (uint32_t)j);
        const Philox4 pb = philox_word_block(s.seed, s.stream, s.frame0 + (uint64_t)fb, (uint32_t)j);  // (beyond the batch: never read back)
        float za[4], zb[4];
        box_muller<float>(pa.w[0], pa.w[1], za[0], za[1]);
        box_muller<float>(pa.w[2], pa.w[3], za[2], za[3]);
        box_muller<float>(pb.w[0], pb.w[1], zb[0], zb[1]);
        box_muller<float>(pb.w[2], pb.w[3], zb[2], zb[3]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * j + q < n) pt[(int64_t)(4 * j + q) * 64] = make_float2(-(k * (mean + sg * za[q])), -(k * (mean + sg * zb[q])));
    }
}

// Check pass: per check, GATHER the variable -> check lines of its edges (each line exactly once per sweep: no re-read, unlike the
// marginal-resident fp32 passes), apply the rule, STREAM the check -> variable lines out.  First sweep: v2c = prior (src/bpa.py:19).
// FIRST is a template parameter: as a run-time flag the compiler kept a branch per line and waited for every gathered line before issuing the next
template <int ALG, int DCMAX, int FIXED_DC, int UNR, bool FIRST>
__global__ __launch_bounds__(256) void k_cn16(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var, const int32_t* __restrict__ edge_vpos,
                                              __half2* __restrict__ c2v, const __half2* __restrict__ v2c, const float2* __restrict__ prior_t,
                                              const u64* __restrict__ live, int m, int n, int64_t E, int pairs, int tiles, int chunks,
                                              typename last_int_arg<float, ALG>::type cpw_arg) {
    const int cpw = last_int_arg<float, ALG>::value(cpw_arg);  // (corrected min-sum: scale and offset ride behind it, ldpc_cn.hpp)
    const Correction<float> corr = last_int_arg<float, ALG>::correction(cpw_arg);  // applied in fp32, before the message is rounded to half
    const float cap = last_int_arg<float, ALG>::cap(cpw_arg);                      // (fixed-point min-sum: every message is an integer <= 2047, exact in half)
    const int lane = threadIdx.x;
    int P, chunk;
    if (!task_of(pairs, chunks, 0, &P, &chunk)) return;
    if ((live[2 * P] | (2 * P + 1 < tiles ? live[2 * P + 1] : 0ull)) == 0) return;
    __half2* ct = c2v + (int64_t)P * E * 64 + lane;
    const __half2* vt = v2c + (int64_t)P * E * 64 + lane;
    const float2* pt = prior_t + (int64_t)P * n * 64 + lane;
    const int c_end = min(m, (chunk + 1) * cpw);
    for (int c = chunk * cpw; c < c_end; c += UNR) {
        float vx[UNR][DCMAX], vy[UNR][DCMAX];
        int k0[UNR], deg[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int cc = c + u;
            if (cc < c_end) {
                k0[u] = FIXED_DC > 0 ? cc * FIXED_DC : row_ptr[cc];
                deg[u] = FIXED_DC > 0 ? FIXED_DC : row_ptr[cc + 1] - k0[u];
            } else {
                k0[u] = 0;
                deg[u] = 0;
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
#pragma unroll
            for (int j = 0; j < DCMAX; ++j) {
                // a short row re-reads its last edge (an empty row edge 0): no branch per line
                const int kk = FIXED_DC > 0 ? k0[u] + j : (deg[u] > 0 ? k0[u] + (j < deg[u] ? j : deg[u] - 1) : 0);
                float2 v;
                if constexpr (FIRST) v = pt[(int64_t)edge_var[kk] * 64];
                else v = msg16_ld(vt + (int64_t)edge_vpos[kk] * 64);
                vx[u][j] = v.x;
                vy[u][j] = v.y;
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            cn_rule<float, ALG, DCMAX>(vx[u], deg[u], corr, cap);
            cn_rule<float, ALG, DCMAX>(vy[u], deg[u], corr, cap);
#pragma unroll
            for (int j = 0; j < DCMAX; ++j)
                if (j < deg[u]) msg16_st<ALG>(ct + (int64_t)(k0[u] + j) * 64, vx[u][j], vy[u][j]);
        }
    }
}

// Variable pass: per variable, gather its check -> variable lines (each read once), marginal = prior + ordered sum (src/bpa.py:35), decision
// bits, and v2c_j = marginal - c2v_j (src/bpa.py:37) STREAMED out in variable-major order (line p0 + j).  The marginal itself is written
// only when a soft output was asked for.
template <int ALG, int DVMAX, int UNR, int FIXED_DV>
__global__ __launch_bounds__(256) void k_vn16(const int32_t* __restrict__ col_ptr, const int32_t* __restrict__ col_edge, const __half2* __restrict__ c2v,
                                              __half2* __restrict__ v2c, const float2* __restrict__ prior_t, float2* __restrict__ marg_t,
                                              const u64* __restrict__ live, u64* __restrict__ xbits, int n, int64_t E, int pairs, int tiles, int chunks, int vpw) {
    const int lane = threadIdx.x;
    int P, chunk;
    if (!task_of(pairs, chunks, 0, &P, &chunk)) return;
    const bool has_b = 2 * P + 1 < tiles;
    const u64 lva = live[2 * P], lvb = has_b ? live[2 * P + 1] : 0ull;
    if ((lva | lvb) == 0) return;
    const __half2* ct = c2v + (int64_t)P * E * 64 + lane;
    __half2* vt = v2c + (int64_t)P * E * 64 + lane;
    const float2* pt = prior_t + (int64_t)P * n * 64 + lane;
    float2* mt = marg_t ? marg_t + (int64_t)P * n * 64 + lane : nullptr;
    u64* xa = xbits + plane_at(2 * P, 0, n);
    u64* xb = xbits + plane_at(2 * P + 1, 0, n);  // (only touched when the pair has a second tile)
    const int v_end = min(n, (chunk + 1) * vpw);
    for (int vbase = chunk * vpw; vbase < v_end; vbase += UNR) {
        float2 c[UNR][DVMAX], pr[UNR];
        uint32_t raw[UNR][DVMAX];
        u64 olda[UNR], oldb[UNR];
        int deg[UNR], p0[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int vv = vbase + u < v_end ? vbase + u : v_end - 1;  // past the end: the last variable once more, result unused
            p0[u] = FIXED_DV > 0 ? vv * FIXED_DV : col_ptr[vv];
            deg[u] = vbase + u < v_end ? (FIXED_DV > 0 ? FIXED_DV : col_ptr[vv + 1] - p0[u]) : -1;
            pr[u] = pt[(int64_t)vv * 64];
            // decisions of frames that have left, read with the lines (a read behind the stores of this variable would wait for them)
            if (lva != ~0ull) olda[u] = uniform_ld64(xa + 8 * vv);
            if (has_b && lvb != ~0ull) oldb[u] = uniform_ld64(xb + 8 * vv);
            // lines of an irregular variable sit behind a wave-uniform branch each; nothing in the branch but the load (no default value, no
            // conversion), so that no load waits for the one before it
#pragma unroll
            for (int j = 0; j < DVMAX; ++j) {
                if (FIXED_DV > 0 || j < deg[u]) raw[u][j] = msg16_ld_raw(ct + (int64_t)col_edge[p0[u] + j] * 64);
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int j = 0; j < DVMAX; ++j) c[u][j] = (FIXED_DV > 0 || j < deg[u]) ? msg16_cvt(raw[u][j]) : make_float2(0.0f, 0.0f);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (deg[u] < 0) continue;  // wave-uniform
            float sx = 0.0f, sy = 0.0f;  // ordered sum from +0.0, prior last (src/bpa.py:35, src/math_utils.py:7)
#pragma unroll
            for (int j = 0; j < DVMAX; ++j)
                if (FIXED_DV > 0 || j < deg[u]) {
                    sx += c[u][j].x;
                    sy += c[u][j].y;
                }
            const float2 marg = make_float2(pr[u].x + sx, pr[u].y + sy);
            if (mt) {  // soft output (diagnostic path): a frame that has left keeps the marginal of ITS last sweep, as the fp32 / fp64 kernels do
                float2 w = marg;
                if (lva != ~0ull || lvb != ~0ull) {
                    const float2 old = mt[(int64_t)(vbase + u) * 64];
                    if (!((lva >> lane) & 1ull)) w.x = old.x;
                    if (!((lvb >> lane) & 1ull)) w.y = old.y;
                }
                mt[(int64_t)(vbase + u) * 64] = w;
            }
#pragma unroll
            for (int j = 0; j < DVMAX; ++j)
                if (FIXED_DV > 0 || j < deg[u]) msg16_st<ALG>(vt + (int64_t)(p0[u] + j) * 64, marg.x - c[u][j].x, marg.y - c[u][j].y);
            const u64 onea = __ballot(marg.x < 0.0f), oneb = __ballot(marg.y < 0.0f);  // NaN marginal -> 0 (src/bpa.py:38,62)
            const int vv = vbase + u;
            u64 ma = onea, mb = oneb;
            if (lva != ~0ull) ma = (olda[u] & ~lva) | (onea & lva);  // frames that have left keep their decisions
            if (has_b && lvb != ~0ull) mb = (oldb[u] & ~lvb) | (oneb & lvb);
            if (lane == 0) {
                xa[8 * vv] = ma;
                if (has_b) xb[8 * vv] = mb;
            }
        }
    }
}

// marginal pair-tile [n][64] float2 -> [B,n] (diagnostic / tolerance tests; the MESSAGES of a frame that has left keep evolving in this
// mode, its stored marginal and decisions do not: k_vn16 masks both by the live words)
__global__ void k_soft_out16(const float2* __restrict__ soft_t, float* __restrict__ out, int64_t B, int n) {
    const int P = blockIdx.y, lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n) return;
    const float2 m = soft_t[((int64_t)P * n + v) * 64 + lane];
    const int64_t fa = (int64_t)P * 128 + lane, fb = fa + 64;
    if (fa < B) out[fa * n + v] = m.x;
    if (fb < B) out[fb * n + v] = m.y;
}

// Frame repack of the fp16 storage mode (the policy and the ranking of ldpc_repack.hpp, as k_repack above).  The two halves of a pair-tile are
// two 64-frame tiles (2P: the x components, 2P + 1: the y components), so a destination lane draws its two frames from two unrelated
// (tile, lane) sources: component (tile & 1) of lane `lane` of pair tile >> 1.  What has to move after a variable pass: the variable -> check
// lines, the priors, the decision planes, the live words and the frame map; the check -> variable lines are rewritten by the next check pass.
__global__ __launch_bounds__(256) void k_repack16(const __half2* __restrict__ v2c_src, __half2* __restrict__ v2c_dst, const float2* __restrict__ prior_src,
                                                  float2* __restrict__ prior_dst, const u64* __restrict__ xb_src, u64* __restrict__ xb_dst,
                                                  const u64* __restrict__ live_src, u64* __restrict__ live_dst, const int32_t* __restrict__ base,
                                                  const int32_t* __restrict__ frame_src, int32_t* __restrict__ frame_dst, int tiles_src, int n, int64_t E,
                                                  int rows_per_wave) {
    const int lane = threadIdx.x;
    const int dp = blockIdx.y;  // destination pair
    int sa, la, sb, lb;
    const bool ha = repack_source(base, live_src, tiles_src, (2 * dp) * 64 + lane, &sa, &la);
    const bool hb = repack_source(base, live_src, tiles_src, (2 * dp + 1) * 64 + lane, &sb, &lb);
    const int chunk = blockIdx.x * 4 + threadIdx.y;
    const int64_t rows = E + n;
    const int64_t r0 = (int64_t)chunk * rows_per_wave, r1 = min(rows, r0 + rows_per_wave);
    // a message line is 64 half2 = 128 halves, a prior line 64 float2 = 128 floats
    const __half* va = reinterpret_cast<const __half*>(v2c_src + ((int64_t)(sa >> 1) * E * 64 + la)) + (sa & 1);
    const __half* vb = reinterpret_cast<const __half*>(v2c_src + ((int64_t)(sb >> 1) * E * 64 + lb)) + (sb & 1);
    const float* pa = reinterpret_cast<const float*>(prior_src + ((int64_t)(sa >> 1) * n * 64 + la)) + (sa & 1);
    const float* pb = reinterpret_cast<const float*>(prior_src + ((int64_t)(sb >> 1) * n * 64 + lb)) + (sb & 1);
    __half2* vd = v2c_dst + (int64_t)dp * E * 64 + lane;
    float2* pd = prior_dst + (int64_t)dp * n * 64 + lane;
    const __half hz = __float2half(0.0f);
    for (int64_t r = r0; r < r1; ++r) {
        if (r < E) {
            vd[r * 64] = __halves2half2(ha ? va[r * 128] : hz, hb ? vb[r * 128] : hz);
        } else {
            const int64_t v = r - E;
            pd[v * 64] = make_float2(ha ? pa[v * 128] : 0.0f, hb ? pb[v * 128] : 0.0f);
            const u64 wa = ha ? xb_src[plane_at(sa, v, n)] : 0ull, wb = hb ? xb_src[plane_at(sb, v, n)] : 0ull;
            const u64 plane_a = __ballot(ha && ((wa >> la) & 1ull)), plane_b = __ballot(hb && ((wb >> lb) & 1ull));
            if (lane == 0) {
                xb_dst[plane_at(2 * dp, v, n)] = plane_a;
                xb_dst[plane_at(2 * dp + 1, v, n)] = plane_b;
            }
        }
    }
    if (chunk == 0) {
        frame_dst[(int64_t)(2 * dp) * 64 + lane] = ha ? (frame_src ? frame_src[(int64_t)sa * 64 + la] : sa * 64 + la) : -1;
        frame_dst[(int64_t)(2 * dp + 1) * 64 + lane] = hb ? (frame_src ? frame_src[(int64_t)sb * 64 + lb] : sb * 64 + lb) : -1;
        const u64 lva = __ballot(ha), lvb = __ballot(hb);
        if (lane == 0) {
            live_dst[2 * dp] = lva;
            live_dst[2 * dp + 1] = lvb;
        }
    }
}

template <int ALG>
int run16(Decoder* d, const DecodeCall& k, const SimSource* sim) {
    const Code* c = d->code;
    const int n = c->n, m = c->m;
    const int64_t E = c->E, B = k.B;
    const int32_t max_iter = k.max_iter;
    const uint8_t* const y0 = k.y0;
    int32_t* const iters = k.iters;
    float* const soft_out = (float*)k.soft;
    const hipStream_t st = k.stream;
    if (!degrees_supported(c)) return LDPC_E_UNSUPPORTED;
    RuleParams rule;
    LDPC_TRY(rule_params(d, &rule));
    const int tiles0 = (int)((B + 63) / 64), pairs0 = (tiles0 + 1) / 2;
    int tiles = tiles0, pairs = pairs0;  // shrink when the live frames are repacked into dense pair-tiles
    const bool early = !(k.flags & FLAG_NO_EARLY_EXIT);
    // a state set of this mode: variable -> check lines (edge), priors, planes, live words, map; marginals (node) only with a soft output
    TileSet* const set = d->set;
    LDPC_TRY(d->c2v16.reserve((size_t)pairs * E * 64 * sizeof(__half2)));
    LDPC_TRY(set[0].edge.reserve((size_t)pairs * E * 64 * sizeof(__half2)));  // variable -> check lines, variable-major
    // Frame repack (k_repack16; policy of the fp32 passes): the live frames are gathered into dense pair-tiles
    RepackPolicy repack(early && soft_out == nullptr && tiles0 >= 4);
    if (repack.on) {
        const size_t np2 = (repack.target_tiles(tiles0) + 1) / 2;  // pairs of the second set
        if (set[1].edge.reserve(np2 * E * 64 * sizeof(__half2)) || set[1].prior.reserve(np2 * n * 64 * sizeof(float2)) ||
            set[1].planes.reserve(plane_words((int)(2 * np2), n) * 8) || set[1].live.reserve(2 * np2 * 8) || set[1].fmap.reserve(2 * np2 * 64 * sizeof(int32_t)) ||
            set[0].fmap.reserve(2 * np2 * 64 * sizeof(int32_t)) || d->rbase.reserve(((size_t)tiles0 + 2) * sizeof(int32_t)))
            repack.on = false;  // no room for a second set: decode without repacking
    }
    if (soft_out) LDPC_TRY(set[0].node.reserve((size_t)pairs * n * 64 * sizeof(float2)));
    if (!d->graph_tab.p) {  // row-major edge k -> its position in the CSC edge list (where the variable pass writes its v2c line)
        std::vector<int32_t> vpos((size_t)E);
        for (int64_t p = 0; p < E; ++p) vpos[(size_t)c->col_edge[(size_t)p]] = (int32_t)p;
        LDPC_TRY(d->graph_tab.reserve((size_t)E * sizeof(int32_t) + 16));
        LDPC_HIP_TRY(hipMemcpy(d->graph_tab.p, vpos.data(), (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    const int32_t* edge_vpos = (const int32_t*)d->graph_tab.p;
    LDPC_TRY(set[0].prior.reserve((size_t)pairs * n * 64 * sizeof(float2)));
    LDPC_TRY(set[0].planes.reserve(plane_words(2 * pairs, n) * 8));
    LDPC_TRY(set[0].live.reserve((size_t)2 * pairs * 8));
    LDPC_TRY(d->flags.reserve((size_t)2 * pairs * 16 + 64 + POLL_RING_BYTES));
    __half2* msg = (__half2*)d->c2v16.p;
    float2* marg = soft_out ? (float2*)set[0].node.p : nullptr;
    int cur = 0;  // which set holds the state; the pointers below are re-read from it after a flip
    __half2* v2c;
    float2* prior;
    u64 *xbits, *live;
    int32_t* fmap = nullptr;  // frame of (tile, lane); null = identity (never repacked)
    auto use_set = [&](int s) {
        cur = s;
        v2c = (__half2*)set[s].edge.p;
        prior = (float2*)set[s].prior.p;
        xbits = (u64*)set[s].planes.p;
        live = (u64*)set[s].live.p;
    };
    use_set(0);
    u64* tflags = (u64*)d->flags.p;  // [2 * pairs][2], the device poll ring behind them
    hipEvent_t poll_ev[POLL_RING];
    for (int i = 0; i < POLL_RING; ++i) LDPC_TRY(prof_event(d, i, &poll_ev[i]));
    DecodeProf prof{d, st, POLL_RING};
    LDPC_HIP_TRY(hipMemsetAsync(xbits, 0, plane_words(2 * pairs, n) * 8, st));
    LDPC_HIP_TRY(hipMemsetAsync(tflags, 0, (size_t)2 * pairs * 16 + 64 + POLL_RING_BYTES, st));
    LDPC_HIP_TRY(hipMemsetAsync(live, 0, (size_t)2 * pairs * 8, st));
    LDPC_HIP_TRY(hipMemsetAsync(iters, 0, (size_t)B * sizeof(int32_t), st));
    if (marg) LDPC_HIP_TRY(hipMemsetAsync(marg, 0, (size_t)pairs * n * 64 * sizeof(float2), st));  // frames that never sweep report 0
    if (sim) {
        const int bpf = (n + 3) / 4, bpw = 16;
        hipLaunchKernelGGL(k_biawgn_tile16, dim3(((bpf + bpw - 1) / bpw + 3) / 4, pairs), dim3(64, 4), 0, st, *sim, B, n, bpf, bpw, prior);
    } else {
        hipLaunchKernelGGL(k_load_tile16, dim3((n + 63) / 64, pairs), dim3(256), 0, st, (const float*)k.priors, y0, B, n, prior, xbits);
    }
    if constexpr (ALG == ALG_QMSA) launch_quantise<float>(rule, reinterpret_cast<float*>(prior), (int64_t)pairs * n * 128, st);  // priors -> levels
    tiles_init_live(live, B, tiles, st);
    const int cpw = 4, vpw = 16;
    const int cn_chunks = (m + cpw - 1) / cpw, vn_chunks = (n + vpw - 1) / vpw;
    const int cap = max_iter > 0 ? max_iter : 100000;
    // the live counters are read at once, every fourth sweep; every sweep where a sweep is more than ~1.5 ms of streaming work
    // (the round trip is then a percent of it, and frames leave by the thousand per sweep: the repack should not wait three sweeps)
    const double bytes_per_frame = 8.0 * E + 4.0 * n;
    SweepPolls p{st, (int*)((char*)d->flags.p + (size_t)2 * pairs * 16 + 64), (volatile int*)d->pinned, poll_ev, repack, cap, tiles, bytes_per_frame};
    p.poll_every = sweep_us(tiles, bytes_per_frame) > 1500.0 ? 1 : 4;
    p.eager = true;
    const auto syndrome = [&](int* slot_dev) { tiles_syndrome(c, xbits, live, tflags, iters, slot_dev, B, tiles, p.sweeps, fmap, st); };
    const auto repack_into = [&](int nt) {
        const int np = (nt + 1) / 2;
        const TileSet& to = set[1 - cur];
        // the decisions of every frame of the old tiles (those that left keep them; the moved ones overwrite theirs at the end)
        launch_unpack(k, xbits, n, tiles, fmap);
        hipLaunchKernelGGL(k_repack_plan, dim3(1), dim3(1024), 0, st, live, tiles, (int32_t*)d->rbase.p);
        const int rows_per_wave = 128;
        const int chunks = (int)((E + n + rows_per_wave - 1) / rows_per_wave);
        hipLaunchKernelGGL(k_repack16, dim3((chunks + 3) / 4, np), dim3(64, 4), 0, st, v2c, (__half2*)to.edge.p, prior, (float2*)to.prior.p, xbits,
                           (u64*)to.planes.p, live, (u64*)to.live.p, (const int32_t*)d->rbase.p, (const int32_t*)fmap, (int32_t*)to.fmap.p, tiles, n, E,
                           rows_per_wave);
        use_set(1 - cur);
        fmap = (int32_t*)to.fmap.p;
        pairs = np;
        tiles = 2 * np;  // (an odd tile count leaves the last pair's second tile without a live frame)
        return tiles;
    };
    for (int it = 0; it < cap && !p.all_left; ++it) {
        if (early && (it > 0 || y0 != nullptr)) {
            LDPC_TRY(p.check_point(it, syndrome, repack_into));
            if (p.all_left) break;
        }
        LDPC_TRY(prof.mark(0));
        const dim3 cgrid(task_blocks(pairs, cn_chunks, 0)), vgrid(task_blocks(pairs, vn_chunks, 0)), blk(64, 4);
        check_class(c, [&](auto dcm, auto fdc) {
            constexpr int DCM = decltype(dcm)::value, FDC = decltype(fdc)::value, UNR = DCM <= 6 ? 2 : 1;
            const auto kern = it == 0 ? k_cn16<ALG, DCM, FDC, UNR, true> : k_cn16<ALG, DCM, FDC, UNR, false>;
            hipLaunchKernelGGL(kern, cgrid, blk, 0, st, c->d_row_ptr, c->d_edge_var, edge_vpos, msg, v2c, prior, live, m, n, E, pairs, tiles, cn_chunks,
                               last_int_arg<float, ALG>::make(cpw, rule));
        });
        LDPC_TRY(prof.mark(1));
        var_class<false>(c, [&](auto dvm, auto fdv) {
            constexpr int DVM = decltype(dvm)::value, UNR = DVM <= 4 ? 4 : (DVM == 8 ? 2 : 1);
            hipLaunchKernelGGL((k_vn16<alg_family(ALG), DVM, UNR, decltype(fdv)::value>), vgrid, blk, 0, st, c->d_col_ptr, c->d_col_edge, msg, v2c, prior, marg, live, xbits, n, E,
                               pairs, tiles, vn_chunks, vpw);
        });
        LDPC_TRY(prof.mark(2));
        ++p.sweeps;
    }
    launch_decisions(k, xbits, live, n, tiles, p.sweeps, fmap);
    if (soft_out) hipLaunchKernelGGL(k_soft_out16, dim3((n + 3) / 4, pairs), dim3(256), 0, st, marg, soft_out, B, n);  // (no repack with a soft output)
    LDPC_TRY(p.finish());
    return end_decode(d, prof, p.sweeps, p.repacks);
}

bool batch_fits(int64_t B) {
    if (B <= (int64_t)65535 * 64) return true;
    set_error("batch of %lld frames exceeds one launch (max %d); split the call", (long long)B, 65535 * 64);
    return false;
}

// The decoder's algorithm -> f(ALG) as a std::integral_constant: one arm per LLR row of kAlgs
template <class F>
int alg_class(const Decoder* d, F&& f) {
    switch (d->alg) {
        case ALG_MSA: return f(int_c<ALG_MSA>{});
        case ALG_NMSA: return f(int_c<ALG_NMSA>{});
        case ALG_QMSA: return f(int_c<ALG_QMSA>{});
        case ALG_LMSA: return f(int_c<ALG_LMSA>{});
        default: return f(int_c<ALG_SPA>{});
    }
}

// LLR decoders: the driver of the decoder's storage type; with `sim` the priors are drawn into the tiles instead of loaded
int run_llr(Decoder* d, const DecodeCall& k, const SimSource* sim) {
    return alg_class(d, [&](auto alg) -> int {
        constexpr int ALG = decltype(alg)::value;
        if constexpr (alg_row(ALG).f16)
            if (d->dtype == DT_F16) return run16<ALG>(d, k, sim);  // priors are fp32
        return d->dtype == DT_F64 ? run<double, ALG>(d, k, sim) : run<float, ALG>(d, k, sim);
    });
}

}  // namespace

// ldpc_simulate on the streaming kernels, BI-AWGN with the all-`codeword` word: channel + LLR generated into the tiles, then the decode
int stream_simulate_biawgn(Decoder* d, const DecodeCall& k, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0) {
    if (k.B <= 0) return LDPC_OK;
    if (d->alg == ALG_BEC) {
        set_error("stream_simulate_biawgn: LLR decoders only");
        return LDPC_E_ARG;
    }
    if (!batch_fits(k.B)) return LDPC_E_ARG;
    const double var = pow(10.0, -param / 10.0);  // src/biawgn.py:10 -- the host arithmetic of channel_generate()
    const SimSource s{sqrt(var), 2.0 / var, codeword, seed, frame0, (uint32_t)stream_id};
    return run_llr(d, k, &s);
}

int stream_decode(Decoder* d, const DecodeCall& k) {
    if (k.B <= 0) return LDPC_OK;
    if (!batch_fits(k.B)) return LDPC_E_ARG;
    if (d->alg == ALG_BEC ? !k.y0 : !k.priors) {
        set_error(d->alg == ALG_BEC ? "erasure decoder needs the received symbols (y0)" : "priors pointer is null");
        return LDPC_E_ARG;
    }
    return d->alg == ALG_BEC ? becs_stream_decode(d, k) : run_llr(d, k, nullptr);  // erasure: bit-sliced, ldpc_bec_stream.hip
}

}  // namespace ldpc

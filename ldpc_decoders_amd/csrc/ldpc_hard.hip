// Bit-sliced Gallager-B hard-decision decoding (include/ldpc_hip.h, ldpc_hard_*).
//
// A message is ONE bit; a plane word holds it for the 32 frames of a slab (bit f = frame f), so every step of the contract is word logic
// (ldpc_bec_planes.hpp): the check rule is an XOR, the variable rule a vertical counter of the d disagreement planes and two
// comparisons against constants.
//
// Streaming kernels (any code).  A supertile is 64 slabs = 2048 frames: lane L of a wave owns slab L, a "line" is the 64 words of one
// plane of one supertile (256 contiguous bytes), every H index is wave-uniform.  Per supertile, in lines:
//     [0, n)            y      the received word
//     [n, 2n)           x      the decisions, latched under the live mask
//     [2n, 2n + E)      v2c    in variable-major (CSC) order: the variable pass writes a stream, a check gathers each of its lines once
//     [2n + E, .. + m)  P      the parity of all messages into each check
// k_hard_load transposes [B, n] bytes into y / x / v2c (iteration 0: v2c = y); one sweep is k_hard_check (P of v2c, and the syndrome of x
// in the same gathers: the exit test of the sweep BEFORE, at sweep 1 the iteration-0 test), k_hard_exit (per-frame iters, live masks,
// supertiles without a live frame are switched off) and k_hard_var; k_hard_unload writes bytes and / or packed words.
//
// LDS-resident kernel (k_hard_lds).  One workgroup of 256 threads owns one slab for all its sweeps: the same four arrays as 32-bit
// words in the LDS, hard_lds_bytes() per slab; thread t takes checks / variables t, t + 256, ...; the graph tables are read through L2.
// Slabs are handed out by an atomic dispenser.  LDPC_HARD_TABLES=lds (read at create) selects the measured alternative, the tables as
// 16-bit words in the LDS behind the planes: fewer slabs per CU, and slower (profiles/r13_galb.md) -- kept so that the record can be re-run.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include "ldpc_bec_planes.hpp"
#include "ldpc_hard.hpp"
#include "ldpc_sim.hpp"

namespace ldpc {

struct Hard {
    Code* code = nullptr;
    int backend = BK_AUTO;  // as requested
    bool use_lds = false;   // what it resolved to
    int t = 0;              // threshold parameter (ldpc_hard_set_threshold)
    int last_backend = BK_STREAM;
    int num_cu = 0, slabs_per_cu = 0;
    int64_t lds_bytes = 0;   // the LDS-fit rule's left side
    bool tab_lds = false;    // measurement variant (LDPC_HARD_TABLES=lds): graph tables as 16-bit words in the LDS
    int64_t launch_lds = 0;  // dynamic LDS of the launch
    DevBuf vpos;        // [E] variable-major position of row-major edge e
    DevBuf chk_of_pos;  // [E] check of variable-major position p
    DevBuf state;       // streaming planes
    DevBuf ctl;         // streaming: live [S][64], unsat [S][64], stlive [S]; then 2 words: live supertiles, slab dispenser
    SimStage sim;       // staging of ldpc_hard_simulate
    uint32_t* pinned = nullptr;  // host poll word
};

namespace {

constexpr int NB_CNT = 6;  // planes of the vertical counter: degrees up to HARD_MAX_DV = 63

// S += plane (a ripple of half adders from the low plane up)
__device__ __forceinline__ void ripple_add(uint32_t (&S)[NB_CNT], uint32_t carry) {
#pragma unroll
    for (int b = 0; b < NB_CNT; ++b) {
        const uint32_t c = S[b] & carry;
        S[b] ^= carry;
        carry = c;
    }
}
// flip threshold b_d of the contract
__device__ __forceinline__ int flip_threshold(int d, int t) {
    if (t == 0) return (d > 0 ? (d - 1) / 2 : 0) + 1;
    const int cap = d - 1 > 1 ? d - 1 : 1;
    return t < cap ? t : cap;
}

// The variable rule for one variable, on any memory: V = the v2c words of this variable's positions [p0, p1), P = the check parities.
// Returns the decision plane; rewrites the messages.
template <class IDX, class LoadV, class StoreV, class LoadP>
__device__ __forceinline__ uint32_t variable_rule(uint32_t y, int p0, int p1, int t, const IDX* __restrict__ chk_of_pos, LoadV&& loadV,
                                                  StoreV&& storeV, LoadP&& loadP) {
    const int d = p1 - p0;
    uint32_t S[NB_CNT] = {0, 0, 0, 0, 0, 0};
    for (int p = p0; p < p1; ++p) ripple_add(S, loadP(chk_of_pos[p]) ^ loadV(p) ^ y);
    const int b = flip_threshold(d, t);
    const uint32_t flip = plane_ge<NB_CNT>(S, (d + 1) / 2 + 1);  // 2 T > d + 1
    const uint32_t ge_b = plane_ge<NB_CNT>(S, b), ge_b1 = plane_ge<NB_CNT>(S, b + 1);
    for (int p = p0; p < p1; ++p) {
        const uint32_t delta = loadP(chk_of_pos[p]) ^ loadV(p) ^ y;
        storeV(p, y ^ mux(delta, ge_b1, ge_b));  // T - delta >= b
    }
    return y ^ flip;
}

__device__ __forceinline__ uint32_t slab_mask(int64_t B, int64_t f0) {
    const int64_t cnt = B - f0;
    return cnt >= HARD_SLAB ? ~0u : cnt <= 0 ? 0u : ((1u << (int)cnt) - 1u);
}

// ---- streaming kernels ----------------------------------------------------------------------------------------------------------

// [B, n] bytes -> y, x and v2c planes of supertile blockIdx.y, variables [64 blockIdx.x, + 64); block (0, s) also sets the live masks
__global__ __launch_bounds__(256) void k_hard_load(const uint8_t* __restrict__ y, int64_t B, int n, int64_t E, int m, uint32_t* __restrict__ state,
                                                   const int32_t* __restrict__ col_ptr, uint32_t* __restrict__ live, uint32_t* __restrict__ unsat,
                                                   int32_t* __restrict__ stlive) {
    __shared__ uint8_t part[4][64][68];  // [quarter of the slab][slab][variable]: rows of 17 words, the second phase reads down a column
    const int t = threadIdx.x, lo = t & 63, q = t >> 6, s = blockIdx.y;
    const int v0 = blockIdx.x * 64;
    const size_t NW = 2 * (size_t)n + (size_t)E + (size_t)m;
    uint32_t* base = state + (size_t)s * NW * 64;
    if (blockIdx.x == 0 && t < 64) {
        live[s * 64 + t] = slab_mask(B, (int64_t)s * HARD_SUPER + (int64_t)t * HARD_SLAB);
        unsat[s * 64 + t] = 0u;
        if (t == 0) stlive[s] = 1;
    }
    const int v = v0 + lo;
    for (int L = 0; L < 64; ++L) {
        const int64_t f0 = (int64_t)s * HARD_SUPER + (int64_t)L * HARD_SLAB + q * 8;
        uint32_t b = 0;
        if (v < n)
            for (int k = 0; k < 8; ++k)
                if (f0 + k < B) b |= (uint32_t)(y[(size_t)(f0 + k) * n + v] & 1u) << k;
        part[q][L][lo] = (uint8_t)b;
    }
    __syncthreads();
    for (int vl = q * 16; vl < q * 16 + 16; ++vl) {
        const int vv = v0 + vl;
        if (vv >= n) break;
        const uint32_t w = (uint32_t)part[0][lo][vl] | ((uint32_t)part[1][lo][vl] << 8) | ((uint32_t)part[2][lo][vl] << 16) | ((uint32_t)part[3][lo][vl] << 24);
        base[(size_t)vv * 64 + lo] = w;
        base[((size_t)n + vv) * 64 + lo] = w;
        for (int p = col_ptr[vv]; p < col_ptr[vv + 1]; ++p) base[(2 * (size_t)n + p) * 64 + lo] = w;
    }
}

// one wave per (supertile, check): P_c = XOR of the messages into c; the syndrome of x at c is OR-ed into the supertile's unsat words
__global__ __launch_bounds__(256) void k_hard_check(uint32_t* __restrict__ state, int n, int64_t E, int m, int nst, const int32_t* __restrict__ row_ptr,
                                                    const int32_t* __restrict__ vpos, const int32_t* __restrict__ edge_var,
                                                    const int32_t* __restrict__ stlive, uint32_t* __restrict__ unsat) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = __builtin_amdgcn_readfirstlane((int)((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (gw >= (int64_t)nst * m) return;
    const int s = (int)(gw / m), c = (int)(gw - (int64_t)s * m);
    if (!stlive[s]) return;
    const size_t NW = 2 * (size_t)n + (size_t)E + (size_t)m;
    uint32_t* base = state + (size_t)s * NW * 64;
    const uint32_t* X = base + (size_t)n * 64;
    const uint32_t* V = base + 2 * (size_t)n * 64;
    uint32_t par = 0, syn = 0;
    for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
        par ^= V[(size_t)vpos[e] * 64 + lane];
        syn ^= X[(size_t)edge_var[e] * 64 + lane];
    }
    base[(2 * (size_t)n + (size_t)E + c) * 64 + lane] = par;
    if (syn) atomicOr(&unsat[s * 64 + lane], syn);
}

// one wave per supertile: the frames whose x satisfies every check (all live frames when `final`, none before it under no_early) leave
// with iters = sweep; a supertile whose last frame has left is switched off
__global__ __launch_bounds__(64) void k_hard_exit(uint32_t* __restrict__ live, uint32_t* __restrict__ unsat, int32_t* __restrict__ stlive,
                                                  int32_t* __restrict__ iters, int64_t B, int sweep, int final, int no_early,
                                                  uint32_t* __restrict__ live_tiles) {
    const int s = blockIdx.x, L = threadIdx.x;
    if (!stlive[s]) return;
    uint32_t lv = live[s * 64 + L];
    const uint32_t us = unsat[s * 64 + L];
    const uint32_t leaving = final ? lv : no_early ? 0u : (lv & ~us);
    const int64_t f0 = (int64_t)s * HARD_SUPER + (int64_t)L * HARD_SLAB;
    for (uint32_t rest = leaving; rest; rest &= rest - 1) {
        const int64_t f = f0 + __builtin_ctz(rest);
        if (f < B) iters[f] = sweep;
    }
    lv &= ~leaving;
    live[s * 64 + L] = lv;
    unsat[s * 64 + L] = 0u;
    const bool any = __ballot(lv != 0u) != 0ull;
    if (L == 0) {
        stlive[s] = any ? 1 : 0;
        if (any) atomicAdd(live_tiles, 1u);
    }
}

// one wave per (supertile, variable)
__global__ __launch_bounds__(256) void k_hard_var(uint32_t* __restrict__ state, int n, int64_t E, int m, int nst, int t, const int32_t* __restrict__ col_ptr,
                                                  const int32_t* __restrict__ chk_of_pos, const int32_t* __restrict__ stlive,
                                                  const uint32_t* __restrict__ live) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = __builtin_amdgcn_readfirstlane((int)((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (gw >= (int64_t)nst * n) return;
    const int s = (int)(gw / n), v = (int)(gw - (int64_t)s * n);
    if (!stlive[s]) return;
    const size_t NW = 2 * (size_t)n + (size_t)E + (size_t)m;
    uint32_t* base = state + (size_t)s * NW * 64;
    uint32_t* V = base + 2 * (size_t)n * 64;
    const uint32_t* P = base + (2 * (size_t)n + (size_t)E) * 64;
    const uint32_t y = base[(size_t)v * 64 + lane];
    const uint32_t x = variable_rule(
        y, col_ptr[v], col_ptr[v + 1], t, chk_of_pos, [&](int p) { return V[(size_t)p * 64 + lane]; },
        [&](int p, uint32_t w) { V[(size_t)p * 64 + lane] = w; }, [&](int c) { return P[(size_t)c * 64 + lane]; });
    uint32_t* xp = base + ((size_t)n + v) * 64 + lane;
    *xp = mux(live[s * 64 + lane], x, *xp);
}

// x planes of supertile blockIdx.y, variables [64 blockIdx.x, + 64) -> bytes [B, n] and / or packed words [B, W]
__global__ __launch_bounds__(256) void k_hard_unload(const uint32_t* __restrict__ state, int64_t B, int n, int64_t E, int m, uint8_t* __restrict__ xhat,
                                                     uint32_t* __restrict__ bits) {
    __shared__ uint32_t tile[64][65];  // [variable][slab]
    const int t = threadIdx.x, lo = t & 63, q = t >> 6, s = blockIdx.y;
    const int v0 = blockIdx.x * 64, W = (n + 31) / 32;
    const size_t NW = 2 * (size_t)n + (size_t)E + (size_t)m;
    const uint32_t* X = state + ((size_t)s * NW + (size_t)n) * 64;
    for (int vl = q * 16; vl < q * 16 + 16; ++vl) tile[vl][lo] = v0 + vl < n ? X[(size_t)(v0 + vl) * 64 + lo] : 0u;
    __syncthreads();
    const int64_t fs = (int64_t)s * HARD_SUPER;
    if (xhat && v0 + lo < n) {
        for (int L = 0; L < 64; ++L) {
            const uint32_t w = tile[lo][L];
            for (int k = 0; k < 8; ++k) {
                const int64_t f = fs + L * HARD_SLAB + q * 8 + k;
                if (f < B) xhat[(size_t)f * n + v0 + lo] = (uint8_t)((w >> (q * 8 + k)) & 1u);
            }
        }
    }
    if (bits) {
        for (int k = 0; k < 8; ++k) {
            const int fr = t + 256 * k;
            if (fs + fr >= B) break;
            for (int w = 0; w < 2; ++w) {
                if (v0 / 32 + w >= W) break;
                uint32_t word = 0;
                for (int i = 0; i < 32; ++i) word |= ((tile[w * 32 + i][fr >> 5] >> (fr & 31)) & 1u) << i;
                bits[(size_t)(fs + fr) * W + v0 / 32 + w] = word;
            }
        }
    }
}

// ---- LDS-resident kernel ---------------------------------------------------------------------------------------------------------

// TAB_LDS: the five graph tables as 16-bit words in the LDS behind the planes (E < 65536) instead of 32-bit words read through L2
template <bool TAB_LDS>
__global__ __launch_bounds__(256) void k_hard_lds(const uint8_t* __restrict__ y, int64_t B, int n, int E, int m, int t, int max_iter, int no_early,
                                                  const int32_t* __restrict__ g_row_ptr, const int32_t* __restrict__ g_vpos,
                                                  const int32_t* __restrict__ g_edge_var, const int32_t* __restrict__ g_col_ptr,
                                                  const int32_t* __restrict__ g_chk_of_pos, uint32_t* __restrict__ dispenser,
                                                  uint8_t* __restrict__ xhat, uint32_t* __restrict__ bits, int32_t* __restrict__ iters) {
    extern __shared__ uint32_t sm[];
    uint32_t* Y = sm;
    uint32_t* X = sm + n;
    uint32_t* V = sm + 2 * (size_t)n;
    uint32_t* P = V + E;
    uint32_t* ctl = P + m;  // [0] slab index, [1] unsatisfied frames
    const int tid = threadIdx.x, W = (n + 31) / 32;
    using IDX = typename std::conditional<TAB_LDS, uint16_t, int32_t>::type;
    const IDX *row_ptr, *vpos, *edge_var, *col_ptr, *chk_of_pos;
    if constexpr (TAB_LDS) {
        uint16_t* tb = (uint16_t*)(ctl + 4);
        uint16_t *t_rp = tb, *t_vp = t_rp + (m + 1), *t_ev = t_vp + E, *t_cp = t_ev + E, *t_cop = t_cp + (n + 1);
        for (int i = tid; i <= m; i += 256) t_rp[i] = (uint16_t)g_row_ptr[i];
        for (int i = tid; i <= n; i += 256) t_cp[i] = (uint16_t)g_col_ptr[i];
        for (int i = tid; i < E; i += 256) {
            t_vp[i] = (uint16_t)g_vpos[i];
            t_ev[i] = (uint16_t)g_edge_var[i];
            t_cop[i] = (uint16_t)g_chk_of_pos[i];
        }
        row_ptr = t_rp, vpos = t_vp, edge_var = t_ev, col_ptr = t_cp, chk_of_pos = t_cop;
    } else {
        row_ptr = g_row_ptr, vpos = g_vpos, edge_var = g_edge_var, col_ptr = g_col_ptr, chk_of_pos = g_chk_of_pos;
    }
    const int64_t nslabs = (B + HARD_SLAB - 1) / HARD_SLAB;
    for (;;) {
        if (tid == 0) {
            ctl[0] = atomicAdd(dispenser, 1u);
            ctl[1] = 0u;
        }
        __syncthreads();
        const int64_t slab = ctl[0];
        if (slab >= nslabs) break;
        const int64_t f0 = slab * HARD_SLAB;
        const int cnt = (int)(B - f0 < HARD_SLAB ? B - f0 : HARD_SLAB);
        uint32_t live = slab_mask(B, f0);
        for (int v = tid; v < n; v += 256) {
            uint32_t w = 0;
            for (int f = 0; f < cnt; ++f) w |= (uint32_t)(y[(size_t)(f0 + f) * n + v] & 1u) << f;
            Y[v] = w;
            X[v] = w;
            for (int p = col_ptr[v]; p < col_ptr[v + 1]; ++p) V[p] = w;
        }
        __syncthreads();
        for (int sweep = 0;; ++sweep) {
            uint32_t syn_any = 0;
            for (int c = tid; c < m; c += 256) {
                uint32_t par = 0, syn = 0;
                for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
                    par ^= V[vpos[e]];
                    syn ^= X[edge_var[e]];
                }
                P[c] = par;
                syn_any |= syn;
            }
            if (syn_any) atomicOr(&ctl[1], syn_any);
            __syncthreads();
            const uint32_t leaving = sweep == max_iter ? live : no_early ? 0u : (live & ~ctl[1]);
            if (tid < HARD_SLAB && ((leaving >> tid) & 1u)) iters[f0 + tid] = sweep;
            live &= ~leaving;
            __syncthreads();
            if (tid == 0) ctl[1] = 0u;
            if (!live) break;
            for (int v = tid; v < n; v += 256) {
                const uint32_t x = variable_rule(
                    Y[v], col_ptr[v], col_ptr[v + 1], t, chk_of_pos, [&](int p) { return V[p]; }, [&](int p, uint32_t w) { V[p] = w; },
                    [&](int c) { return P[c]; });
                X[v] = mux(live, x, X[v]);
            }
            __syncthreads();
        }
        if (xhat)
            for (int v = tid; v < n; v += 256) {
                const uint32_t w = X[v];
                for (int f = 0; f < cnt; ++f) xhat[(size_t)(f0 + f) * n + v] = (uint8_t)((w >> f) & 1u);
            }
        if (bits)
            for (int idx = tid; idx < cnt * W; idx += 256) {
                const int f = idx / W, wd = idx - f * W;
                uint32_t word = 0;
                for (int i = 0; i < 32 && wd * 32 + i < n; ++i) word |= ((X[wd * 32 + i] >> f) & 1u) << i;
                bits[(size_t)(f0 + f) * W + wd] = word;
            }
        __syncthreads();  // the next slab's load overwrites x
    }
}

// BI-AWGN: the received word is the LLR sliced at prior < 0
__global__ __launch_bounds__(256) void k_hard_slice(const float* __restrict__ pri, int64_t total, uint8_t* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) y[i] = pri[i] < 0.f ? 1 : 0;
}

constexpr size_t STATE_CAP = (size_t)1 << 30;  // streaming planes of one pass

int stream_pass(Hard* h, const uint8_t* y, int64_t B, int32_t max_iter, bool no_early, uint8_t* xhat, uint32_t* bits, int32_t* iters, hipStream_t st) {
    const Code* c = h->code;
    const int n = c->n, m = c->m;
    const int64_t E = c->E;
    const size_t NW = 2 * (size_t)n + (size_t)E + (size_t)m;
    const int nst = (int)((B + HARD_SUPER - 1) / HARD_SUPER);
    LDPC_TRY(h->state.reserve(NW * 256 * (size_t)nst));
    LDPC_TRY(h->ctl.reserve(((size_t)nst * 129 + 2) * 4));
    uint32_t* state = (uint32_t*)h->state.p;
    uint32_t* live = (uint32_t*)h->ctl.p;
    uint32_t* unsat = live + (size_t)nst * 64;
    int32_t* stlive = (int32_t*)(unsat + (size_t)nst * 64);
    uint32_t* live_tiles = (uint32_t*)(stlive + nst);
    const dim3 tiles((unsigned)((n + 63) / 64), (unsigned)nst);
    hipLaunchKernelGGL(k_hard_load, tiles, dim3(256), 0, st, y, B, n, E, m, state, c->d_col_ptr, live, unsat, stlive);
    LDPC_HIP_TRY(hipGetLastError());
    const unsigned chk_blocks = (unsigned)(((int64_t)nst * m + 3) / 4), var_blocks = (unsigned)(((int64_t)nst * n + 3) / 4);
    for (int sweep = 0;; ++sweep) {
        const bool final = sweep == max_iter;
        hipLaunchKernelGGL(k_hard_check, dim3(chk_blocks), dim3(256), 0, st, state, n, E, m, nst, c->d_row_ptr, (const int32_t*)h->vpos.p, c->d_edge_var,
                           stlive, unsat);
        LDPC_HIP_TRY(hipGetLastError());
        if (!no_early) LDPC_HIP_TRY(hipMemsetAsync(live_tiles, 0, 4, st));
        hipLaunchKernelGGL(k_hard_exit, dim3((unsigned)nst), dim3(64), 0, st, live, unsat, stlive, iters, B, sweep, final ? 1 : 0, no_early ? 1 : 0,
                           live_tiles);
        LDPC_HIP_TRY(hipGetLastError());
        if (final) break;
        if (!no_early) {  // all frames gone: the remaining sweeps would be skipped tile by tile anyway
            LDPC_HIP_TRY(hipMemcpyAsync(h->pinned, live_tiles, 4, hipMemcpyDeviceToHost, st));
            LDPC_HIP_TRY(hipStreamSynchronize(st));
            if (*h->pinned == 0u) break;
        }
        hipLaunchKernelGGL(k_hard_var, dim3(var_blocks), dim3(256), 0, st, state, n, E, m, nst, h->t, c->d_col_ptr, (const int32_t*)h->chk_of_pos.p, stlive,
                           live);
        LDPC_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_hard_unload, tiles, dim3(256), 0, st, state, B, n, E, m, xhat, bits);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace

int hard_create(Code* code, int backend, Hard** out) {
    if (backend != BK_AUTO && backend != BK_STREAM && backend != BK_FUSED) {
        set_error("ldpc_hard_create: backend must be LDPC_BACKEND_AUTO, _STREAM or _FUSED (got %d)", backend);
        return LDPC_E_ARG;
    }
    if (code->max_dv > HARD_MAX_DV) {
        set_error("ldpc_hard_create: a variable of degree %d: the vertical counters hold degrees up to %d", code->max_dv, HARD_MAX_DV);
        return LDPC_E_UNSUPPORTED;
    }
    const int64_t need = hard_lds_bytes(code->m, code->n, code->E);
    const bool fits = need <= HARD_LDS_BYTES;
    if (backend == BK_FUSED && !fits) {
        set_error("ldpc_hard_create: LDPC_BACKEND_FUSED: one slab of this code (m = %d, n = %d, E = %lld) needs %lld bytes of LDS, above one CU's "
                  "%lld; use LDPC_BACKEND_AUTO or _STREAM", code->m, code->n, (long long)code->E, (long long)need, (long long)HARD_LDS_BYTES);
        return LDPC_E_UNSUPPORTED;
    }
    LDPC_HIP_TRY(hipSetDevice(code->device));
    Hard* h = new Hard();
    h->code = code;
    h->backend = backend;
    h->lds_bytes = need;
    h->use_lds = fits && backend != BK_STREAM;
    h->last_backend = h->use_lds ? BK_FUSED : BK_STREAM;
    std::vector<int32_t> vpos((size_t)code->E), chk((size_t)code->E);
    for (int32_t v = 0; v < code->n; ++v)
        for (int32_t p = code->col_ptr[v]; p < code->col_ptr[v + 1]; ++p) {
            vpos[code->col_edge[p]] = p;
            chk[p] = code->edge_chk[code->col_edge[p]];
        }
    const size_t tab = std::max<size_t>((size_t)code->E, 1) * sizeof(int32_t);
    int rc = h->vpos.reserve(tab);
    if (rc == LDPC_OK) rc = h->chk_of_pos.reserve(tab);
    if (rc != LDPC_OK) {
        hard_destroy(h);
        return rc;
    }
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, code->device);
    if (e == hipSuccess && code->E) e = hipMemcpy(h->vpos.p, vpos.data(), (size_t)code->E * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && code->E) e = hipMemcpy(h->chk_of_pos.p, chk.data(), (size_t)code->E * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->pinned, 64, hipHostMallocDefault);
    const int64_t with_tab = need + (2 * (3 * code->E + code->m + code->n + 2) + 3) / 4 * 4;
    const char* tabs = std::getenv("LDPC_HARD_TABLES");
    h->tab_lds = tabs && !std::strcmp(tabs, "lds") && with_tab <= HARD_LDS_BYTES && code->E < 65536;
    h->launch_lds = h->tab_lds ? with_tab : need;
    if (e == hipSuccess && fits && h->launch_lds > 64 * 1024)  // above 64 KiB a workgroup's LDS has to be asked for
        e = hipFuncSetAttribute(h->tab_lds ? (const void*)k_hard_lds<true> : (const void*)k_hard_lds<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)h->launch_lds);
    if (e != hipSuccess) {
        set_error("ldpc_hard_create: device setup failed: %s", hipGetErrorString(e));
        hard_destroy(h);
        return LDPC_E_HIP;
    }
    h->num_cu = prop.multiProcessorCount;
    // 32 waves per CU = 8 workgroups of 4 waves; the LDS holds floor(160 KiB / slab) of them
    h->slabs_per_cu = fits ? (int)std::min<int64_t>(8, HARD_LDS_BYTES / h->launch_lds) : 0;
    *out = h;
    return LDPC_OK;
}

void hard_destroy(Hard* h) {
    if (!h) return;
    for (DevBuf* b : {&h->vpos, &h->chk_of_pos, &h->state, &h->ctl}) b->release();
    h->sim.release();
    if (h->pinned) (void)hipHostFree(h->pinned);
    delete h;
}

int hard_set_threshold(Hard* h, int t) {
    if (t < 0 || t > 255) {
        set_error("ldpc_hard_set_threshold: 0 <= t <= 255 (0: the majority of the extrinsic messages; got %d)", t);
        return LDPC_E_ARG;
    }
    h->t = t;
    return LDPC_OK;
}
int hard_get_threshold(const Hard* h) { return h->t; }
int hard_last_backend(const Hard* h) { return h->last_backend; }
void hard_info(const Hard* h, double* out4) {
    out4[0] = (double)(h->use_lds ? h->launch_lds : h->lds_bytes);
    out4[1] = HARD_SLAB;
    out4[2] = h->use_lds ? h->slabs_per_cu : 0;
    out4[3] = h->use_lds ? (double)h->num_cu * h->slabs_per_cu : 0;
}

int hard_decode(Hard* h, const uint8_t* y, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat, uint32_t* bits, int32_t* iters, hipStream_t st) {
    if (max_iter <= 0) {
        set_error("ldpc_hard_decode: max_iter must be >= 1 (a hard-decision decoder may oscillate for ever: it has no exit of its own; got %d)", max_iter);
        return LDPC_E_ARG;
    }
    if (flags & ~FLAG_NO_EARLY_EXIT) {
        set_error("ldpc_hard_decode: the only flag is LDPC_FLAG_NO_EARLY_EXIT (got 0x%x)", flags);
        return LDPC_E_UNSUPPORTED;
    }
    const Code* c = h->code;
    LDPC_HIP_TRY(hipSetDevice(c->device));
    h->last_backend = h->use_lds ? BK_FUSED : BK_STREAM;
    if (B == 0) return LDPC_OK;
    const bool no_early = (flags & FLAG_NO_EARLY_EXIT) != 0;
    const size_t n = (size_t)c->n, W = (n + 31) / 32;
    if (h->use_lds) {
        LDPC_TRY(h->ctl.reserve(8));
        uint32_t* dispenser = (uint32_t*)h->ctl.p;
        LDPC_HIP_TRY(hipMemsetAsync(dispenser, 0, 4, st));
        const int64_t nslabs = (B + HARD_SLAB - 1) / HARD_SLAB;
        const unsigned groups = (unsigned)std::min<int64_t>(nslabs, (int64_t)h->num_cu * h->slabs_per_cu);
        hipLaunchKernelGGL(h->tab_lds ? k_hard_lds<true> : k_hard_lds<false>, dim3(groups), dim3(256), (size_t)h->launch_lds, st, y, B, c->n, (int)c->E, c->m, h->t, max_iter, no_early ? 1 : 0,
                           c->d_row_ptr, (const int32_t*)h->vpos.p, c->d_edge_var, c->d_col_ptr, (const int32_t*)h->chk_of_pos.p, dispenser, xhat, bits,
                           iters);
        LDPC_HIP_TRY(hipGetLastError());
        return LDPC_OK;
    }
    // streaming: passes of whole supertiles whose planes fit STATE_CAP (and whose wave counts stay below 2^31)
    const size_t per_tile = (2 * n + (size_t)c->E + (size_t)c->m) * 256;
    int64_t tiles = (int64_t)std::max<size_t>(1, STATE_CAP / per_tile);
    tiles = std::min<int64_t>(tiles, ((int64_t)1 << 30) / std::max<int64_t>(1, std::max(c->n, c->m)));
    tiles = std::max<int64_t>(tiles, 1);
    const int64_t step = tiles * HARD_SUPER;
    for (int64_t b0 = 0; b0 < B; b0 += step) {
        const int64_t nb = std::min(step, B - b0);
        LDPC_TRY(stream_pass(h, y + (size_t)b0 * n, nb, max_iter, no_early, xhat ? xhat + (size_t)b0 * n : nullptr, bits ? bits + (size_t)b0 * W : nullptr,
                             iters + b0, st));
    }
    return LDPC_OK;
}

int hard_simulate(Hard* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                  uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st) {
    if (max_iter <= 0) {
        set_error("ldpc_hard_simulate: max_iter must be >= 1 (got %d)", max_iter);
        return LDPC_E_ARG;
    }
    const bool awgn = channel == CH_BIAWGN;
    const int32_t n = h->code->n;
    SimStage& s = h->sim;
    // the received bytes of one pass: about 256 MiB, whole supertiles
    const int64_t cap = std::max<int64_t>((int64_t)((((size_t)256 << 20) / (size_t)n) / HARD_SUPER * HARD_SUPER), HARD_SUPER);
    return sim_passes(
        SimCall{"ldpc_hard_simulate", h->code, codeword, frame0, B, hist_bins, counters, st},
        awgn || channel == CH_BSC ? nullptr : "LDPC_CH_BSC or LDPC_CH_BIAWGN (a hard-decision decoder has no erasures to work on)", cap,
        [&](int64_t frames) -> int { return s.reserve(frames, (size_t)n, awgn, true); },
        [&](uint64_t first, int64_t nb, const uint32_t*& bits, const int32_t*& iters) -> int {
            uint8_t* y = (uint8_t*)s.y.p;
            LDPC_TRY(channel_generate(channel, DT_F32, param, codeword, seed, stream_id, first, nb, n, awgn ? s.pri.p : nullptr, awgn ? nullptr : y, st));
            if (awgn) {  // the word sliced at prior < 0
                const int64_t total = nb * (int64_t)n;
                hipLaunchKernelGGL(k_hard_slice, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)s.pri.p, total, y);
                LDPC_HIP_TRY(hipGetLastError());
            }
            bits = (const uint32_t*)s.bits.p;
            iters = (const int32_t*)s.iters.p;
            return hard_decode(h, y, nb, max_iter, flags, nullptr, (uint32_t*)s.bits.p, (int32_t*)s.iters.p, st);
        });
}

}  // namespace ldpc

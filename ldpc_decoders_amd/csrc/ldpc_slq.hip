// Streaming layered fixed-point min-sum (include/ldpc_hip.h, ldpc_slq_*): the integer rule of ldpc_layered_fx.hpp,
// which LQMSA and QCMSA run in the LDS, on LMSA's streaming machinery (ldpc_stream.hip), for codes whose frame does not fit the LDS.
//
// State per tile of 64 frames (lane == frame), in HBM:
//     marg  [tile][n][64]   int16  the marginals in levels; the priors are quantised on load (quantise_prior: LDPC_ALG_QMSA's quantiser)
//     c2v   [tile][E][64]   int8   check -> variable messages, row-major edge order
//     xbits [tile/8][n][8]  u64    decision bit planes, eight tiles interleaved per variable (the layout of ldpc_stream.hip)
//     live  [tile]          u64    frames that are still iterating
// Every H index is wave-uniform (scalar loads, 32-bit); a marginal row is 128 bytes, a message row 64 bytes.
// One sweep = one layer pass per layer (k_slq_layer: v = marg - c2v_old, the rule (FxCheck) on the row, c2v = the new message, marg = v + c2v,
// in place; the checks of a layer share no variable) and a decision pass (k_slq_decide: sign -> planes).  Model bytes per frame-sweep:
// 6E (2 + 2 + 1 + 1 per edge) + 2n.  Early termination per frame: syndrome of the planes before every sweep, polls of the live counters
// that the host reads one behind, and a repack of the live frames into dense tiles (k_slq_repack) under the policy and the knobs of the
// floating-point streaming decoders (LDPC_STREAM_REPACK, LDPC_STREAM_REPACK_FILL).
// The tile machinery -- task order, planes, syndrome, unpack, repack policy, poll ring and the check points of the sweep loop -- is that of
// ldpc_stream.hip, shared through ldpc_tiles.hpp; the kernels of this file are the load, the passes, the repack copy and the soft output.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>

#include "ldpc_cn.hpp"
#include "ldpc_layered_fx.hpp"
#include "ldpc_repack.hpp"
#include "ldpc_slq.hpp"
#include "ldpc_tiles.hpp"

namespace ldpc {

struct SlqSet {
    DevBuf c2v, marg, planes, live, fmap;
};

struct Slq {
    Code* code = nullptr;
    FixedPoint fx;
    std::vector<int32_t> layer_of_check, layer_start;
    DevBuf order;  // int32 [m]: the checks sorted by (layer, index), the processing order
    SlqSet set[2];  // set[0] holds the state when a chunk begins, every repack moves it to the other set
    DevBuf rbase;   // repack plan: first destination slot of every source tile
    DevBuf flags;   // per-tile syndrome words + the device poll ring behind them (SweepPolls, ldpc_tiles.hpp)
    void* pinned = nullptr;  // page-locked poll ring
    hipEvent_t poll_ev[POLL_RING] = {};
    SimStage sim;   // staging of ldpc_slq_simulate
    // ldpc_slq_profile: [0] the layer passes of a sweep, [1] its decision pass, [2] a whole decode
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[3] = {0, 0, 0};
    int64_t prof_launches[3] = {0, 0, 0};
    int last_sweeps = 0, last_repacks = 0, last_chunks = 0;
};

namespace {

// ---- load: priors [B, n] (fp32 / fp64, frame-major) -> int16 marginal rows [n][64], quantised in the type they arrive in; y0 -> planes ---
template <typename T>
__global__ __launch_bounds__(256) void k_slq_load(const T* __restrict__ priors, const uint8_t* __restrict__ y0, int64_t B, int n, T step, T vmax,
                                                  int16_t* __restrict__ marg, u64* __restrict__ xbits) {
    __shared__ int16_t sp[64][66];
    __shared__ uint8_t sy[64][68];
    const int tile = blockIdx.y, v0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int f = ty; f < 64; f += 4) {
        const int64_t fr = (int64_t)tile * 64 + f;
        const int v = v0 + tx;
        int16_t val = 0;
        uint8_t yy = 0;
        if (fr < B && v < n) {
            if (y0) yy = y0[fr * n + v];
            val = (int16_t)(int)quantise_prior<T>(priors[fr * n + v], step, vmax);
        }
        sp[f][tx] = val;
        sy[f][tx] = yy;
    }
    __syncthreads();
    for (int vv = ty; vv < 64; vv += 4) {
        const int v = v0 + vv;
        if (v < n) {
            marg[((int64_t)tile * n + v) * 64 + tx] = sp[tx][vv];
            if (y0) {
                const u64 one = __ballot((sy[tx][vv] & 1u) != 0u);
                if (tx == 0) xbits[plane_at(tile, v, n)] = one;
            }
        }
    }
}

// ---- the layer pass ---------------------------------------------------------------------------------------------------------------------
// A wave takes (tile, run of the layer's checks) out of `order`; `c0` .. `c1` is the layer's range in that list; UNR checks are in flight
// together (all of one layer, hence independent).  Per edge: one marginal row (128 B) and one message row (64 B) read, one each written.
// FIRST: the first sweep, where every old message is 0: nothing is read.  `freeze`: a soft-output decode keeps the marginals of a frame
// that has left.  `dense`: as in k_layer -- where most rows are nearly DCMAX long every row is fetched unconditionally (a short check
// re-reads its last edge; the value does not enter the rule).
template <int DCMAX, int FIXED_DC, int UNR, bool FIRST>
__global__ __launch_bounds__(256) void k_slq_layer(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var,
                                                   const int32_t* __restrict__ order, int8_t* c2v, int16_t* marg, const u64* __restrict__ live, int m,
                                                   int n, int64_t E, int tiles, int chunks, int cpw, int c0, int c1, int xcd_aware, int freeze,
                                                   int scale64, int offset, int V) {
    const int lane = threadIdx.x;
    int tile, chunk;
    if (!task_of(tiles, chunks, xcd_aware, &tile, &chunk)) return;
    const u64 lv = live[tile];
    if (lv == 0) return;
    const bool on = freeze ? (bool)((lv >> lane) & 1ull) : true;
    if (!on) return;  // (no wave-wide operation below)
    const bool dense = FIXED_DC > 0 || (DCMAX <= 8 && E * 4 >= (int64_t)m * DCMAX * 3);  // (wave-uniform)
    int8_t* ct = c2v + (int64_t)tile * E * 64 + lane;
    int16_t* mt = marg + (int64_t)tile * n * 64 + lane;
    const int i_end = min(c1, c0 + (chunk + 1) * cpw);
    for (int i = c0 + chunk * cpw; i < i_end; i += UNR) {
        int v[UNR][DCMAX];
        [[maybe_unused]] int w[UNR][DCMAX];
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
                    if constexpr (!FIRST) w[u][j] = __builtin_nontemporal_load(ct + (int64_t)kk * 64);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
#pragma unroll
                for (int j = 0; j < DCMAX; ++j) {
                    v[u][j] = 0;
                    if constexpr (!FIRST) w[u][j] = 0;
                    if (j < deg[u]) {
                        v[u][j] = mt[(int64_t)edge_var[k0[u] + j] * 64];
                        if constexpr (!FIRST) w[u][j] = __builtin_nontemporal_load(ct + (int64_t)(k0[u] + j) * 64);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            FxCheck k(V);
#pragma unroll
            for (int j = 0; j < DCMAX; ++j) {
                if constexpr (!FIRST) v[u][j] -= w[u][j];
                if (j < deg[u]) k.take(j, v[u][j], V);
            }
            k.finish(scale64, offset);
#pragma unroll
            for (int j = 0; j < DCMAX; ++j) {
                if (j < deg[u]) {
                    const int c = k.out(j, v[u][j]);
                    __builtin_nontemporal_store((int8_t)c, ct + (int64_t)(k0[u] + j) * 64);
                    mt[(int64_t)edge_var[k0[u] + j] * 64] = (int16_t)(v[u][j] + c);
                }
            }
        }
    }
}

// Checks of more than 64 variables: one check at a time, its rows read twice (minima, then messages) instead of held in registers.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_slq_layer_wide(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var,
                                                        const int32_t* __restrict__ order, int8_t* c2v, int16_t* marg, const u64* __restrict__ live,
                                                        int m, int n, int64_t E, int tiles, int chunks, int cpw, int c0, int c1, int xcd_aware,
                                                        int freeze, int scale64, int offset, int V) {
    const int lane = threadIdx.x;
    int tile, chunk;
    if (!task_of(tiles, chunks, xcd_aware, &tile, &chunk)) return;
    const u64 lv = live[tile];
    if (lv == 0) return;
    const bool on = freeze ? (bool)((lv >> lane) & 1ull) : true;
    if (!on) return;
    int8_t* ct = c2v + (int64_t)tile * E * 64 + lane;
    int16_t* mt = marg + (int64_t)tile * n * 64 + lane;
    const int i_end = min(c1, c0 + (chunk + 1) * cpw);
    for (int i = c0 + chunk * cpw; i < i_end; ++i) {
        const int cc = order[i];
        const int k0 = row_ptr[cc], deg = row_ptr[cc + 1] - k0;
        FxCheck k(V);
        for (int j = 0; j < deg; ++j) {
            int v = mt[(int64_t)edge_var[k0 + j] * 64];
            if constexpr (!FIRST) v -= (int)ct[(int64_t)(k0 + j) * 64];
            k.take(j, v, V);
        }
        k.finish(scale64, offset);
        for (int j = 0; j < deg; ++j) {
            int16_t* mp = mt + (int64_t)edge_var[k0 + j] * 64;
            int v = *mp;
            if constexpr (!FIRST) v -= (int)ct[(int64_t)(k0 + j) * 64];
            const int c = k.out(j, v);
            ct[(int64_t)(k0 + j) * 64] = (int8_t)c;
            *mp = (int16_t)(v + c);
        }
    }
}

// Decision pass: marginals -> decision bit planes, behind the last layer of a sweep.  The words keep the bits of the frames that have left.
__global__ __launch_bounds__(256) void k_slq_decide(const int16_t* __restrict__ marg, const u64* __restrict__ live, u64* __restrict__ xbits, int n,
                                                    int tiles, int chunks, int vpw, int xcd_aware) {
    const int lane = threadIdx.x;
    int tile, chunk;
    if (!task_of(tiles, chunks, xcd_aware, &tile, &chunk)) return;
    const u64 lv = live[tile];
    if (lv == 0) return;
    const int16_t* mt = marg + (int64_t)tile * n * 64 + lane;
    u64* xb = xbits + plane_at(tile, 0, n);  // word of variable v at xb[8 * v]
    const int v_end = min(n, (chunk + 1) * vpw);
    constexpr int G = 8;  // rows in flight: a 128-byte row per load, the ballots behind them
    for (int v0 = chunk * vpw; v0 < v_end; v0 += G) {
        int16_t x[G];
#pragma unroll
        for (int u = 0; u < G; ++u) x[u] = mt[(int64_t)min(v0 + u, v_end - 1) * 64];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int v = v0 + u;
            if (v < v_end) {  // (wave-uniform)
                const u64 one = __ballot(x[u] < 0);
                u64 merged = one;
                if (lv != ~0ull) merged = (uniform_ld64(xb + 8 * v) & ~lv) | (one & lv);
                if (lane == 0) xb[8 * v] = merged;
            }
        }
    }
}

// soft output: the marginal rows start as the levels, so a frame that never swept (iters == 0) reports 0
__global__ void k_slq_soft_out(const int16_t* __restrict__ marg, const int32_t* __restrict__ iters, int16_t* __restrict__ out, int64_t B, int n) {
    const int tile = blockIdx.y, lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t fr = (int64_t)tile * 64 + lane;
    if (v < n && fr < B) out[fr * n + v] = iters[fr] > 0 ? marg[((int64_t)tile * n + v) * 64 + lane] : (int16_t)0;
}

// ---- frame repack (ldpc_repack.hpp): the separate copy kernel for the two integer types ------------------------------------------------
// destination lane j reads (source tile, source lane) of the j-th live frame: message rows, then per variable the marginal row and one
// plane word; lanes beyond the live frames get zeros
__global__ __launch_bounds__(256) void k_slq_repack(const int8_t* __restrict__ msg_src, int8_t* __restrict__ msg_dst, const int16_t* __restrict__ marg_src,
                                                    int16_t* __restrict__ marg_dst, const u64* __restrict__ xb_src, u64* __restrict__ xb_dst,
                                                    const u64* __restrict__ live_src, u64* __restrict__ live_dst, const int32_t* __restrict__ base,
                                                    const int32_t* __restrict__ frame_src, int32_t* __restrict__ frame_dst, int tiles_src, int n,
                                                    int64_t E, int rows_per_wave) {
    const int lane = threadIdx.x;
    const int dt = blockIdx.y;  // destination tile
    int st, sl;
    const bool has = repack_source(base, live_src, tiles_src, dt * 64 + lane, &st, &sl);
    const int chunk = blockIdx.x * 4 + threadIdx.y;
    const int64_t rows = E + n;
    const int64_t r0 = (int64_t)chunk * rows_per_wave, r1 = min(rows, r0 + rows_per_wave);
    const int8_t* ms = msg_src + (int64_t)st * E * 64 + sl;
    int8_t* md = msg_dst + (int64_t)dt * E * 64 + lane;
    const int64_t so = (int64_t)st * n * 64 + sl, dof = (int64_t)dt * n * 64 + lane;
    for (int64_t r = r0; r < r1; ++r) {
        if (r < E) {
            md[r * 64] = has ? ms[r * 64] : (int8_t)0;
        } else {
            const int64_t v = r - E;
            marg_dst[dof + v * 64] = has ? marg_src[so + v * 64] : (int16_t)0;
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

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// the arguments of one chunk of a decode: every pointer already points at the chunk's first frame
struct SlqCall {
    const void* priors;
    const uint8_t* y0;
    int64_t B;
    int32_t max_iter;
    uint32_t flags;
    uint8_t* xhat;
    uint32_t* bits;
    int32_t* iters;
    int16_t* soft;
    hipStream_t stream;
};

struct SlqGeometry {
    int tiles, cpw, vn_chunks, vpw, xcd_aware, freeze;
    int scale64, offset, vmax;
};

// Degree classes of the layer pass, those of ldpc_stream.hip's check_class -- regular dc = 6; degrees up to 6; else the next power of two
// up to 64 -- and the two-pass kernel above 64.  Checks in flight per wave: about 32 VGPRs of rows.
template <int DCMAX, int FDC>
void launch_layers(const Slq* h, int8_t* c2v, int16_t* marg, const u64* live, const SlqGeometry& g, bool first, hipStream_t st) {
    const Code* c = h->code;
    constexpr int UNR = DCMAX <= 8 ? 4 : (DCMAX <= 16 ? 2 : 1);
    void (*kern)(const int32_t*, const int32_t*, const int32_t*, int8_t*, int16_t*, const u64*, int, int, int64_t, int, int, int, int, int, int, int, int, int, int);
    if constexpr (DCMAX > 64)
        kern = first ? k_slq_layer_wide<true> : k_slq_layer_wide<false>;
    else
        kern = first ? k_slq_layer<DCMAX, FDC, UNR, true> : k_slq_layer<DCMAX, FDC, UNR, false>;
    for (size_t l = 0; l + 1 < h->layer_start.size(); ++l) {
        const int c0 = h->layer_start[l], c1 = h->layer_start[l + 1];
        const int chunks = (c1 - c0 + g.cpw - 1) / g.cpw;
        hipLaunchKernelGGL(kern, dim3(task_blocks(g.tiles, chunks, g.xcd_aware)), dim3(64, 4), 0, st, c->d_row_ptr, c->d_edge_var, (const int32_t*)h->order.p,
                           c2v, marg, live, c->m, c->n, c->E, g.tiles, chunks, g.cpw, c0, c1, g.xcd_aware, g.freeze, g.scale64, g.offset, g.vmax);
    }
}
void dispatch_layers(const Slq* h, int8_t* c2v, int16_t* marg, const u64* live, const SlqGeometry& g, bool first, hipStream_t st) {
    const Code* c = h->code;
    if (c->min_dc == c->max_dc && c->max_dc == 6) return launch_layers<6, 6>(h, c2v, marg, live, g, first, st);
    if (c->max_dc > 4 && c->max_dc <= 6) return launch_layers<6, 0>(h, c2v, marg, live, g, first, st);
    if (c->max_dc <= 4) return launch_layers<4, 0>(h, c2v, marg, live, g, first, st);
    if (c->max_dc <= 8) return launch_layers<8, 0>(h, c2v, marg, live, g, first, st);
    if (c->max_dc <= 16) return launch_layers<16, 0>(h, c2v, marg, live, g, first, st);
    if (c->max_dc <= 32) return launch_layers<32, 0>(h, c2v, marg, live, g, first, st);
    if (c->max_dc <= 64) return launch_layers<64, 0>(h, c2v, marg, live, g, first, st);
    return launch_layers<65, 0>(h, c2v, marg, live, g, first, st);
}

int slq_event(Slq* h, size_t idx, hipEvent_t* out) {
    while (h->ev_pool.size() <= idx) {
        hipEvent_t e;
        LDPC_HIP_TRY(hipEventCreate(&e));
        h->ev_pool.push_back(e);
    }
    *out = h->ev_pool[idx];
    return LDPC_OK;
}

int64_t workspace_bytes() {
    if (const char* e = std::getenv("LDPC_SLQ_WORKSPACE_MB")) {
        const long long mb = atoll(e);
        if (mb > 0) return (int64_t)mb << 20;
    }
    return SLQ_WORKSPACE_BYTES;
}
// tiles per chunk: a chunk's state (marginals, messages, planes) twice -- the set in use and a repack target -- within the bound; at least
// one tile, at most 2^15 (grid dimensions, the one-workgroup repack plan)
int chunk_tiles(const Code* c) {
    const int64_t per_tile = 64 * slq_state_bytes(c->n, c->E) + 8 * (int64_t)c->n + 1024;
    return (int)std::min<int64_t>(std::max<int64_t>(workspace_bytes() / (2 * per_tile), 1), 1 << 15);
}

// One chunk of frames: the sweep loop of ldpc_stream.hip's run<T, ALG_LMSA>, its check points those of SweepPolls (ldpc_tiles.hpp).
// `prof_next`: first free profile event of the pool.
template <typename T>
int run_chunk(Slq* h, const SlqCall& k, size_t* prof_next, std::vector<hipEvent_t>* spans, int* sweeps_out, int* repacks_out) {
    const Code* c = h->code;
    const int n = c->n, m = c->m;
    const int64_t E = c->E, B = k.B;
    const hipStream_t st = k.stream;
    const int tiles = (int)((B + 63) / 64);
    const bool early = !(k.flags & FLAG_NO_EARLY_EXIT);
    RepackPolicy repack(early && k.soft == nullptr && tiles >= 2);

    SlqSet* const set = h->set;
    LDPC_TRY(set[0].c2v.reserve((size_t)tiles * E * 64));
    LDPC_TRY(set[0].marg.reserve((size_t)tiles * n * 64 * sizeof(int16_t)));
    LDPC_TRY(set[0].planes.reserve(plane_words(tiles, n) * 8));
    LDPC_TRY(set[0].live.reserve((size_t)tiles * 8));
    LDPC_TRY(h->flags.reserve((size_t)tiles * 16 + 64 + POLL_RING_BYTES));
    if (repack.on) {
        const size_t nt = repack.target_tiles(tiles);  // second state set
        if (set[1].c2v.reserve(nt * E * 64) || set[1].marg.reserve(nt * n * 64 * sizeof(int16_t)) || set[1].planes.reserve(plane_words((int)nt, n) * 8) ||
            set[1].live.reserve(nt * 8) || set[1].fmap.reserve(nt * 64 * sizeof(int32_t)) || set[0].fmap.reserve(nt * 64 * sizeof(int32_t)) ||
            h->rbase.reserve(((size_t)tiles + 1) * sizeof(int32_t)))
            repack.on = false;  // no room for a second set: decode without repacking
    }
    int cur = 0;
    int8_t* msg;
    int16_t* marg;
    u64 *xbits, *live;
    int32_t* fmap = nullptr;  // frame index of (tile, lane); null = identity (never repacked)
    auto use_set = [&](int s) {
        cur = s;
        msg = (int8_t*)set[s].c2v.p;
        marg = (int16_t*)set[s].marg.p;
        xbits = (u64*)set[s].planes.p;
        live = (u64*)set[s].live.p;
    };
    use_set(0);
    u64* tflags = (u64*)h->flags.p;  // [tiles][2], the device poll ring behind them

    SlqGeometry g;
    g.tiles = tiles;
    g.freeze = k.soft != nullptr ? 1 : 0;
    g.scale64 = h->fx.scale64();
    g.offset = h->fx.clamped_offset();
    g.vmax = h->fx.vmax();
    // nodes per wave: many short wave tasks in tile-major order, as measured for the floating-point passes; longer runs only beyond 2^22
    // tasks per launch (measured here too, 32 768 frames of (3,6) n = 64 800, ten sweeps: 4 / 8 / 16 checks per wave 73.1 / 74.9 / 76.0 ms of
    // layer passes; 16 .. 128 variables per wave 12.8 .. 12.6 ms of decision passes)
    auto per_wave = [&](int nodes, int base) {
        long v = base;
        while ((long)((nodes + v - 1) / v) * tiles > (1L << 22) && v < 256) v *= 2;
        return (int)(v > nodes ? ((nodes + 3) / 4 * 4) : v);
    };
    g.cpw = per_wave(m, 4);
    g.vpw = per_wave(n, 16);
    g.vn_chunks = (n + g.vpw - 1) / g.vpw;
    g.xcd_aware = (size_t)n * 64 * sizeof(int16_t) <= ((size_t)4 << 20) ? 1 : 0;  // a tile's marginal rows fit one XCD's L2

    LDPC_HIP_TRY(hipMemsetAsync(xbits, 0, plane_words(tiles, n) * 8, st));
    LDPC_HIP_TRY(hipMemsetAsync(tflags, 0, (size_t)tiles * 16 + 64 + POLL_RING_BYTES, st));
    LDPC_HIP_TRY(hipMemsetAsync(k.iters, 0, (size_t)B * sizeof(int32_t), st));
    hipLaunchKernelGGL((k_slq_load<T>), dim3((n + 63) / 64, tiles), dim3(256), 0, st, (const T*)k.priors, k.y0, B, n, (T)h->fx.step(), (T)g.vmax, marg, xbits);
    tiles_init_live(live, B, tiles, st);

    const int cap = k.max_iter > 0 ? k.max_iter : 100000;
    const double bytes_per_frame = 6.0 * E + 2.0 * n;
    SweepPolls p{st, (int*)((char*)h->flags.p + (size_t)tiles * 16 + 64), (volatile int*)h->pinned, h->poll_ev, repack, cap, tiles, bytes_per_frame};
    p.poll_every = SweepPolls::poll_every_300us(tiles, bytes_per_frame);
    p.every_sweep = p.eager = k.max_iter <= 0;  // an unbounded run polls at every sweep and reads at once
    const auto syndrome = [&](int* slot_dev) { tiles_syndrome(c, xbits, live, tflags, k.iters, slot_dev, B, p.cur_tiles, p.sweeps, fmap, st); };
    const auto repack_into = [&](int nt) {
        const SlqSet& to = set[1 - cur];
        // the decisions of every frame of the old tiles (those that left keep them; the moved ones overwrite theirs later)
        tiles_unpack(xbits, k.xhat, k.bits, B, n, p.cur_tiles, fmap, st);
        hipLaunchKernelGGL(k_repack_plan, dim3(1), dim3(1024), 0, st, live, p.cur_tiles, (int32_t*)h->rbase.p);
        const int rows_per_wave = 128;
        const int chunks = (int)((E + n + rows_per_wave - 1) / rows_per_wave);
        hipLaunchKernelGGL(k_slq_repack, dim3((chunks + 3) / 4, nt), dim3(64, 4), 0, st, msg, (int8_t*)to.c2v.p, marg, (int16_t*)to.marg.p, xbits,
                           (u64*)to.planes.p, live, (u64*)to.live.p, (const int32_t*)h->rbase.p, fmap, (int32_t*)to.fmap.p, p.cur_tiles, n, E, rows_per_wave);
        use_set(1 - cur);
        fmap = (int32_t*)to.fmap.p;
        g.tiles = nt;
        return nt;
    };
    for (int it = 0; it < cap && !p.all_left; ++it) {
        if (early && (it > 0 || k.y0 != nullptr)) {
            LDPC_TRY(p.check_point(it, syndrome, repack_into));
            if (p.all_left) break;
        }
        hipEvent_t e[3] = {};
        if (h->profile) {
            for (hipEvent_t& x : e) LDPC_TRY(slq_event(h, (*prof_next)++, &x));
            LDPC_HIP_TRY(hipEventRecord(e[0], st));
        }
        dispatch_layers(h, msg, marg, live, g, it == 0, st);
        if (h->profile) LDPC_HIP_TRY(hipEventRecord(e[1], st));
        hipLaunchKernelGGL(k_slq_decide, dim3(task_blocks(g.tiles, g.vn_chunks, g.xcd_aware)), dim3(64, 4), 0, st, marg, live, xbits, n, g.tiles, g.vn_chunks,
                           g.vpw, g.xcd_aware);
        if (h->profile) {
            LDPC_HIP_TRY(hipEventRecord(e[2], st));
            spans->insert(spans->end(), e, e + 3);
        }
        ++p.sweeps;
    }
    tiles_finish_iters(live, k.iters, B, p.cur_tiles, p.sweeps, fmap, st);
    tiles_unpack(xbits, k.xhat, k.bits, B, n, p.cur_tiles, fmap, st);
    // (a soft-output decode never repacks: `marg` is set 0 in the identity tiling)
    if (k.soft) hipLaunchKernelGGL(k_slq_soft_out, dim3((n + 3) / 4, tiles), dim3(256), 0, st, marg, (const int32_t*)k.iters, k.soft, B, n);
    LDPC_TRY(p.finish());  // (before the next chunk or call reuses the slots)
    LDPC_HIP_TRY(hipGetLastError());
    *sweeps_out = p.sweeps;
    *repacks_out = p.repacks;
    return LDPC_OK;
}

// the layering (host side) and its device mirror
int install(Slq* h, const int32_t* layer_of_check) {
    const Code* c = h->code;
    std::vector<int32_t> of_check, sorted, start;
    LDPC_TRY(layering_build(c, layer_of_check, &of_check, &sorted, &start));
    // a decode of this handle still in flight reads the old order
    LDPC_HIP_TRY(hipSetDevice(c->device));
    LDPC_HIP_TRY(hipDeviceSynchronize());
    LDPC_TRY(h->order.reserve(std::max<size_t>(sorted.size(), 1) * sizeof(int32_t)));
    if (!sorted.empty()) LDPC_HIP_TRY(hipMemcpy(h->order.p, sorted.data(), sorted.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    h->layer_of_check.swap(of_check);
    h->layer_start.swap(start);
    return LDPC_OK;
}

}  // namespace

int slq_create(Code* code, Slq** out) {
    LDPC_TRY(fx_check_degrees("ldpc_slq_create", "check", code->min_dc, code->max_dv, SLQ_MAX_DV));
    LDPC_HIP_TRY(hipSetDevice(code->device));
    Slq* h = new Slq();
    h->code = code;
    hipError_t e = hipHostMalloc(&h->pinned, 256, hipHostMallocDefault);
    for (int i = 0; i < POLL_RING && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->poll_ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        set_error("ldpc_slq_create: device setup failed: %s", hipGetErrorString(e));
        slq_destroy(h);
        return LDPC_E_HIP;
    }
    const int rc = install(h, nullptr);
    if (rc != LDPC_OK) {
        slq_destroy(h);
        return rc;
    }
    *out = h;
    return LDPC_OK;
}

void slq_destroy(Slq* h) {
    if (!h) return;
    for (SlqSet& s : h->set)
        for (DevBuf* b : {&s.c2v, &s.marg, &s.planes, &s.live, &s.fmap}) b->release();
    for (DevBuf* b : {&h->order, &h->rbase, &h->flags}) b->release();
    h->sim.release();
    for (hipEvent_t e : h->poll_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    if (h->pinned) (void)hipHostFree(h->pinned);
    delete h;
}

int slq_set_fixed_point(Slq* h, int bits, int frac_bits, double scale, int offset) {
    return h->fx.set("ldpc_slq_set_fixed_point", bits, frac_bits, scale, offset);
}

void slq_get_fixed_point(const Slq* h, int* bits, int* frac_bits, double* scale, int* offset) { h->fx.get(bits, frac_bits, scale, offset); }

int slq_set_layers(Slq* h, const int32_t* layer_of_check, int32_t m) {
    if (layer_of_check && m != h->code->m) {
        set_error("ldpc_slq_set_layers: %d entries for a code of %d checks", m, h->code->m);
        return LDPC_E_ARG;
    }
    return install(h, layer_of_check);
}

void slq_get_layers(const Slq* h, int32_t* nlayers, int32_t* layer_of_check) {
    *nlayers = (int32_t)h->layer_start.size() - 1;
    if (layer_of_check) std::copy(h->layer_of_check.begin(), h->layer_of_check.end(), layer_of_check);
}

void slq_info(const Slq* h, double* out4) {
    out4[0] = (double)slq_state_bytes(h->code->n, h->code->E);
    out4[1] = chunk_tiles(h->code);
    out4[2] = (double)h->layer_start.size() - 1;
    out4[3] = (double)h->layer_start.size();  // one launch per layer and the decision pass
}

void slq_profile(Slq* h, int enable, double* ms3, int64_t* launches3, int reset) {
    if (enable >= 0) h->profile = enable != 0;
    for (int i = 0; i < 3; ++i) {
        if (ms3) ms3[i] = h->prof_ms[i];
        if (launches3) launches3[i] = h->prof_launches[i];
        if (reset) {
            h->prof_ms[i] = 0;
            h->prof_launches[i] = 0;
        }
    }
}

void slq_last_stats(const Slq* h, int32_t* out3) {
    out3[0] = h->last_sweeps;
    out3[1] = h->last_repacks;
    out3[2] = h->last_chunks;
}

int slq_decode(Slq* h, int dtype, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat, uint32_t* bits,
               int32_t* iters, int16_t* soft, hipStream_t st) {
    LDPC_TRY(fx_check_decode("ldpc_slq_decode", dtype, flags, B));
    const Code* c = h->code;
    LDPC_HIP_TRY(hipSetDevice(c->device));
    h->last_sweeps = h->last_repacks = h->last_chunks = 0;
    if (B == 0) return LDPC_OK;
    const size_t n = (size_t)c->n, W = (n + 31) / 32, esz = dtype == DT_F64 ? sizeof(double) : sizeof(float);
    // chunks of equal size (a short last chunk would run its sweeps on a nearly empty chip)
    const int64_t tiles = (B + 63) / 64, cap = chunk_tiles(c);
    const int64_t nchunks = (tiles + cap - 1) / cap, per = (tiles + nchunks - 1) / nchunks * 64;
    size_t prof_next = 0;
    std::vector<hipEvent_t> spans;
    hipEvent_t whole[2] = {};
    if (h->profile) {
        for (hipEvent_t& x : whole) LDPC_TRY(slq_event(h, prof_next++, &x));
        LDPC_HIP_TRY(hipEventRecord(whole[0], st));
    }
    for (int64_t b0 = 0; b0 < B; b0 += per) {
        SlqCall k;
        k.priors = (const char*)priors + (size_t)b0 * n * esz;
        k.y0 = y0 ? y0 + (size_t)b0 * n : nullptr;
        k.B = std::min(per, B - b0);
        k.max_iter = max_iter;
        k.flags = flags;
        k.xhat = xhat ? xhat + (size_t)b0 * n : nullptr;
        k.bits = bits ? bits + (size_t)b0 * W : nullptr;
        k.iters = iters + b0;
        k.soft = soft ? soft + (size_t)b0 * n : nullptr;
        k.stream = st;
        int sweeps = 0, repacks = 0;
        LDPC_TRY(dtype == DT_F64 ? run_chunk<double>(h, k, &prof_next, &spans, &sweeps, &repacks)
                                 : run_chunk<float>(h, k, &prof_next, &spans, &sweeps, &repacks));
        h->last_sweeps = std::max(h->last_sweeps, sweeps);
        h->last_repacks += repacks;
        h->last_chunks += 1;
    }
    if (h->profile) {
        LDPC_HIP_TRY(hipEventRecord(whole[1], st));
        LDPC_HIP_TRY(hipStreamSynchronize(st));
        float ms = 0.f;
        for (size_t i = 0; i + 2 < spans.size(); i += 3)
            for (int kind = 0; kind < 2; ++kind) {
                LDPC_HIP_TRY(hipEventElapsedTime(&ms, spans[i + kind], spans[i + kind + 1]));
                h->prof_ms[kind] += ms;
                h->prof_launches[kind] += 1;
            }
        LDPC_HIP_TRY(hipEventElapsedTime(&ms, whole[0], whole[1]));
        h->prof_ms[2] += ms;
        h->prof_launches[2] += 1;
    }
    return LDPC_OK;
}

int slq_simulate(Slq* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                 uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st) {
    // the fp32 priors of one pass: a third of the workspace bound, whole state chunks where one fits
    const int64_t fit = std::max<int64_t>(workspace_bytes() / 3 / (int64_t)((size_t)h->code->n * sizeof(float)), 1), ct = (int64_t)chunk_tiles(h->code) * 64;
    return fx_simulate("ldpc_slq_simulate", h->code, h->sim, fit >= ct ? fit / ct * ct : fit, channel, param, codeword, seed, stream_id, frame0, B,
                       hist_bins, counters, st, [&](const void* pri, const uint8_t* y, int64_t nb, uint32_t* bits, int32_t* iters) {
                           return slq_decode(h, DT_F32, pri, y, nb, max_iter, flags, nullptr, bits, iters, nullptr, st);
                       });
}

}  // namespace ldpc

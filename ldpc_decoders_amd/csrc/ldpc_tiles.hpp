// The tile machinery of the streaming decoders, stated once for ldpc_stream.hip (fp32 / fp64 run<T, ALG>, fp16 storage run16<ALG>) and
// ldpc_slq.hip (SLQMSA run_chunk<T>): 64 frames per tile (lane == frame), decision bit planes, live words, a syndrome pass that votes frames
// out, live counters the host polls from a ring, and a repack of thinning batches into dense tiles.  Here: the device helpers of the tile
// layout, the launchers of the six bookkeeping kernels (the kernels themselves live in ldpc_stream.hip), the repack policy and the poll /
// repack protocol of the sweep loop.  What a decoder keeps to itself: its reservations, its geometry, its load and pass kernels, its repack
// kernels and its profile marks.  (ldpc_admm.hip and ldpc_bec_stream.hip poll at a different point of their loops and share only ldpc_repack.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <vector>

#include "ldpc_common.hpp"

namespace ldpc {

using u64 = unsigned long long;

// ---- device helpers -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 wave_or(u64 x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)(x & 0xffffffffull), off, 64);
        const unsigned hi = __shfl_xor((unsigned)(x >> 32), off, 64);
        x |= ((u64)hi << 32) | lo;
    }
    return x;
}

// Wave task -> (tile, chunk of nodes).  XCD-aware (MI355X_MICROARCH.md: block b runs on XCD b % 8, each XCD has its own L2): the
// blocks of ONE tile all carry the same b % 8, so the marginal lines a check pass re-reads (each is used by dv checks of the tile)
// are re-read through ONE L2 instead of up to dv different ones.  Grid = 8 x ceil(tiles / 8) x blocks per tile (4 waves per block).
__device__ __forceinline__ bool task_of(int tiles, int chunks, int xcd_aware, int* tile, int* chunk) {
    const int q = blockIdx.x, w = threadIdx.y;
    if (xcd_aware) {
        const int bpt = (chunks + 3) >> 2;
        const int x = q & 7, local = q >> 3;
        const int tl = local / bpt, cb = local - tl * bpt;
        *tile = __builtin_amdgcn_readfirstlane(tl * 8 + x);
        *chunk = __builtin_amdgcn_readfirstlane(cb * 4 + w);
    } else {
        const int task = q * 4 + w;
        *tile = __builtin_amdgcn_readfirstlane(task / chunks);
        *chunk = __builtin_amdgcn_readfirstlane(task - (task / chunks) * chunks);
    }
    return *tile < tiles && *chunk < chunks;
}
__host__ inline int task_blocks(int tiles, int chunks, int xcd_aware) {
    return xcd_aware ? 8 * ((tiles + 7) / 8) * ((chunks + 3) / 4) : (int)(((long)tiles * chunks + 3) / 4);
}

// Wave-uniform 8-byte read through the SCALAR cache (constant address space: the compiler emits s_load_dwordx2, counted by lgkmcnt and
// therefore independent of the vector loads and stores in flight).  Only for words no wave writes before this wave has read them in the
// same launch: the decision word of (tile, variable) is read and then written by exactly one wave per sweep.
__device__ __forceinline__ u64 uniform_ld64(const u64* p) {
    typedef const __attribute__((address_space(4))) u64* cptr;
    return *(cptr)(uintptr_t)p;
}
// index of the bit-plane word of (tile, variable): eight tiles interleaved per variable
__host__ __device__ __forceinline__ int64_t plane_at(int tile, int64_t v, int n) { return ((int64_t)(tile >> 3) * n + v) * 8 + (tile & 7); }
__host__ inline size_t plane_words(int tiles, int n) { return (size_t)((tiles + 7) / 8) * n * 8; }

// ---- the bookkeeping kernels of ldpc_stream.hip, by launcher ---------------------------------------------------------------------------
// live words of a batch of B frames in `tiles` tiles
void tiles_init_live(u64* live, int64_t B, int tiles, hipStream_t st);
// syndrome of the decisions of `tiles` tiles: frames that satisfy every check leave (live bit cleared, iters = sweeps); with `poll_dev`
// the tiles that still hold a live frame and the live frames are added into poll_dev[0], poll_dev[1]
void tiles_syndrome(const Code* c, const u64* xbits, u64* live, u64* tflags, int32_t* iters, int* poll_dev, int64_t B, int tiles, int sweeps,
                    const int32_t* fmap, hipStream_t st);
// decisions of the frames of `tiles` tiles as packed words [B, ceil(n / 32)] and / or bytes [B, n]: whichever is not null
void tiles_unpack(const u64* xbits, uint8_t* xhat, uint32_t* bits, int64_t B, int n, int tiles, const int32_t* fmap, hipStream_t st);
// frames still live when the loop ends: iters = sweeps
void tiles_finish_iters(const u64* live, int32_t* iters, int64_t B, int tiles, int sweeps, const int32_t* fmap, hipStream_t st);

// ---- host side: repack policy and the poll / repack protocol of a sweep loop -----------------------------------------------------------
// Frame repack (ldpc_repack.hpp): decodes with early exit and without soft output.  Policy: at a poll, when the live frames would fill less
// than `fill` of the tiles that still hold one, gather them into dense tiles -- a repack moves (E + 2n) lines per tile once, a sweep
// moves about (3E + 3n), so it pays as soon as about one more sweep follows.  Read from the environment at the top of every decode:
// LDPC_STREAM_REPACK=0 switches it off, LDPC_STREAM_REPACK_FILL is clamped to [0, 0.95] (negative or NaN: 0, which never repacks).
struct RepackPolicy {
    bool on;
    double fill = 0.75;
    explicit RepackPolicy(bool eligible) : on(eligible) {
        if (const char* e = std::getenv("LDPC_STREAM_REPACK")) on = on && atoi(e) != 0;
        if (const char* e = std::getenv("LDPC_STREAM_REPACK_FILL")) fill = atof(e);
        if (fill > 0.95) fill = 0.95;
        if (!(fill >= 0.0)) fill = 0.0;
    }
    // (a "rent or buy" schedule -- repack once the tile-sweeps spent on departed lanes reach the cost of a repack -- was measured within
    // the run-to-run spread of this rule in round 5 and removed in round 6: HISTORY.md)
    bool wants(int live_tiles, int live_frames) const { return live_tiles >= 2 && (double)live_frames <= fill * 64.0 * live_tiles; }
    // tiles of the second state set: the first repack fires at <= fill * 64 live frames per tile, later ones only shrink
    size_t target_tiles(int tiles) const { return (size_t)(fill * tiles) + 2; }
};

// One poll of the live counters, in flight: the syndrome kernels of a check point add the live tiles / frames into `slot` of the
// device ring, a copy brings them to the pinned ring, an event marks it.  The host reads poll k only after it has enqueued the work
// up to poll k + 1, so the GPU never waits for the host inside the sweep loop.
struct PendingPoll {
    int slot, it, sweeps;
    bool tiling_current;  // false once a repack has been enqueued after this poll: its counts no longer describe the tiling
};
constexpr int POLL_RING = 4;
constexpr size_t POLL_RING_BYTES = POLL_RING * 16;  // [POLL_RING][4] ints: live tiles, live frames

// streaming work of one sweep over `tiles` tiles, in microseconds at 5 TB/s
inline double sweep_us(int tiles, double bytes_per_frame) { return (double)tiles * 64.0 * bytes_per_frame / 5.0e6; }

// The check points of a sweep loop.  The decoder's loop is
//     for (it = 0; it < cap && !p.all_left; ++it) { if (a check is due) { p.check_point(it, ...); if (p.all_left) break; }  passes;  ++p.sweeps; }
//     ... outputs ...;  p.finish();
// and the decoder hands check_point two callables: syndrome(slot_dev) launches the syndrome of the current tiling (p.cur_tiles tiles, p.sweeps
// sweeps; slot_dev: where the live counters go, null at a check point without a poll) and repack_into(nt) enqueues the repack of the live
// frames into nt dense tiles, flips the decoder's state set and returns the tile count of the new tiling.
struct SweepPolls {
    hipStream_t st;
    int* ring_dev;             // device ring (behind the per-tile syndrome words of the decoder's flags buffer)
    volatile int* ring_host;   // the same, page-locked
    const hipEvent_t* ev;      // [POLL_RING]
    RepackPolicy repack;
    int cap;                   // sweeps at most
    int cur_tiles;             // tiles of the current tiling
    double bytes_per_frame;    // streaming bytes of a frame-sweep: behind poll_every_300us and the long-sweep rule below
    int poll_every = 1;        // a poll at every poll_every-th check point ...
    bool every_sweep = false;  // ... or at all of them
    bool eager = false;        // every poll is read at once
    int polls = 0, sweeps = 0, repacks = 0;
    bool all_left = false;
    std::vector<PendingPoll> pending = {};

    // a poll about every 300 us of streaming work
    static int poll_every_300us(int tiles, double bytes_per_frame) {
        const int e = (int)(300.0 / (15.0 + sweep_us(tiles, bytes_per_frame)));
        return e < 1 ? 1 : (e > 16 ? 16 : e);
    }

    template <class Syndrome, class Repack>
    int check_point(int it, Syndrome&& syndrome, Repack&& repack_into) {
        if (!((it % poll_every) == 0 || every_sweep)) {
            syndrome((int*)nullptr);
            return LDPC_OK;
        }
        const int slot = polls % POLL_RING;
        int* slot_dev = ring_dev + 4 * slot;
        LDPC_HIP_TRY(hipMemsetAsync(slot_dev, 0, 2 * sizeof(int), st));
        syndrome(slot_dev);
        LDPC_HIP_TRY(hipMemcpyAsync((void*)(ring_host + 4 * slot), slot_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        LDPC_HIP_TRY(hipEventRecord(ev[slot], st));
        pending.push_back({slot, it, sweeps, true});
        ++polls;
        // Read the OLDEST poll once a newer one is enqueued behind it (its event has long fired: a block of sweeps lies in
        // between); with a single-tile batch, or an unbounded run, there is nothing to overlap and the newest is read at once.
        // LONG sweeps (more than ~1.5 ms of streaming work: n = 64 800 x 512 tiles is 19 ms) also read the newest at once: the
        // host round trip is a percent of one sweep, and the repack decision then rests on the live counts of THIS check point
        // instead of those of a sweep ago -- while frames leave by the thousand per sweep (profiles/r05_config5_timeline.txt).
        const bool now = eager || cur_tiles < 2 || sweep_us(cur_tiles, bytes_per_frame) > 1500.0;
        while (!pending.empty() && (pending.size() >= 2 || now)) {
            const PendingPoll pp = pending.front();
            pending.erase(pending.begin());
            LDPC_HIP_TRY(hipEventSynchronize(ev[pp.slot]));
            const int lt = ring_host[4 * pp.slot], lf = ring_host[4 * pp.slot + 1];
            if (lt == 0) {  // every frame had left at that check point; what was enqueued since found no live tile
                all_left = true;
                sweeps = pp.sweeps;
                break;
            }
            if (repack.on && pp.tiling_current && pp.it > 0 && repack.wants(lt, lf) && it + 1 < cap) {
                cur_tiles = repack_into((lf + 63) / 64);
                ++repacks;
                for (PendingPoll& q : pending) q.tiling_current = false;
            }
        }
        return LDPC_OK;
    }

    // polls still in flight copy into the pinned ring; the next decode of the handle may run on another stream and reuse the slots:
    // let the last copy land first (everything of this decode is enqueued by now, the GPU is not waiting for the host)
    int finish() {
        if (!pending.empty()) LDPC_HIP_TRY(hipEventSynchronize(ev[pending.back().slot]));
        return LDPC_OK;
    }
};

}  // namespace ldpc

/*
 * ldpc_hip.h -- C ABI of libldpc_hip.so: MI355X (gfx950) belief-propagation LDPC decoding.
 *
 * This is the drop-in boundary for the BP hot path of thadikari/ldpc_decoders.  The upstream code is pure
 * Python on this path; its own FFI precedent is the ctypes binding of the ADMM projection
 * (src/parity_polytope/exact.py:12-21,49-53 -> extern "C" proj_vec/proj_csr, projection.cpp:252,266):
 * extern "C", caller-allocated buffers, plain pointers and sizes.  The entry points below follow that
 * pattern; each cites the upstream interface it replaces.  INTEGRATION.md shows the ctypes stub a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative LDPC_E_* code; ldpc_last_error() gives the text
 *     (thread-local).  Nothing throws across the boundary.
 *   - "dev" pointers are device (HBM) addresses on the handle's GPU; "host" pointers are ordinary memory.
 *   - frames are rows: priors / y / xhat are [B, n] row-major, exactly what numpy hands over.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Work is enqueued on it; calls may
 *     synchronise that stream internally (early-termination polling) but never the device.
 *   - handles are not thread-safe: one decoder per host thread / stream.
 */
#ifndef LDPC_HIP_H
#define LDPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ldpc_code_s* ldpc_code_t;
typedef struct ldpc_decoder_s* ldpc_decoder_t;

enum { LDPC_ALG_MSA = 0, LDPC_ALG_SPA = 1, LDPC_ALG_BEC = 2 };      /* decoder selector: src/utils.py:16, main.py:12 */
/* Corrected (normalised and / or offset) min-sum.  No upstream counterpart: it modifies the min-sum rule of src/bpa.py:86-102, which sends
 * on edge j of a check the sign s_j times m_j = min_{i != j} |v2c_i|.  The corrected decoder sends
 *     c2v_j = s_j * max( fl( fl(scale * m_j) - offset ), 0 )
 * in the decoder's arithmetic (fp64 or fp32; fp16 storage: in fp32, before the message is rounded to half), scale and offset rounded to
 * that type once on the host, two roundings (a multiply, then a subtraction: never a fused multiply-add).  A clamped message is +-0 and
 * contributes nothing.  Everything else of BPA.decode (src/bpa.py:17-63) is untouched.  scale = 1, offset = 0 (the state after create)
 * is bit-identical to LDPC_ALG_MSA.  Every dtype and backend, the same kernel shapes and layout plans as LDPC_ALG_MSA; accepted wherever
 * LDPC_ALG_MSA is, except LDPC_FLAG_PRIOR_GRID (LDPC_E_UNSUPPORTED on every backend: a scale takes values off the grid). */
enum { LDPC_ALG_NMSA = 3 };
/* Fixed-point min-sum: the decoder that is built in silicon -- q-bit channel values, q-bit saturating messages, a correction that stays on
 * the integer grid.  No upstream counterpart: it modifies src/bpa.py:86-102 the way LDPC_ALG_NMSA does.  Parameters (decoder state,
 * ldpc_decoder_set_fixed_point): bits q in 2..12 (default 6), frac_bits k in -8..8 (2), scale a multiple of 1/64 in (0, 1] (0.8125), offset
 * an integer >= 0 in levels (0).  V = 2^(q-1) - 1.
 *   1. Quantiser, the decoder's input stage:  level_v = clamp(rint(prior_v * 2^k), -V, +V), evaluated in the type the priors arrive in; the
 *      multiply is exact, rint rounds half to even, +-inf becomes +-V.  The caller's buffer is const and is not modified; NaN priors are
 *      outside the contract.  Everything below is in levels.
 *   2. Check rule: with s_j the sign of src/bpa.py:86-102 (sgn(0) = +1) and m_j = min(V, min_{i != j} |v2c_i|),
 *          c2v_j = s_j * max( floor(scale * m_j) - offset, 0 ).
 *      A check of degree 1 sends max(floor(scale * V) - offset, 0), not +inf.  scale * m is exact in fp32 (64 scale <= 64, m <= 2047).
 *   3. Everything else of BPA.decode (src/bpa.py:17-63) is unchanged: marginal = level + sum of c2v; v2c = marginal - c2v is stored
 *      unsaturated and saturates at the next check's input (hardware whose APP registers hold ceil(log2(V (1 + dv_max))) + 1 bits);
 *      syndrome exit, the iteration-0 check of y0 and marginal < 0 <=> bit 1 as upstream.  The soft output of ldpc_decode_soft is in levels.
 *   4. Exactness: every value is an integer of magnitude <= V (1 + dv_max) < 2^24, every c2v <= 2047 (exact in fp16).  LDPC_DTYPE_F64, _F32
 *      and _F16 decoders, streaming and LDS-resident backend, return identical decisions, iteration counts and (converted) soft outputs for
 *      the same priors, provided those are exactly representable in fp32 -- and equal an all-integer model of the rule.
 * Same kernel shapes and layout plans as LDPC_ALG_MSA; accepted wherever LDPC_ALG_MSA is, except LDPC_FLAG_PRIOR_GRID (LDPC_E_UNSUPPORTED: it
 * would add nothing). */
enum { LDPC_ALG_QMSA = 4 };
/* Layered (serial-C) corrected min-sum.  No upstream counterpart: BPA.decode (src/bpa.py:17-63) runs the flooding schedule -- every check
 * of a sweep sees the marginals the PREVIOUS sweep left.  Here the checks are processed in groups (layers), and every layer already sees
 * the marginals the layer before it left behind; a frame converges in roughly half the sweeps.  Per frame, in the decoder's arithmetic
 * T (fp64 or fp32):
 *   1. Layers.  layer_of_check[m] holds non-negative ints; two checks of one layer share no variable.  Default (greedy, on the host at
 *      create): for c = 0 .. m-1 in order, layer(c) is the smallest l >= 0 such that no check c' < c with layer(c') = l shares a variable
 *      with c.  Processing order: ascending (layer, check index); the checks of a layer are independent, so the result equals processing
 *      the checks one by one in that order.  ldpc_decoder_set_layers / _get_layers.
 *   2. Init.  marg_v = prior_v, every c2v = +0.  x_hat = y0 if given (the iteration-0 rule of src/bpa.py:20,29), else undefined until the
 *      first sweep.  Exits exactly as BPA.decode: before each sweep, stop if sweeps >= max_iter (max_iter <= 0: unbounded, capped at
 *      100000), or if H x_hat = 0 -- checked from sweep 1 on, at sweep 0 only when y0 is given.  iters = sweeps executed.
 *   3. One sweep.  For every check c in processing order, with its edges j = 0 .. dc-1 in H's row-major order:
 *          v_j   = marg[var_j] - c2v_j                              (one subtraction)
 *          s_j   = product of the signs of the other v_i, sgn(x) = -1 iff x < 0 (+-0 counts as +);  m_j = min_{i != j} |v_i|
 *          c2v_j = s_j * max( fl( fl(scale * m_j) - offset ), 0 )   (the rule of LDPC_ALG_NMSA: two roundings, never an FMA)
 *          marg[var_j] = v_j + c2v_j                                (one addition)
 *      After the last layer: x_hat_v = (marg_v < 0).
 *   4. Outputs.  A variable of degree 0 keeps marg = prior.  A frame that has left keeps its word and, with ldpc_decode_soft, the
 *      marginals of its last executed sweep (0 where it never swept).
 *   5. Correction.  scale and offset through ldpc_decoder_set_correction / _get_correction; after create (1, 0); ranges as LDPC_ALG_NMSA.
 *   6. Refusals.  LDPC_E_UNSUPPORTED: LDPC_BACKEND_FUSED, LDPC_DTYPE_F16, LDPC_FLAG_PRIOR_GRID, and a code with a check of degree < 2
 *      (its message is +inf: inf - inf at the second sweep).  LDPC_BACKEND_AUTO resolves to the streaming kernels;
 *      ldpc_decoder_kernel_name gives "", ldpc_decoder_fused_info reports 0 wavefronts.
 * Every value has one defined operation order: fp64 and fp32 results (decisions, iteration counts, soft outputs) are those of a
 * restatement in IEEE arithmetic, bit for bit, whatever the tiling, batch size, poll cadence or frame repacks.  Accepted by every entry
 * point that accepts LDPC_ALG_NMSA, with its shapes and flags. */
enum { LDPC_ALG_LMSA = 5 };
enum { LDPC_DTYPE_F32 = 0, LDPC_DTYPE_F64 = 1,                       /* message arithmetic                             */
       LDPC_DTYPE_F16 = 2 };  /* fp16 STORAGE of the check messages on the streaming kernels, fp32 arithmetic, fp32 priors / channel output:
                               * a throughput mode for codes whose state lives in HBM (the E-sized traffic halves); held to a
                               * stated tolerance, never the parity mode.  ldpc_decoder_create only. */
enum { LDPC_BACKEND_AUTO = 0, LDPC_BACKEND_STREAM = 1, LDPC_BACKEND_FUSED = 2 };
enum { LDPC_CH_BIAWGN = 0, LDPC_CH_BSC = 1, LDPC_CH_BEC = 2 };       /* channel selector: src/models.py:3               */
enum { LDPC_CH_RAW_OBSERVATION = 0x100 };  /* or-ed into LDPC_CH_BIAWGN for ldpc_channel: write y itself, not -2y/sigma^2 */
enum { LDPC_FLAG_NO_EARLY_EXIT = 1 };                                /* NOT reference behaviour: run exactly max_iter   */
/* Exact-in-fp32 min-sum (no upstream counterpart; the injection point is BPA.decode(y, priors), src/bpa.py:17): priors rounded to
 * multiples of 2^-k.  Min-sum only adds, subtracts and compares, so on such priors fp32 arithmetic reproduces the fp64 reference BIT FOR
 * BIT for as long as every prior and every check message stays below L = 2^(24-k) / (dv_max + 2), rounded down to a power of two (2^(21-k)
 * for variable degrees up to 6): then no partial sum, marginal or v2c of any sweep reaches 2^(24-k).  The LDS-resident fp32 kernels check
 * exactly that (priors once per frame, outgoing check magnitudes in every sweep) and count the frames
 * that do not (ldpc_decoder_grid_violations -- a run is exact iff the count is 0).  k = 0..23.
 *   ldpc_simulate / ldpc_decode: flags | LDPC_FLAG_PRIOR_GRID(k)   (simulate: quantises the generated priors AND arms the guard; decode: arms the guard;
 *                                both return LDPC_E_UNSUPPORTED for an fp32 / fp16 decoder that runs on the streaming kernels, which have no guard;
 *                                fp64 decoders need none: the flag is a no-op there)
 *   ldpc_channel:                channel | LDPC_CH_PRIOR_GRID(k)   (quantises the LLRs it writes; any dtype) */
#define LDPC_FLAG_PRIOR_GRID(k) ((((uint32_t)(k)) + 1u) << 8)
#define LDPC_FLAG_PRIOR_GRID_OF(flags) ((int)(((flags) >> 8) & 0x1fu) - 1) /* -1: off */
#define LDPC_CH_PRIOR_GRID(k) ((((int)(k)) + 1) << 12)
#define LDPC_CH_PRIOR_GRID_OF(channel) ((((channel) >> 12) & 0x1f) - 1)
enum { LDPC_E_ARG = -1, LDPC_E_HIP = -2, LDPC_E_GRAPH = -3, LDPC_E_UNSUPPORTED = -4, LDPC_E_NOMEM = -5 };

/* counters written by ldpc_count_errors / ldpc_simulate (int64 each) */
enum { LDPC_CNT_TOT = 0, LDPC_CNT_WEC = 1, LDPC_CNT_BEC = 2, LDPC_CNT_ITER_SUM = 3, LDPC_CNT_HIST0 = 4 };

const char* ldpc_last_error(void);
int ldpc_abi_version(void);
int ldpc_device_count(int* count);

/* Tanner graph from the row-major edge list of H: edge k = (edge_chk[k], edge_var[k]) sorted by check, then
 * variable -- the order of `xx, yy = np.where(parity_mtx)` in BPA.__init__ (src/bpa.py:9-15) and bec.SPA.__init__
 * (src/bec.py:77).  Host pointers; the graph is copied to `device` once (CSR + CSC index lists in HBM). */
int ldpc_code_create(int device, int32_t m, int32_t n, int64_t E, const int32_t* edge_chk, const int32_t* edge_var,
                     ldpc_code_t* out);
int ldpc_code_destroy(ldpc_code_t code);
int ldpc_code_info(ldpc_code_t code, int32_t* m, int32_t* n, int64_t* E, int32_t* max_dc, int32_t* max_dv);

/* Decoder = graph + algorithm + arithmetic + workspace.  Replaces the constructors bpa.SPA / bpa.MSA
 * (src/bpa.py:66-84) and bec.SPA / bec.MSA (src/bec.py:70-81,125). */
int ldpc_decoder_create(ldpc_code_t code, int alg, int dtype, int backend, ldpc_decoder_t* out);
int ldpc_decoder_destroy(ldpc_decoder_t dec);
/* backend actually used by the last decode (LDPC_BACKEND_*) and the number of sweeps the batch ran */
int ldpc_decoder_last_stats(ldpc_decoder_t dec, int* backend, int* sweeps);
/* streaming backend: how often the last decode gathered its live frames into dense tiles (per-frame early termination,
 * src/bpa.py:28-29: a frame that has left costs nothing; tiles of 64 frames are re-formed from the live ones) */
int ldpc_decoder_last_repacks(ldpc_decoder_t dec, int* repacks);
/* streaming backend: frames per pass through the kernels (sized once from the free HBM: the reference decodes one frame per call,
 * src/main.py:37-48, so any batch size is the build's own) and how often a failed workspace reservation made ldpc_decode halve it */
int ldpc_decoder_chunk_state(ldpc_decoder_t dec, int64_t* chunk_frames, int* retries);
/* exact-in-fp32 mode: frames in which a message left the range where fp32 sums of grid multiples are exact (a frame caught in a
 * trapping set: its min-sum messages grow geometrically; about 1 in 10^4 at 2 dB), since the last reset.  Such a frame is NOT counted
 * by ldpc_simulate, and ldpc_decode marks it with iters = -1 - sweeps; its global frame index (frame0 + position) is listed in
 * frames[0 .. min(count, cap, 4095)) so that the caller decodes it again in fp64 on the same priors (ldpc_decoders_amd/_device.py does).
 * Synchronises the device. */
int ldpc_decoder_grid_violations(ldpc_decoder_t dec, int64_t* count, int64_t* frames, int64_t cap, int reset);

/* The same redo list WITHOUT a host round trip (exact-in-fp32 Monte-Carlo rounds kept in flight, ldpc_decoders_amd/montecarlo.py): the
 * list as it lives in device memory -- list_dev[0] = frames set aside since the last reset, list_dev[1 .. cap] their global indices --
 * consumed on a stream by ldpc_channel_list (the priors of exactly those frames) -> ldpc_decode (fp64 decoder, `rows` frames: rows beyond
 * the list decode whatever the buffer holds and are not counted) -> ldpc_count_errors_list (counts the first min(list_dev[0], rows) rows,
 * each into the counter row of ITS round: counters_dev + ((frame - frame_base) / round_stride) * counter_stride, so that `nrounds` guarded
 * launches may share one redo pass and still keep one exact counter row per round; redone2_dev[0] += the rows counted, redone2_dev[1] += 1
 * if the list held more than `rows`: the caller must treat those rounds as failed) -> ldpc_decoder_grid_list_reset.  The guarded kernel
 * of the NEXT launch of the same decoder must be ordered behind the reset.  No upstream counterpart (see LDPC_FLAG_PRIOR_GRID). */
int ldpc_decoder_grid_list(ldpc_decoder_t dec, uint64_t** list_dev, int64_t* cap, void* stream);
int ldpc_decoder_grid_list_reset(ldpc_decoder_t dec, void* stream);
int ldpc_channel_list(int channel, int dtype, double param, int codeword, uint64_t seed, uint64_t stream_id, const uint64_t* list_dev,
                      int64_t rows, int32_t n, void* priors_dev, void* stream);
int ldpc_count_errors_list(const uint8_t* xhat_dev, int codeword, const int32_t* iters_dev, const uint64_t* list_dev, int64_t rows, int32_t n,
                           int32_t hist_bins, int64_t* counters_dev, int64_t counter_stride, uint64_t frame_base, uint64_t round_stride,
                           int64_t nrounds, int64_t* redone2_dev, void* stream);

/* Fused-backend plan of this decoder: out8 = {wavefronts per frame (0 = fused backend unavailable), conflict-free LDS gather cycles per sweep, extra bank-conflict
 * cycles with the trivial placement, extra cycles with the planned placement, resident waves per CU, LDS bytes per
 * frame, check rounds, variable rounds}. */
int ldpc_decoder_fused_info(ldpc_decoder_t dec, double* out8);

/* Host-only (no GPU needed): the LDS layout plan the fused backend would use for this (graph, algorithm, arithmetic) -- chosen
 * kernel shape, bank-conflict-minimising placement of checks / variables / edge positions (csrc/ldpc_layout.hpp) -- annealed with
 * `moves` moves (0: the default short run) and stored as <key>.plan in out_dir (NULL: not stored).  moves < 0: what decoder
 * construction does -- a stored plan is used if there is one (info4[0] is then negated), otherwise ONE process per node anneals the
 * default run (lock file next to the plan; the others wait for the file) and keeps it in out_dir / the per-user cache.  Decoders find such files in
 * $LDPC_FUSED_PLAN_DIR, in <package>/plans and in the per-user cache.  No upstream counterpart (the placement is a property of this
 * implementation; the graph arguments are those of ldpc_code_create, i.e. BPA.__init__'s edge lists, src/bpa.py:9-15).
 * info4 = {wavefronts per frame (0: no fused shape for this graph), conflict-free LDS gather cycles per sweep, extra bank-conflict
 * cycles of the trivial placement, extra cycles of the plan}. */
int ldpc_plan_layout(int32_t m, int32_t n, int64_t E, const int32_t* edge_chk, const int32_t* edge_var, int alg, int dtype,
                     int64_t moves, const char* out_dir, double* info4);

/* Name of the LDS-resident kernel this decoder launches (simulate != 0: the Monte-Carlo variant behind ldpc_simulate), exactly as
 * rocprofv3 prints it, e.g. "k_fused_bp<0, 6, 3, 5, 10, 2, true, 0, 3>" -- the key under which its committed PMC counters are filed
 * (profiles/roofline_counters.json).  Empty string: the decoder runs on the streaming kernels.  No upstream counterpart. */
int ldpc_decoder_kernel_name(ldpc_decoder_t dec, int simulate, char* buf, int64_t len);

/* Scale and offset of a corrected min-sum decoder (LDPC_ALG_NMSA, LDPC_ALG_LMSA).  No upstream counterpart: the rule they modify is src/bpa.py:86-102
 * (see LDPC_ALG_NMSA above).  0 < scale <= 1, offset >= 0, both finite; LDPC_E_ARG otherwise and for a decoder of another algorithm.
 * After ldpc_decoder_create: 1, 0.  Decoder state, read when a call is enqueued: a change takes effect from the next call. */
int ldpc_decoder_set_correction(ldpc_decoder_t dec, double scale, double offset);
/* The values in force (LDPC_E_ARG for a decoder of another algorithm).  No upstream counterpart (src/bpa.py:86-102 has neither). */
int ldpc_decoder_get_correction(ldpc_decoder_t dec, double* scale, double* offset);
/* Word length and correction of a fixed-point min-sum decoder (LDPC_ALG_QMSA, see there).  No upstream counterpart (src/bpa.py:86-102 has
 * none of them).  2 <= bits <= 12, -8 <= frac_bits <= 8, scale a multiple of 1/64 with 0 < scale <= 1, offset >= 0 in levels; LDPC_E_ARG
 * otherwise and for a decoder of another algorithm (ldpc_decoder_set_correction in turn refuses an LDPC_ALG_QMSA decoder).  After
 * ldpc_decoder_create: 6, 2, 0.8125, 0.  Decoder state, read when a call is enqueued: a change takes effect from the next call. */
int ldpc_decoder_set_fixed_point(ldpc_decoder_t dec, int bits, int frac_bits, double scale, int offset);
/* The values in force (LDPC_E_ARG for a decoder of another algorithm).  No upstream counterpart (src/bpa.py:86-102). */
int ldpc_decoder_get_fixed_point(ldpc_decoder_t dec, int* bits, int* frac_bits, double* scale, int* offset);
/* Layering of a layered min-sum decoder (LDPC_ALG_LMSA, see there; no upstream counterpart).  layer_of_check_host[m]: the layer of every
 * check; NULL restores the greedy layering of ldpc_decoder_create.  LDPC_E_ARG for a decoder of another algorithm, m != the code's number
 * of checks, a negative entry, or two checks of one layer that share a variable; a refused call leaves the previous layering in force
 * and the decoder usable.  Decoder state: in force from the next call.  The call waits for the whole device (hipDeviceSynchronize: a
 * decode of this decoder still in flight on any stream reads the old list), so it must not be made while a stream is being captured. */
int ldpc_decoder_set_layers(ldpc_decoder_t dec, const int32_t* layer_of_check_host, int32_t m);
/* The layering in force: *nlayers = number of distinct layers; layer_of_check_host_or_NULL[m], if given, receives the layer of every
 * check.  LDPC_E_ARG for a decoder of another algorithm.  No upstream counterpart. */
int ldpc_decoder_get_layers(ldpc_decoder_t dec, int32_t* nlayers, int32_t* layer_of_check_host_or_NULL);

/* Per-kernel timing for roofline reports: when enabled, decode calls bracket their dominant kernels with HIP events
 * recorded ON THE DECODE STREAM and accumulate elapsed milliseconds / launch counts per kernel class:
 * [0] streaming check pass, [1] streaming variable pass, [2] fused decode kernel, [3] a whole streaming decode, first to last
 * enqueued kernel (the two passes + tile load, syndrome, repack and unpack kernels: [3] - [0] - [1] is what the side kernels cost).
 * LDPC_ALG_LMSA: [0] the layer passes of a sweep (one launch per layer), [1] its decision pass, [3] the whole decode.
 * Enabling it makes every decode call end with a stream synchronise. */
int ldpc_decoder_profile(ldpc_decoder_t dec, int enable);
int ldpc_decoder_profile_read(ldpc_decoder_t dec, double* ms4, int64_t* launches4, int reset);

/* Batched BPA.decode(y, priors) (src/bpa.py:17-63) / bec.SPA.decode(y) (src/bec.py:83-122).
 *   priors_dev  [B,n] float or double per `dtype` (ignored for LDPC_ALG_BEC)
 *   y0_dev      [B,n] uint8 or NULL: hard received word checked at iteration 0 (src/bpa.py:20,29: BSC), or
 *               the received symbols {0,1,2} for LDPC_ALG_BEC (required)
 *   max_iter    sweep cap; <= 0 means "until every frame has left" as upstream (src/bpa.py:28), bounded at 100000
 *   xhat_dev    [B,n] uint8 out: decisions in {0,1} ({0,1,2} for BEC, 2 = still erased)
 *   iters_dev   [B]  int32 out: sweeps executed by each frame (0 = left at the iteration-0 check, x_hat = y0) */
int ldpc_decode(ldpc_decoder_t dec, const void* priors_dev, const uint8_t* y0_dev, int64_t B, int32_t max_iter,
                uint32_t flags, uint8_t* xhat_dev, int32_t* iters_dev, void* stream);
/* The same decode with PACKED decisions -- the information BPA.decode returns (src/bpa.py:62: n hard decisions) in n bits instead of n
 * bytes:
 *   xhat_bits_dev    [B, W] uint32, W = ceil(n / 32): bit (v & 31) of word (v >> 5) of row f = decision of variable v of frame f
 *                    (little-endian bit order: np.unpackbits(words.view(np.uint8), bitorder="little")[:, :n] gives the bytes of ldpc_decode);
 *                    padding bits of the last word are 0
 *   erased_bits_dev  [B, W] uint32: LDPC_ALG_BEC (required there): bit set = the symbol is still erased (x_hat = 2, src/bec.py:120), its
 *                    decision bit is then 0.  LLR decoders: may be NULL; written as all-zero when given.
 * The LLR decoders on the streaming kernels write the words straight from their decision bit planes (no [B,n] byte array exists). */
int ldpc_decode_bits(ldpc_decoder_t dec, const void* priors_dev, const uint8_t* y0_dev, int64_t B, int32_t max_iter, uint32_t flags,
                     uint32_t* xhat_bits_dev, uint32_t* erased_bits_dev, int32_t* iters_dev, void* stream);
/* Same (on whichever backend the decoder uses: streaming or fused), additionally returning the soft output:
 * marginals_dev [B,n] (`dtype`) = the marginal LLRs (prior + sum of check messages, src/bpa.py:35 -- a local of the
 * reference's loop, captured upstream only through its sum_cols hook) of each frame's LAST executed sweep (0 where a
 * frame never swept).  LLR decoders only; B <= 2^17. */
int ldpc_decode_soft(ldpc_decoder_t dec, const void* priors_dev, const uint8_t* y0_dev, int64_t B, int32_t max_iter,
                     uint32_t flags, uint8_t* xhat_dev, int32_t* iters_dev, void* marginals_dev, void* stream);
/* Same with host buffers (numpy ndpointer style, as exact.proj_csr); copies in, decodes, copies out, synchronises.  The decisions cross
 * PCIe PACKED (ldpc_decode_bits: n / 8 bytes per frame) and are expanded to bytes on the host. */
int ldpc_decode_host(ldpc_decoder_t dec, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags,
                     uint8_t* xhat, int32_t* iters);
/* Host buffers in, packed decisions out (layout of ldpc_decode_bits; erased_bits required for LDPC_ALG_BEC, optional otherwise). */
int ldpc_decode_host_bits(ldpc_decoder_t dec, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags,
                          uint32_t* xhat_bits, uint32_t* erased_bits, int32_t* iters);

/* Channel.send + LLR for frames [frame0, frame0+B) of the all-`codeword` word, Philox4x32-10 keyed by
 * (seed, stream_id, global frame index) -- biawgn.Channel.send/LLR.decode (src/biawgn.py:13-28),
 * bsc (src/bsc.py:11-25), bec.Channel.send (src/bec.py:11-18).  priors_dev [B,n] (`dtype`; NULL for BEC),
 * y_dev [B,n] uint8 (BSC: received bits, BEC: symbols; may be NULL for BI-AWGN).  priors_dev may be NULL for the BSC.
 * LDPC_CH_BIAWGN | LDPC_CH_RAW_OBSERVATION writes the received values y into priors_dev instead of their LLRs. */
int ldpc_channel(int channel, int dtype, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0,
                 int64_t B, int32_t n, void* priors_dev, uint8_t* y_dev, void* stream);

/* The same for a RANDOM codeword per frame -- `--codeword -1`, src/main.py:38: x = code.cb[np.random.choice(K)] -- frame f sends
 * word floor(w * K / 2^32) of codebook_dev ([K,n] uint8, Code.cb of src/codes.py:11-14, K <= 2^31), w = first Philox word of block
 * 0xFFFFFFFE of the frame; sent_dev [B,n] uint8 receives the word each frame sent (for ldpc_count_errors_words). */
int ldpc_channel_words(int channel, int dtype, double param, const uint8_t* codebook_dev, int64_t K, uint64_t seed, uint64_t stream_id,
                       uint64_t frame0, int64_t B, int32_t n, void* priors_dev, uint8_t* y_dev, uint8_t* sent_dev, void* stream);

/* Monte-Carlo counters of main.test (src/main.py:41-45), ACCUMULATED into counters_dev (int64[4 + hist_bins]):
 * tot += B, wec += #frames with errors, bec += bit errors, iter_sum += sum(iters), hist[min(iters, bins-1)] += 1.
 * `sent_dev` is the transmitted word [n] or NULL for the all-`codeword` word; iters_dev may be NULL. */
int ldpc_count_errors(const uint8_t* xhat_dev, const uint8_t* sent_dev, int codeword, const int32_t* iters_dev, int64_t B,
                      int32_t n, int32_t hist_bins, int64_t* counters_dev, void* stream);

/* The same counters from PACKED decisions (ldpc_decode_bits): errors of a frame = popcount((xhat_bits ^ sent) | erased) over its n bits.
 * sent_bits_dev [W] = the transmitted word, packed, or NULL for the all-`codeword` word; erased_bits_dev may be NULL (LLR decoders). */
int ldpc_count_errors_bits(const uint32_t* xhat_bits_dev, const uint32_t* erased_bits_dev, const uint32_t* sent_bits_dev, int codeword,
                           const int32_t* iters_dev, int64_t B, int32_t n, int32_t hist_bins, int64_t* counters_dev, void* stream);

/* The same against one sent word PER FRAME: sent_dev [B,n] (ldpc_channel_words). */
int ldpc_count_errors_words(const uint8_t* xhat_dev, const uint8_t* sent_dev, const int32_t* iters_dev, int64_t B, int32_t n,
                            int32_t hist_bins, int64_t* counters_dev, void* stream);

/* ---- Systematic GF(2) encoder: a random codeword per frame for ANY code ----------------------------------------
 * `--codeword -1` (src/main.py:38: x = code.cb[np.random.choice(K)]) upstream needs the code book, i.e. a toy code.  The encoder
 * takes the systematic form of H computed on the host (ldpc_decoders_amd/encoder.py: GF(2) elimination, pivot = first row with a 1,
 * columns left to right): par_pos [r] = the r = rank pivot columns, info_pos [k] = the other k = n - r columns, P_bits_host [k, r]
 * bytes in {0,1} (row-major) with  c[par_pos] = u . P mod 2,  c[info_pos] = u.  Host pointers; P is kept on `device` as bits in
 * the fragment order of the i8 matrix cores. */
typedef struct ldpc_encoder_s* ldpc_encoder_t;
int ldpc_encoder_create(int device, int32_t n, int32_t k, int32_t r, const int32_t* info_pos, const int32_t* par_pos, const uint8_t* P_bits_host,
                        ldpc_encoder_t* out);
int ldpc_encoder_destroy(ldpc_encoder_t enc);
/* Read-only: the launch shape the handle settled on, so that a test can assert which kernels it reaches.  out[0] = nt, the 32-column
 * tiles per wave (1, 2, 4 or 8: the instantiation of the GEMM kernel); out[1] = column groups of nt tiles (the grid's y); out[2] =
 * k-groups of 128 information bits, ceil(k / 128); out[3] = 8192-bit chunks of the information-bit kernel, ceil(out[2] / 64). */
int ldpc_encoder_info(ldpc_encoder_t enc, int32_t out[4]);
/* Codewords of B given information words: info_dev [B, k] uint8 in {0,1} -> sent_dev [B, n] uint8 (the layout ldpc_count_errors_words
 * reads).  u . P runs on v_mfma_i32_32x32x32_i8 (int32 accumulation, & 1): exact.  Uses a workspace of the handle (one call at a time). */
int ldpc_encode(ldpc_encoder_t enc, const uint8_t* info_dev, int64_t B, uint8_t* sent_dev, void* stream);
/* The same for RANDOM information words: frame f of [frame0, frame0+B) draws its k bits from Philox4x32-10 keyed by (seed, stream_id,
 * global frame index) like every other draw, blocks 0x80000000 + j: bit t of word w of block j is information bit 128 j + 32 w + t
 * (disjoint from the noise blocks 0 .. n/4 and 0xFFFFFFFE / 0xFFFFFFFF).  A frame's word does not depend on the batching. */
int ldpc_encode_random(ldpc_encoder_t enc, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, uint8_t* sent_dev, void* stream);
/* Channel.send + LLR of ldpc_channel for a GIVEN word per frame, sent_dev [B, n] uint8: the noise is that of ldpc_channel for the same
 * (seed, stream_id, frame), draw for draw -- with an all-zero sent_dev the outputs equal ldpc_channel(codeword = 0)'s.  Plain
 * LDPC_CH_* ids only (no raw-observation or prior-grid flags); priors_dev / y_dev as ldpc_channel. */
int ldpc_channel_sent(int channel, int dtype, double param, const uint8_t* sent_dev, uint64_t seed, uint64_t stream_id, uint64_t frame0,
                      int64_t B, int32_t n, void* priors_dev, uint8_t* y_dev, void* stream);

/* ---- Punctured and shortened transmission (csrc/ldpc_ratematch.hip; no upstream counterpart) -------------------
 * A transmission pattern is one byte per variable of the mother code, kind_dev [n] uint8:
 *   0  sent
 *   1  punctured: a codeword bit that is not transmitted; the decoder starts it from a prior of 0
 *   2  shortened: a filler bit known to be 0 and not transmitted; the decoder starts it from the prior +short_llr
 * (a byte above 2 is not a kind; both entry points read it as shortened).
 * No decoder changes: the pattern lives in what the channel writes and in what the tally counts.  The channel parameter keeps its
 * meaning PER TRANSMITTED SYMBOL (sigma^2 = 10^(-snr/10), src/biawgn.py:10); no rate correction is applied.
 *
 * ldpc_channel_pattern: LDPC_CH_BIAWGN and LDPC_CH_BSC, dtype fp32 / fp64, frames [frame0, frame0 + B); one thread = 4 consecutive
 * variables = one Philox block, as ldpc_channel.  sent_dev [B, n] uint8 is the word of every frame, or NULL for the all-`codeword` word.
 *   kind 0   the outputs of ldpc_channel_sent (sent_dev NULL: of ldpc_channel(codeword)) for the same (seed, stream_id, global frame,
 *            variable), draw for draw and bit for bit: the Philox block and word of a variable are those of its index in the mother
 *            code, so a pattern moves the noise of no other bit
 *   kind 1   prior +0.0; y = 0 on the BSC
 *   kind 2   prior +short_llr (positive = bit 0, as -2y/sigma^2); y = 0
 * short_llr must be finite and > 0; 32.0 wherever the package exposes it (a power of two: exact on every prior grid and under the
 * fixed-point quantisers; below |v| ~ 38.2, from where the verbatim fp64 sum-product's tanh is exactly 1.0).  priors_dev / y_dev as
 * ldpc_channel_sent.  kind_dev is read as dwords, and the outputs written as float4 / double2, when n % 4 == 0 and every buffer lies on
 * its natural boundary; as bytes and scalars otherwise.  LDPC_E_ARG, each with a sentence that names this entry point: sent_dev NULL with
 * codeword == 1 and any shortened variable (that word is no codeword of the shortened code; to find out, EVERY call with sent_dev NULL and
 * codeword == 1 copies kind_dev to the host and waits for `stream` -- a caller that knows its pattern passes words of ones in sent_dev
 * and keeps the stream asynchronous, as _device.PatternHandle does), LDPC_CH_BEC, LDPC_CH_RAW_OBSERVATION, LDPC_CH_PRIOR_GRID, a short_llr out of range. */
int ldpc_channel_pattern(int channel, int dtype, double param, const uint8_t* sent_dev, int codeword, const uint8_t* kind_dev, double short_llr,
                         uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t n, void* priors_dev, uint8_t* y_dev, void* stream);
/* The counters of ldpc_count_errors, ACCUMULATED into counters_dev, with a frame's errors taken over the variables of kind < 2: a
 * punctured bit is a codeword bit and is counted, a shortened bit is known and is not.  sent_dev [B, n] (one word PER FRAME, as
 * ldpc_count_errors_words) or NULL for the all-`codeword` word; iters_dev may be NULL.  One wave per frame, as ldpc_count_errors. */
int ldpc_count_errors_pattern(const uint8_t* xhat_dev, const uint8_t* sent_dev, int codeword, const uint8_t* kind_dev, const int32_t* iters_dev,
                              int64_t B, int32_t n, int32_t hist_bins, int64_t* counters_dev, void* stream);

/* ---- Incremental-redundancy HARQ (csrc/ldpc_harq.hip; no upstream counterpart) ---------------------------------
 * The retransmission loop around a rate-matched code: per-frame soft buffers that survive between decodes, a retransmission for the
 * frames whose decode failed, noise for the later copies of a bit that is independent of the first, a tally that knows when a frame
 * leaves.  The schedule is made on the host (ratematch.Harq): the circular buffer is the kind-0 variables of a transmission pattern in
 * ascending index (kind 1: never in the buffer; kind 2: shortened, as above), transmission t sends E_t buffer positions from its start
 * k_t, wrapping; E_t beyond the buffer length repeats.  Per transmission the device gets two bytes per variable, cnt_dev [n] (copies of
 * the variable in this transmission; 0 outside the buffer) and first_dev [n] (copies in all earlier transmissions = the ordinal of this
 * transmission's first copy); over a whole schedule a variable has at most 255 copies.  No decoder changes.
 *
 * ldpc_harq_transmit: LDPC_CH_BIAWGN and LDPC_CH_BSC, dtype fp32 / fp64; one thread = 4 consecutive variables of one output row.
 * Output row i (0 <= i < B_out) of soft_new_dev [B_out, n] is
 *     row src_dev[i] of soft_old_dev [old_rows, n]   (src_dev NULL: row i; soft_old_dev NULL: the first transmission, which starts from
 *                                                      +0.0 for a buffer variable, +0.0 for kind 1 and +short_llr for kind 2)
 *   + the LLR of every copy of this transmission, added in ascending ordinal r = first .. first + cnt - 1, one addition each in dtype
 * for the frame  frame0 + orig_dev[i]  (orig_dev NULL: i) whose sent word is row orig_dev[i] of sent_dev [sent_rows, n] (NULL: the
 * all-`codeword` word).  Copy ordinal r of variable v draws word v % 4 of Philox block v / 4 of the stream word stream_id + (r << 16),
 * through the Box-Muller pairing and the -(2/sigma^2) y form (BSC: the threshold and +-llr) of ldpc_channel_pattern: r = 0 is that
 * entry point's draw bit for bit, every later copy is independent of it and still a function of (seed, stream_id, global frame) alone.
 * A block none of whose four variables has a copy at ordinal r draws nothing for r.  A kind-2 value never changes.  The two buffers
 * ping-pong (soft_old_dev == soft_new_dev is refused): the gather of the frames that go on rides inside the transmission.  A row whose
 * src / orig entry lies outside [0, old_rows) / [0, sent_rows) is left unwritten.  The dword / float4 / double2 path under the alignment
 * rule of ldpc_channel_pattern.  LDPC_E_ARG, each with a sentence that names this entry point: what ldpc_channel_pattern refuses
 * (LDPC_CH_BEC, LDPC_CH_RAW_OBSERVATION, LDPC_CH_PRIOR_GRID, a short_llr out of range, the all-one word with a shortened variable --
 * with the same read-back of kind_dev), and stream_id >= 65536 (the ordinal lives in bits 16 and up of the stream word). */
int ldpc_harq_transmit(int channel, int dtype, double param, const uint8_t* sent_dev, int64_t sent_rows, int codeword, const uint8_t* kind_dev,
                       const uint8_t* cnt_dev, const uint8_t* first_dev, double short_llr, uint64_t seed, uint64_t stream_id, uint64_t frame0,
                       const int64_t* src_dev, const int64_t* orig_dev, const void* soft_old_dev, int64_t old_rows, int64_t B_out, int32_t n,
                       void* soft_new_dev, void* stream);
/* fail_dev [B] uint8: 1 where xhat_dev [B, n] (bytes, bit 0 counts) leaves some check of the code unsatisfied -- the acknowledgement rule
 * of a system without a CRC.  One wave per frame; lanes stride over the checks of the code handle's device edge list. */
int ldpc_harq_syndrome(ldpc_code_t code, const uint8_t* xhat_dev, int64_t B, uint8_t* fail_dev, void* stream);
/* The tally of transmission t of T (1 <= T <= 16), ACCUMULATED into counters_dev [4 + hist_bins + T + 2].  Every row is one decode attempt:
 * its iters enter ITER_SUM and the histogram, and tx_bits (E_t) enters sym.  A row LEAVES when fail_dev[i] == 0 or t == T - 1: it adds 1 to
 * TOT, err > 0 to WEC and err to BEC, err taken over kind < 2 against row orig_dev[i] of sent_dev [sent_rows, n] (orig_dev NULL: row i;
 * sent_dev NULL: the all-`codeword` word).  Behind the histogram: ack[t] (rows leaving with fail == 0 at transmission t; T words),
 * undetected (fail == 0 and err > 0), sym.  iters_dev may be NULL.  One wave per row, as ldpc_count_errors_pattern. */
int ldpc_harq_tally(const uint8_t* xhat_dev, const uint8_t* sent_dev, int64_t sent_rows, int codeword, const uint8_t* kind_dev, const int32_t* iters_dev,
                    const uint8_t* fail_dev, const int64_t* orig_dev, int64_t B, int32_t n, int32_t hist_bins, int32_t t, int32_t T, int64_t tx_bits,
                    int64_t* counters_dev, void* stream);

/* ---- Maximum-likelihood decoding of the short codes by codebook search -----------------------------------------
 * Replaces biawgn.ML (src/biawgn.py:66-78), bsc.ML (src/bsc.py:63-75) and bec.ML (src/bec.py:21-36).  `codebook` is
 * Code.cb (src/codes.py:11-14): [K, n] bytes in {0,1}, host pointer, K <= 2^20 words of n <= 64 bits. */
typedef struct ldpc_ml_s* ldpc_ml_t;
int ldpc_ml_create(int device, const uint8_t* codebook, int64_t K, int32_t n, ldpc_ml_t* out);
int ldpc_ml_destroy(ldpc_ml_t ml);
/* ML.decode for B frames.  y_dev: [B,n] observations -- double or float per `dtype` for LDPC_CH_BIAWGN, uint8 symbols
 * ({0,1}, 2 = erased) for LDPC_CH_BSC / LDPC_CH_BEC.  coef2 (host) holds the constants the upstream constructor
 * computes: {2*noise_var, unused} for BI-AWGN, {log p, log(1-p)} for BSC / BEC.  The log-likelihood of every
 * codeword is evaluated in fp64 in the upstream operation order (including numpy's summation order), so its maximum
 * (best_dev, [B] double) and the set of maximisers (ties_dev [B] = how many; tie_mask_dev [B, ceil(K/32)] uint32,
 * bit k of word k/32 = codeword k attains the maximum) are bit-identical to upstream's.  The pick among the
 * maximisers (math_utils.arg_max_rand, src/math_utils.py:72-74) is maximiser number floor(pick[f] * ties / 2^32) in
 * codebook order, the first one if pick_dev is NULL; index_dev [B] int32 and xhat_dev [B,n] uint8 receive it.  Every
 * output pointer may be NULL. */
int ldpc_ml_decode(ldpc_ml_t ml, int channel, int dtype, const double* coef2, const void* y_dev, int64_t B,
                   const uint32_t* pick_dev, int32_t* index_dev, int32_t* ties_dev, uint32_t* tie_mask_dev, double* best_dev,
                   uint8_t* xhat_dev, void* stream);
/* Channel.send + ML.decode + the counters of main.test for frames [frame0, frame0+B) of the all-`codeword` word; same
 * Philox keying as ldpc_channel, the tie-break word is block 0xFFFFFFFF of the frame.  Accumulates tot/wec/bec. */
int ldpc_ml_simulate(ldpc_ml_t ml, int channel, int dtype, double param, int codeword, uint64_t seed, uint64_t stream_id,
                     uint64_t frame0, int64_t B, int64_t* counters_dev, void* stream);

/* ---- Maximum-likelihood decoding over the BEC for EVERY code: GF(2) elimination ---------------------------------
 * Replaces bec.ML (src/bec.py:21-36: the maximum of the likelihood over the code book, math_utils.arg_max_rand at
 * src/math_utils.py:72-74 picking uniformly among the maximisers) for codes without a code book.  Over the BEC every codeword that
 * agrees with the unerased symbols has the same likelihood, so the maximisers are the solutions of  H_E x_E = H_Ebar y_Ebar  over GF(2):
 *   1. peel: the erasure decoder (LDPC_ALG_BEC, max_iter <= 0) to its stopping-set exit; the bits it leaves erased are the residual
 *      set R (the largest stopping set inside the erasure pattern);
 *   2. the system on the columns R, ascending, with the rows (checks) that touch R, right-hand side = XOR of each row's known bits,
 *      brought to reduced row echelon form (columns in ascending order; pivot = the first unused row, in H's row order, with a 1);
 *   3. free column number t (the non-pivot columns of R, ascending) takes bit t of Philox4x32-10 keyed by (seed, stream_id, global
 *      frame index), block 0xC0000000 + j: bit t of word w of block j is free bit 128 j + 32 w + t (disjoint from the noise blocks
 *      0 .. n/4, the information bits 0x80000000 + j, 0xFFFFFFFE and 0xFFFFFFFF); the pivot columns follow.  The pick is uniform over
 *      the solution set and depends only on the global frame index;
 *   4. nullity [B] int32: d = |R| - rank (the solution set has 2^d words; 0 for a frame peeling finished), -1 if the system is
 *      inconsistent (only possible when the sent word is no codeword; the decisions are then those of the same rule on the
 *      consistent part and are no codeword).  Under nullity -1 the word still returns every unerased symbol unchanged (the peeled ones
 *      too); on R it holds the free bits and the pivot values of step 3, the rows left without a pivot being ignored.
 * The system of a frame lives in the LDS of one CU: create fails with LDPC_E_ARG unless the worst case (every bit erased) fits 160 KiB,
 * i.e.  4 * (3 W + 3 S + S * 64 ceil(m / 64)) <= 163840  with W = ceil(n / 32), S = ceil((n + 1) / 32)  (about m * n <= 1 310 720 bits),
 * and m <= 4096.  Handles are not thread-safe (one workspace). */
typedef struct ldpc_bec_ml_s* ldpc_bec_ml_t;
int ldpc_bec_ml_create(ldpc_code_t code, ldpc_bec_ml_t* out);
int ldpc_bec_ml_destroy(ldpc_bec_ml_t h);
/* Steps 2-4 on already peeled frames: bits_dev / erased_bits_dev [B, W] in the layout ldpc_decode_bits writes (LDPC_ALG_BEC, max_iter
 * <= 0); out_bits_dev [B, W] (may equal bits_dev) receives the resolved words, nullity_dev [B] the nullities.  Frames [frame0, frame0+B). */
int ldpc_bec_ml_solve(ldpc_bec_ml_t h, const uint32_t* bits_dev, const uint32_t* erased_bits_dev, int64_t B, uint64_t seed, uint64_t stream_id,
                      uint64_t frame0, uint32_t* out_bits_dev, int32_t* nullity_dev, void* stream);
/* ML.decode (src/bec.py:21-36) for B frames of symbols y_dev [B, n] uint8 in {0, 1, 2 = erased}: peel + solve; xhat_dev [B, n] uint8
 * in {0, 1}, nullity_dev [B] int32. */
int ldpc_bec_ml_decode(ldpc_bec_ml_t h, const uint8_t* y_dev, int64_t B, uint64_t seed, uint64_t stream_id, uint64_t frame0, uint8_t* xhat_dev,
                       int32_t* nullity_dev, void* stream);
/* Channel.send (src/bec.py:11-18, ldpc_channel's draws) + ML.decode + the counters of main.test (src/main.py:41-45) for frames
 * [frame0, frame0+B) of the all-`codeword` word: accumulates tot / wec / bec into counters_dev (int64[4]); ITER_SUM stays 0, as for
 * ldpc_ml_simulate.  codeword 0 or 1; 1 is refused (LDPC_E_ARG) when a check has odd degree (the all-ones word is then no codeword). */
int ldpc_bec_ml_simulate(ldpc_bec_ml_t h, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                         int64_t* counters_dev, void* stream);

/* ---- Ordered-statistics post-processing (BP+OSD) of the LLR decoders -------------------------------------------
 * No upstream counterpart: it adds to BPA.decode (src/bpa.py:17-63), which returns a word that is no codeword when the sweeps run out.
 * OSD re-decodes exactly those frames from BP's soft output.  Per frame, deterministic (no random draws), for post[n] (the LLRs that
 * order the bits) and prior[n] (the channel LLRs that score candidates), both of one type T in {float, double}; order in {0, 1};
 * depth >= 0:
 *   1. Pass-through.  h_v = (post_v < 0).  If H h = 0 the frame is not touched: the word is h, pick = -1, cost = -1.0.
 *   2. Order.  rho_v = |post_v| rounded to fp32 (nearest-even; NaN -> 0; magnitudes below 2^-126 are outside the contract).  The key of
 *      variable v is (uint64(bits(rho_v)) << 32) | v; the keys are unique, the ascending sort is a total order: pi(p) = the variable at
 *      sorted position p, least reliable first, ties broken by the variable index.
 *   3. Eliminate.  H with its columns in the order pi is brought to reduced row echelon form over GF(2), columns left to right; the
 *      pivot of a column is any unused row with a 1 there (the reduced form does not depend on that choice).  The positions with a
 *      pivot number rank(H); the others, f_0 < f_1 < ..., are free.
 *   4. Candidates.  Candidate 0 takes the free positions from h and each pivot position from its row (the XOR of the row's free bits):
 *      the unique codeword that agrees with h on the most reliable information set.  order == 1: candidate t, 1 <= t <= min(depth, number
 *      of free positions), is the same with free position f_(t-1) flipped.
 *   5. Score and pick.  g_v = (prior_v < 0), w_v = (double)|prior_v| (NaN -> 0).  cost(x) = the fp64 sum, from +0.0, over p = 0 .. n-1 in
 *      that order, of w_pi(p) wherever x_pi(p) != g_pi(p) (plain adds).  The smallest cost wins, on equal cost the smallest t.  Outputs:
 *      the word, pick = t, cost.
 * One wave per failed frame, the frame's whole system in the LDS of one CU: create fails with LDPC_E_ARG unless
 *   4 * osd_lds_words(m, n) <= 163840  and  m <= 4096,   osd_lds_words = 2 NP + S * RP + 4 n + 5 S,
 * NP = the power of two >= n (the sort keys, 64 bits each), S = ceil(n / 32), RP = 64 ceil(m / 64) (the matrix, S words per row), 4 n for
 * pi, its inverse, the pivot row of every position and the list of free positions, 5 S for the bit masks in position order.  Handles are
 * not thread-safe (one workspace). */
typedef struct ldpc_osd_s* ldpc_osd_t;
int ldpc_osd_create(ldpc_code_t code, ldpc_osd_t* out);
int ldpc_osd_destroy(ldpc_osd_t h);
/* Steps 1-5 for B frames.  dtype: LDPC_DTYPE_F32 / _F64 = the type of post_dev and prior_dev [B, n]; out_bits_dev [B, W] uint32 in the
 * layout of ldpc_decode_bits; pick_dev [B] int32; cost_dev [B] double or NULL.  order outside {0, 1} or depth < 0: LDPC_E_ARG. */
int ldpc_osd_solve(ldpc_osd_t h, int dtype, const void* post_dev, const void* prior_dev, int64_t B, int32_t order, int64_t depth,
                   uint32_t* out_bits_dev, int32_t* pick_dev, double* cost_dev, void* stream);
/* BPA.decode (src/bpa.py:17-63) by `dec`, then OSD of the frames it left without a codeword: ldpc_decode_soft in chunks of <= 2^17 frames
 * (post = the marginals of the last sweep; a frame that left at the iteration-0 check of y0 never swept: post = its priors), solve,
 * unpack.  `dec` is any fp32 or fp64 LDPC_ALG_MSA / SPA / NMSA / QMSA / LMSA decoder of the same code (an fp16 or LDPC_ALG_BEC decoder:
 * LDPC_E_UNSUPPORTED; a decoder of another code: LDPC_E_ARG); priors_dev / y0_dev / max_iter / flags as ldpc_decode.  xhat_dev [B, n] uint8,
 * iters_dev [B] = BP's sweeps, pick_dev [B]. */
int ldpc_osd_decode(ldpc_osd_t h, ldpc_decoder_t dec, const void* priors_dev, const uint8_t* y0_dev, int64_t B, int32_t max_iter,
                    uint32_t flags, int32_t order, int64_t depth, uint8_t* xhat_dev, int32_t* iters_dev, int32_t* pick_dev, void* stream);
/* ldpc_channel + ldpc_osd_decode + ldpc_count_errors_bits for frames [frame0, frame0+B) of the all-`codeword` word -- the body of
 * `while wec < min_wec` (src/main.py:37-45) as ldpc_simulate is.  ITER_SUM and the histogram come from BP's iteration counts.  LDPC_CH_BIAWGN
 * and LDPC_CH_BSC; codeword 0 or 1; 1 is refused (LDPC_E_ARG) when a check has odd degree, as in ldpc_bec_ml_simulate. */
int ldpc_osd_simulate(ldpc_osd_t h, ldpc_decoder_t dec, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id,
                      uint64_t frame0, int64_t B, int32_t max_iter, uint32_t flags, int32_t order, int64_t depth, int32_t hist_bins,
                      int64_t* counters_dev, void* stream);

/* ---- Hard-decision decoding: bit-sliced Gallager-B (GALB) ------------------------------------------------------
 * No upstream counterpart: every decoder of the reference works on soft values (src/bpa.py) or on erasures (src/bec.py).  Gallager's
 * algorithm A / B passes ONE BIT per edge.  Per frame, for the received word y in {0,1}^n, d_v the degree of variable v and the
 * threshold parameter t (0 <= t <= 255, ldpc_hard_set_threshold), the flip threshold of a variable of degree d is
 *     b_d = floor((d - 1) / 2) + 1      for t = 0   (the majority of the d - 1 extrinsic messages; Gallager A for d = 3),
 *     b_d = min(t, max(d - 1, 1))       for t >= 1  (any t >= dv_max - 1 is Gallager A).
 *   1. Iteration 0.  If H y = 0 the frame leaves with x = y, iters = 0.  Otherwise v2c_(v->c) = y_v on every edge.
 *   2. Sweep l = 1, 2, ...
 *        check:     c2v_(c->v) = XOR over v' in N(c) \ {v} of v2c_(v'->c)   ( = P_c ^ v2c_(v->c), P_c the parity of all messages into c)
 *        variable:  delta_j = c2v_j ^ y_v on each of the d edges, T = sum of delta_j;
 *                   decision  x_v = y_v ^ [2 T > d + 1]          (majority of the d + 1 votes, the received bit wins a tie)
 *                   message   v2c_j = y_v ^ [T - delta_j >= b_d]
 *                   a variable of degree 0 keeps x_v = y_v
 *        exit:      if H x = 0 the frame leaves with x and iters = l; after sweep max_iter every remaining frame leaves with the x of
 *                   that sweep and iters = max_iter.
 *   3. LDPC_FLAG_NO_EARLY_EXIT: exactly max_iter sweeps for every frame (the iteration-0 exit is off too), iters = max_iter.
 *   4. Refusals.  max_iter <= 0: LDPC_E_ARG (a hard-decision decoder may oscillate for ever and has no "nothing changed" exit).
 *      t outside 0..255: LDPC_E_ARG.  A code with a variable of degree above 63: LDPC_E_UNSUPPORTED (ldpc_hard_create).
 *      LDPC_BACKEND_FUSED on a code whose slab does not fit the LDS (below): LDPC_E_UNSUPPORTED (ldpc_hard_create).
 * Everything is an integer: decisions and iteration counts are one function of (H, y, t, max_iter, flags), the same on both backends, for
 * any batch size and any position of a frame in its batch.
 * Backends.  A message is one bit; a machine word holds it for 32 frames (a slab), bit f = frame f of the slab.
 *   LDPC_BACKEND_STREAM  any code: the planes live in HBM in supertiles of 64 slabs (2048 frames, one wave lane per slab), v2c lines in
 *                        variable-major order; a load / transposition kernel, one check + syndrome pass and one variable pass per sweep,
 *                        exit bookkeeping per supertile (a supertile without a live frame is skipped), an unload kernel.
 *   LDPC_BACKEND_FUSED   one workgroup owns one slab for all its sweeps: y, the decisions, v2c and the check parities live in the LDS,
 *                        HBM sees the received word in and the decisions out, once.  LDS-fit rule:
 *                            hard_lds_bytes = 4 * (2 n + E + m + 4) <= 163840
 *                        (n words of y, n of x, E of v2c, m of parities, 4 of slab state).  Slabs are handed out by an atomic dispenser.
 *   LDPC_BACKEND_AUTO    the LDS kernel where the rule holds, the streaming kernels otherwise.
 * Handles are not thread-safe (one workspace). */
typedef struct ldpc_hard_s* ldpc_hard_t;
int ldpc_hard_create(ldpc_code_t code, int backend, ldpc_hard_t* out);
int ldpc_hard_destroy(ldpc_hard_t h);
/* The threshold parameter t of the rule above; after ldpc_hard_create: 0.  Handle state, read when a call is enqueued. */
int ldpc_hard_set_threshold(ldpc_hard_t h, int t);
int ldpc_hard_get_threshold(ldpc_hard_t h, int* t);
/* Steps 1-3 for B frames.  y_dev [B, n] uint8 in {0, 1} (only bit 0 of a byte is read); xhat_dev [B, n] uint8 or NULL; xhat_bits_dev
 * [B, W] uint32 in the layout of ldpc_decode_bits or NULL (at least one of the two); iters_dev [B] int32.  May synchronise `stream`. */
int ldpc_hard_decode(ldpc_hard_t h, const uint8_t* y_dev, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat_dev,
                     uint32_t* xhat_bits_dev, int32_t* iters_dev, void* stream);
/* ldpc_channel + ldpc_hard_decode + ldpc_count_errors_bits for frames [frame0, frame0+B) of the all-`codeword` word -- the body of
 * `while wec < min_wec` (src/main.py:37-45) as ldpc_osd_simulate is.  LDPC_CH_BSC (the received bits) and LDPC_CH_BIAWGN (the word sliced
 * at prior < 0); codeword 0 or 1; 1 is refused (LDPC_E_ARG) when a check has odd degree.  The received bytes cross HBM once. */
int ldpc_hard_simulate(ldpc_hard_t h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                       int32_t max_iter, uint32_t flags, int32_t hist_bins, int64_t* counters_dev, void* stream);
/* kernels of the last decode / simulate: LDPC_BACKEND_STREAM or LDPC_BACKEND_FUSED (before the first call: what AUTO resolved to) */
int ldpc_hard_last_backend(ldpc_hard_t h, int* backend);
/* out4 = {LDS bytes per slab (the rule's left side, also when it does not fit), frames per slab, slabs per CU as launched (0: the LDS
 * kernel is not available for this code), workgroups of the LDS kernel's grid} */
int ldpc_hard_info(ldpc_hard_t h, double* out4);

/* ---- Layered fixed-point min-sum, LDS-resident (LQMSA) -----------------------------------------------------------
 * No upstream counterpart: LDPC_ALG_QMSA's integer rule on LDPC_ALG_LMSA's schedule, the whole frame resident in the LDS as integers
 * (int16 marginals, int8 check messages).  Everything after the quantiser is an integer.
 *   Parameters (handle state, ldpc_lqmsa_set_fixed_point; after create 6, 2, 0.8125, 0): bits q in 2..8, V = 2^(q-1) - 1 <= 127;
 *      frac_bits k in -8..8; scale a multiple of 1/64 with 0 < scale <= 1, scale64 = 64 scale; offset an integer >= 0 in levels.
 *      Layers (ldpc_lqmsa_set_layers): validity rule, greedy default and processing order -- ascending (layer, check index) -- are
 *      exactly those of LDPC_ALG_LMSA.
 *   1. Quantiser.  level_v = clamp(rint(prior_v * 2^k), -V, V) in the type the priors arrive in (fp32 or fp64): LDPC_ALG_QMSA's
 *      quantiser, the same levels (+-inf -> +-V, -0 -> 0); what it leaves undefined (NaN) is undefined here.
 *   2. Init and exits.  marg = level, every c2v = 0, x_hat = y0 if given.  Exits as BPA.decode (src/bpa.py:17-63): before each sweep,
 *      stop at max_iter (<= 0: unbounded, capped at 100000), or when H x_hat = 0 -- checked from sweep 1 on, at sweep 0 only when y0 is
 *      given.  LDPC_FLAG_NO_EARLY_EXIT runs exactly max_iter sweeps.  iters = sweeps executed.
 *   3. One sweep.  For every check in processing order, with its edges j in H's row-major order:
 *          v_j   = marg[var_j] - c2v_j
 *          a_j   = min(|v_j|, V);   neg_j = (v_j < 0)
 *          m_j   = min over i != j of a_i;   s_j = XOR over i != j of neg_i
 *          c2v_j = (s_j ? -1 : +1) * max( ((scale64 * m_j) >> 6) - offset, 0 )
 *          marg[var_j] = v_j + c2v_j                    (v_j itself is NOT clipped)
 *      After the last layer x_hat = (marg < 0).  Invariant: marg_v = level_v + sum of c2v, so |marg| <= V (1 + dv) and int16 holds it
 *      for every dv <= 255.  A variable of degree 0 keeps its level.
 *   4. Outputs.  xhat as bytes and / or packed words (layout of ldpc_decode_bits), iters, optionally soft: int16 [B, n], the marginals
 *      in levels of each frame's last executed sweep, 0 where it never swept.
 *   5. Refusals.  ldpc_lqmsa_create, LDPC_E_UNSUPPORTED: a check of degree < 2 (as LDPC_ALG_LMSA), a variable of degree above 255, a
 *      code whose frame does not fit the LDS rule below (use LDPC_ALG_LMSA for it).  ldpc_lqmsa_set_fixed_point, LDPC_E_ARG: a
 *      parameter out of range or a scale off the 1/64 grid.  ldpc_lqmsa_set_layers, LDPC_E_ARG: a bad layering; the previous one stays
 *      in force, as with ldpc_decoder_set_layers.
 * Determinism: decisions, iteration counts and soft outputs are one function of (H, layers, parameters, priors, y0, max_iter, flags): the
 * same for any batch size, any position of a frame in its batch and any number of waves per frame.
 * Kernel.  One workgroup of W waves (W in {1, 2, 4, 8}) owns one frame for all its sweeps, lane = check, a barrier per layer; frames are
 * handed out by an atomic dispenser.  HBM sees the priors in and the word, iters and the optional soft output out, once.  LDS rule:
 *     lqmsa_lds_bytes(m, n, E, dc_max) = 8 ceil(2 n / 8) + m * row(dc_max) + 16 <= 163840,   row(d) = 8 for d <= 8, else 4 ceil(d / 4)
 * (n int16 marginals, one row of int8 messages per check, 16 bytes of frame state; E does not enter), and n <= 65536 (16-bit index
 * tables; implied by the rule for every code without 2^14 variables of degree 0).  With F = floor(163840 / bytes) frames in a CU's LDS, W is the
 * smallest of 1, 2, 4, 8 that gives the CU the most waves, min(F, 32 / W) * W: 1 from F = 32 on, 2 from 16, 4 from 8, 8 below; the environment variable LDPC_LQMSA_NW (1, 2, 4, 8; read at create) overrides it.
 * Handles are not thread-safe (one workspace). */
typedef struct ldpc_lqmsa_s* ldpc_lqmsa_t;
int ldpc_lqmsa_create(ldpc_code_t code, ldpc_lqmsa_t* out);
int ldpc_lqmsa_destroy(ldpc_lqmsa_t h);
/* Word length and correction; ranges above.  Handle state, read when a call is enqueued. */
int ldpc_lqmsa_set_fixed_point(ldpc_lqmsa_t h, int bits, int frac_bits, double scale, int offset);
int ldpc_lqmsa_get_fixed_point(ldpc_lqmsa_t h, int* bits, int* frac_bits, double* scale, int* offset);
/* The layering, with the semantics of ldpc_decoder_set_layers / _get_layers: layer_of_check_host[m], NULL restores the greedy layering; a
 * refused call leaves the previous layering in force and the handle usable; the call waits for the whole device. */
int ldpc_lqmsa_set_layers(ldpc_lqmsa_t h, const int32_t* layer_of_check_host, int32_t m);
int ldpc_lqmsa_get_layers(ldpc_lqmsa_t h, int32_t* nlayers, int32_t* layer_of_check_host_or_NULL);
/* Steps 1-4 for B frames.  priors_dev [B, n] float or double per `dtype` (LDPC_DTYPE_F32 / _F64); y0_dev [B, n] uint8 or NULL; xhat_dev
 * [B, n] uint8 or NULL; xhat_bits_dev [B, W] uint32 or NULL (at least one of the two); iters_dev [B] int32; soft_dev [B, n] int16 or NULL. */
int ldpc_lqmsa_decode(ldpc_lqmsa_t h, int dtype, const void* priors_dev, const uint8_t* y0_dev, int64_t B, int32_t max_iter, uint32_t flags,
                      uint8_t* xhat_dev, uint32_t* xhat_bits_dev, int32_t* iters_dev, int16_t* soft_dev, void* stream);
/* ldpc_channel (fp32 priors) + ldpc_lqmsa_decode + ldpc_count_errors_bits for frames [frame0, frame0+B) of the all-`codeword` word, with
 * the call shape and counters of ldpc_hard_simulate.  LDPC_CH_BIAWGN and LDPC_CH_BSC (the received word takes the iteration-0 check);
 * codeword 0 or 1; 1 is refused (LDPC_E_ARG) when a check has odd degree. */
int ldpc_lqmsa_simulate(ldpc_lqmsa_t h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                        int32_t max_iter, uint32_t flags, int32_t hist_bins, int64_t* counters_dev, void* stream);
/* out4 = {LDS bytes per frame, waves per frame, frames per CU as launched, workgroups of the kernel's grid} */
int ldpc_lqmsa_info(ldpc_lqmsa_t h, double* out4);

/* ---- Quasi-cyclic codes: shift-addressed layered fixed-point min-sum (QCMSA) ---------------------------------------
 * No upstream counterpart.  H is an mb x nb array of Z x Z blocks, each zero or a cyclically shifted identity: block (i, j) with shift
 * s, 0 <= s < Z, has its ones at (i Z + r, j Z + (r + s) mod Z), r = 0 .. Z - 1.  ldpc_qc_create finds the shifts from the code's own
 * edge list for the lifting size Z it is given (no new file format; Z = 1 takes any code and makes every check a layer).
 *   Contract.  The outputs are those of the LQMSA statement above (its steps 1-4: quantiser, init and exits, one sweep, outputs) on the
 *      expanded H with every block row one layer:  layer[c] = position of block row c / Z in the processing order (ldpc_qc_set_order;
 *      after create the natural order 0 .. mb - 1).  A block row's checks touch disjoint variables, and every value is an integer, so
 *      the result depends neither on the order of a check's edges nor on the order of the checks within a layer: ldpc_lqmsa_decode
 *      with that layering returns the same bytes, words, iteration counts and soft outputs.
 *   Parameters (ldpc_qc_set_fixed_point): ranges and defaults of ldpc_lqmsa_set_fixed_point (after create 6, 2, 0.8125, 0).
 *   Refusals.  ldpc_qc_create, LDPC_E_ARG: Z < 1, or Z does not divide m and n.  LDPC_E_UNSUPPORTED: a block that is neither zero nor one
 *      shifted identity (the message names the block; use ldpc_lqmsa_create for such a code); a block row of degree < 2; a variable of
 *      degree above 255; a frame that does not fit the LDS rule below.  ldpc_qc_set_order, LDPC_E_ARG: anything but a permutation of
 *      0 .. mb - 1; the previous order stays in force and the handle usable.
 * Determinism: as LQMSA -- one function of (H, Z, order, parameters, priors, y0, max_iter, flags), the same for any batch size, any
 * position of a frame in its batch and any number of waves per frame.
 * Kernel.  One workgroup of W waves (W in {1, 2, 4, 8}) owns one frame for all its sweeps; lane L of pass k of block row i owns check
 * i Z + 64 k + L and reaches variable j Z + (r + s) mod Z from its row r and two wave-uniform scalars: no index table; the block row's
 * degree is wave-uniform and selects a body unrolled at compile time (degrees 2..8; a loop above).  A barrier per block row; frames
 * from an atomic dispenser.  LDS rule: LQMSA's layout and bound with dc_max = the largest block-row degree,
 *     lqmsa_lds_bytes(m, n, E, dc_max) = 8 ceil(2 n / 8) + m * row(dc_max) + 16 <= 163840.
 * With F = floor(163840 / bytes), W is LQMSA's rule for F capped at the smallest of 1, 2, 4, 8 that is >= ceil(Z / 64) (a block row has
 * ceil(Z / 64) wave passes); the environment variable LDPC_QC_NW (1, 2, 4, 8; read at create) overrides it.
 * Several frames per wave.  With Z < 64 one frame leaves part of the wave dark.  For Z <= 32 (a block row is one pass) a second kernel
 * puts P frames, 2 <= P <= floor(64 / Z), into one workgroup of one wave: lane L serves frame slot L / Z with row L mod Z, lanes >= P Z
 * idle, slot g keeps its own frame image (the layout above) at byte g * stride of the LDS,
 *     stride(bytes, Z) = the smallest multiple of 16 that is >= bytes and congruent to 16 ceil(2 Z / 16) modulo 128
 * (slots that share a 32-lane group then read one block column on disjoint LDS banks).  The slots are independent: own frame index, own
 * sweep count, the syndrome is the wave's ballot under the slot's lane mask, and a slot whose frame has left (syndrome zero, cap, or the
 * received word at sweep 0) writes its outputs and draws the next frame at once while the others keep sweeping.  The outputs are those of
 * the contract above for every P.  The rule, pick(Z, bytes): 1 for Z > 32, else min(floor(64 / Z), floor(163840 / stride)), at least
 * 1; at P >= 2 the grid holds min(floor(163840 / (P stride)), 32) workgroups per CU and LDPC_QC_NW has no part.  Z = 33 .. 63 and the
 * tail pass of Z > 64 still leave lanes dark.  After create P = 1: ldpc_qcpack_set opts in.  The environment variable LDPC_QC_PACK_GRID
 * (read at create) caps the grid of the second kernel; with 1 the frames are handed out in index order (tests).
 * Handles are not thread-safe (one workspace). */
typedef struct ldpc_qc_s* ldpc_qc_t;
int ldpc_qc_create(ldpc_code_t code, int32_t Z, ldpc_qc_t* out);
int ldpc_qc_destroy(ldpc_qc_t h);
/* Word length and correction; ranges of ldpc_lqmsa_set_fixed_point.  Handle state, read when a call is enqueued. */
int ldpc_qc_set_fixed_point(ldpc_qc_t h, int bits, int frac_bits, double scale, int offset);
int ldpc_qc_get_fixed_point(ldpc_qc_t h, int* bits, int* frac_bits, double* scale, int* offset);
/* The detected base: mb, nb, Z and, unless NULL, shifts_host[mb * nb] row-major, -1 for a zero block. */
int ldpc_qc_get_base(ldpc_qc_t h, int32_t* mb, int32_t* nb, int32_t* Z, int32_t* shifts_host_or_NULL);
/* The processing order of the block rows: order_host[mb], a permutation of 0 .. mb - 1 (block row processed at each position); NULL
 * restores the natural order.  The call waits for the whole device. */
int ldpc_qc_set_order(ldpc_qc_t h, const int32_t* order_host_or_NULL, int32_t mb);
int ldpc_qc_get_order(ldpc_qc_t h, int32_t* mb, int32_t* order_host_or_NULL);
/* Argument lists and semantics of ldpc_lqmsa_decode / ldpc_lqmsa_simulate / ldpc_lqmsa_info. */
int ldpc_qc_decode(ldpc_qc_t h, int dtype, const void* priors_dev, const uint8_t* y0_dev, int64_t B, int32_t max_iter, uint32_t flags,
                   uint8_t* xhat_dev, uint32_t* xhat_bits_dev, int32_t* iters_dev, int16_t* soft_dev, void* stream);
int ldpc_qc_simulate(ldpc_qc_t h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                     int32_t max_iter, uint32_t flags, int32_t hist_bins, int64_t* counters_dev, void* stream);
int ldpc_qc_info(ldpc_qc_t h, double* out4);
/* Frames per wave of ldpc_qc_decode / ldpc_qc_simulate on this handle.  0: the rule's pick; 1: one frame per workgroup (the state after
 * create); P >= 2: LDPC_E_ARG (the message names Z and the bytes, the previous value stays) unless P Z <= 64 and P stride <= 163840.
 * With P >= 2 ldpc_qc_info reports {bytes per frame, 1, P * workgroups per CU, workgroups}. */
int ldpc_qcpack_set(ldpc_qc_t h, int32_t frames_per_wave);
int ldpc_qcpack_get(ldpc_qc_t h, int32_t* frames_per_wave, int32_t* rule_pick);

/* ---- Streaming layered fixed-point min-sum (SLQMSA): the LQMSA contract for codes beyond the LDS -------------------
 * No upstream counterpart.
 *   Contract.  Steps 1-4 of the LQMSA statement above (ldpc_lqmsa_*), word for word: the quantiser; the init and the exits (y0 and the
 *      iteration-0 check, max_iter <= 0, LDPC_FLAG_NO_EARLY_EXIT); the sweep rule with scale64, the offset and the clip at V; the outputs
 *      (bytes and / or packed words, iters, the optional int16 soft output of each frame's last executed sweep, 0 where it never swept).
 *      Parameters, their ranges and defaults are those of ldpc_lqmsa_set_fixed_point; layers those of LDPC_ALG_LMSA (validity rule, greedy
 *      default, processing order), with the refusal semantics of ldpc_lqmsa_set_layers.  On a code both take, ldpc_lqmsa_decode at the
 *      same layering returns the same bytes, words, iteration counts and soft outputs.
 *   Refusals.  ldpc_slq_create, LDPC_E_UNSUPPORTED: a check of degree < 2; a variable of degree above 255 (int16 marginals hold
 *      V (1 + dv)).  Nothing else: no size rule, any check degree, n may exceed 65536 (32-bit indices).
 * Determinism: as LQMSA -- one function of (H, layers, parameters, priors, y0, max_iter, flags), the same for any batch size, position of
 * a frame in its batch, chunking of the batch, poll cadence and frame repack.
 * Kernels.  The state lives in HBM in tiles of 64 frames, lane = frame: int16 marginals [tile][n][64], int8 check messages [tile][E][64],
 * decision bit planes and live words as the floating-point streaming decoders keep them.  One launch per layer (a wave takes a tile and
 * a run of the layer's checks) and a decision pass per sweep: 6 E + 2 n bytes per frame-sweep.  Frames leave one by one (syndrome before
 * every sweep); when the batch has thinned out the live frames are gathered into dense tiles (never with a soft output), under the
 * policy of the floating-point streaming decoders: LDPC_STREAM_REPACK=0 turns it off, LDPC_STREAM_REPACK_FILL sets the fill below which
 * it fires; both are read at every decode.  A batch is decoded in chunks of whole tiles such that a chunk's state and a repack target of
 * the same size stay within 24 GiB (LDPC_SLQ_WORKSPACE_MB, read at every decode, sets another bound; at least one tile per chunk).
 * Handles are not thread-safe (one workspace). */
typedef struct ldpc_slq_s* ldpc_slq_t;
int ldpc_slq_create(ldpc_code_t code, ldpc_slq_t* out);
int ldpc_slq_destroy(ldpc_slq_t h);
/* Ranges, defaults and semantics of ldpc_lqmsa_set_fixed_point / _get_fixed_point / _set_layers / _get_layers. */
int ldpc_slq_set_fixed_point(ldpc_slq_t h, int bits, int frac_bits, double scale, int offset);
int ldpc_slq_get_fixed_point(ldpc_slq_t h, int* bits, int* frac_bits, double* scale, int* offset);
int ldpc_slq_set_layers(ldpc_slq_t h, const int32_t* layer_of_check_host, int32_t m);
int ldpc_slq_get_layers(ldpc_slq_t h, int32_t* nlayers, int32_t* layer_of_check_host_or_NULL);
/* Argument lists and semantics of ldpc_lqmsa_decode / ldpc_lqmsa_simulate.  The calls poll the device while they enqueue and may
 * synchronise `stream`.  ldpc_slq_simulate stages the fp32 priors of a chunk of frames ([chunk, n], 8 n bytes per frame written and
 * read once, against 6 E + 2 n per sweep; there is no in-kernel noise on this path). */
int ldpc_slq_decode(ldpc_slq_t h, int dtype, const void* priors_dev, const uint8_t* y0_dev, int64_t B, int32_t max_iter, uint32_t flags,
                    uint8_t* xhat_dev, uint32_t* xhat_bits_dev, int32_t* iters_dev, int16_t* soft_dev, void* stream);
int ldpc_slq_simulate(ldpc_slq_t h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                      int32_t max_iter, uint32_t flags, int32_t hist_bins, int64_t* counters_dev, void* stream);
/* out4 = {bytes of integer state per frame (2 n + E), tiles per chunk under the workspace bound, layers, launches per sweep (layers + 1)} */
int ldpc_slq_info(ldpc_slq_t h, double* out4);
/* Per-kernel timing, the slots LDPC_ALG_LMSA has in ldpc_decoder_profile: HIP events on the decode stream, accumulated as milliseconds /
 * launch counts in ms3 / launches3 (either may be NULL): [0] the layer passes of a sweep, [1] its decision pass, [2] a whole decode.
 * enable 1 / 0 switches it (a decode then ends with a stream synchronise), a negative value leaves it; reset != 0 clears the sums. */
int ldpc_slq_profile(ldpc_slq_t h, int enable, double* ms3, int64_t* launches3, int reset);
/* out3 = {sweeps enqueued by the last decode (the largest over its chunks), frame repacks, chunks} */
int ldpc_slq_last_stats(ldpc_slq_t h, int32_t* out3);

/* ---- ADMM LP decoding ------------------------------------------------------------------------------------------
 * Replaces admm.ADMM (src/admm.py:9-77) together with its native projection (src/parity_polytope/projection.cpp:30-275, bound
 * upstream through ctypes in exact.py:12-53).  Check degrees up to 16. */
typedef struct ldpc_admm_s* ldpc_admm_t;
int ldpc_admm_create(ldpc_code_t code, ldpc_admm_t* out);
int ldpc_admm_destroy(ldpc_admm_t admm);
/* ADMM_Base.decode(y, gamma) for B frames (src/admm.py:42-69).  gamma_dev [B,n] double: the LLR vectors the channel wrappers
 * hand over (src/biawgn.py:28, src/bsc.py:25, src/bec.py:38-45).  mu, eps, max_iter: the constructor's kwargs (max_iter <= 0 =
 * no cap upstream; bounded at 100000 here).  x_dev [B,n] double out: x_hat as it stands at return, BEFORE
 * math_utils.pseudo_to_cw (src/math_utils.py:28-34); iters_dev [B] int32: iter_count at return (the bin upstream's histogram
 * increments, src/admm.py:49); converged_dev [B] uint8 or NULL: 1 where the stopping test fired.  fp64 throughout, in the
 * upstream operation order: results are bit-identical to upstream's for the same gamma. */
int ldpc_admm_decode(ldpc_admm_t admm, const double* gamma_dev, int64_t B, double mu, double eps, int32_t max_iter, double* x_dev,
                     int32_t* iters_dev, uint8_t* converged_dev, void* stream);

/* how often the last ldpc_admm_decode gathered its live frames into dense tiles (frames leave one by one, src/admm.py:65-66) */
int ldpc_admm_last_repacks(ldpc_admm_t admm, int* repacks);
/* which kernels the last ldpc_admm_decode ran on: 0 = the streaming kernels (state in HBM, any code), 1 = the LDS-resident kernel (one
 * workgroup per frame, z / lambda / x in the LDS of the CU: codes whose checks all have six edges and whose frame fits 160 KB).
 * Same arithmetic either way: estimates and iteration counts are bit-identical.  LDPC_ADMM_BACKEND=stream forces 0. */
int ldpc_admm_last_backend(ldpc_admm_t admm, int* backend);

/* Profiling aid: coalesced 4-byte-per-lane device copy of a known size, used to calibrate the profiler's HBM byte
 * counters for the access width of the streaming kernels. */
int ldpc_debug_copy4(const void* src_dev, void* dst_dev, int64_t nbytes, void* stream);

/* One pass of the whole hot path for frames [frame0, frame0+B): channel -> LLR -> decode -> count, everything on
 * the device; counters accumulate as in ldpc_count_errors.  This is the body of `while wec < min_wec`
 * (src/main.py:37-45) for B frames at once. */
int ldpc_simulate(ldpc_decoder_t dec, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id,
                  uint64_t frame0, int64_t B, int32_t max_iter, uint32_t flags, int32_t hist_bins, int64_t* counters_dev,
                  void* stream);

/* `rounds` passes of ldpc_simulate in ONE call: round r decodes frames frame0 + r * round_stride + [0, B) (round_stride >= B: the
 * distance between the rounds of one rank when a round of the whole job is sharded over ranks; = B on a single GPU) and accumulates into
 * its own counter row counters_dev + r * (4 + hist_bins).  Each row is exactly what ldpc_simulate would have produced for that round --
 * the caller applies the stopping rule of `while wec < min_wec` (src/main.py:37) to the rows in order, so the counters stay a function
 * of the round size, not of how many rounds travelled together.  The LDS-resident erasure decoder runs all rounds as ONE launch (its
 * frame positions are refilled across round boundaries, no drain between rounds); every other decoder is called round by round. */
int ldpc_simulate_rounds(ldpc_decoder_t dec, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0,
                         int64_t B, int32_t rounds, uint64_t round_stride, int32_t max_iter, uint32_t flags, int32_t hist_bins,
                         int64_t* counters_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_H */

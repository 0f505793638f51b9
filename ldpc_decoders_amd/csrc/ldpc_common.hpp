// Shared declarations of the gfx950 LDPC belief-propagation library (libldpc_hip.so).
//
// Data model:
//   * H is flattened once into a row-major edge list (edge k = (chk[k], var[k]), the order of
//     np.where(H) used by the reference, src/bpa.py:12) + CSR row pointers + CSC lists, resident in HBM.
//   * Frames are processed in TILES of 64: one wavefront lane <-> one frame, so every H index is
//     wave-uniform (scalar loads) and every message access is one contiguous 64-element line.
//   * Streaming backend: per tile, check -> variable messages c2v[tile][edge][64] and marginals marg[tile][n][64] live in HBM;
//     the check pass forms v2c = marg - c2v_old on the fly, the variable pass rebuilds the marginals (ldpc_stream.hip).
//     That state is a TileSet; a Decoder holds two (a frame repack gathers the live frames from one into the other) beside
//     the few tables both share.  A decode call's arguments travel in a DecodeCall, never in the Decoder.
//   * Fused backend (regular codes whose state fits the LDS): one wavefront owns one frame for all
//     iterations; messages never leave the CU.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ldpc_hip.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace ldpc {

enum Alg : int {
    ALG_MSA = 0, ALG_SPA = 1, ALG_BEC = 2,
    ALG_NMSA = 3,  // normalised / offset min-sum (ldpc_cn.hpp cn_msa<.., MSA_CORRECTED>)
    ALG_QMSA = 4,  // fixed-point min-sum: q-bit saturating messages on the integer grid (ldpc_cn.hpp cn_msa<.., MSA_FIXED>, quantise_prior)
    ALG_LMSA = 5   // layered (serial-C) corrected min-sum on the streaming kernels (ldpc_stream.hip k_layer; the rule is ALG_NMSA's)
};
// THE table of the algorithms, indexed by Alg: what the entry points, the dispatchers and the messages need to know about one.  A new variant
// is one row here (plus its rule in ldpc_cn.hpp and its row in the Python registry, models.py).
struct AlgRow {
    const char* name;   // ABI name, as messages spell it
    const char* words;  // the algorithm in words, as messages spell it
    bool llr;           // decodes LLR priors (false: the erasure decoder, which decodes received symbols)
    int family;         // whose variable pass, register tuning and table words it shares (alg_family)
    bool corrected;     // carries Decoder::corr_scale / corr_offset (ldpc_decoder_set_correction)
    bool fixed_point;   // carries Decoder::fx_* (ldpc_decoder_set_fixed_point)
    bool layered;       // carries a layering (ldpc_decoder_set_layers); streaming kernels in fp32 / fp64 only
    bool lds;           // LDS-resident shapes exist (fused backend, ldpc_plan_layout)
    bool f16;           // fp16 storage of the streaming messages exists
    const char* no_grid;  // why LDPC_FLAG_PRIOR_GRID is refused in any arithmetic on every backend; null: it is not
};
constexpr int ALG_COUNT = 6;
constexpr AlgRow kAlgs[ALG_COUNT] = {
    {"LDPC_ALG_MSA", "min-sum", true, ALG_MSA, false, false, false, true, true, nullptr},
    {"LDPC_ALG_SPA", "sum-product", true, ALG_SPA, false, false, false, true, true, nullptr},
    {"LDPC_ALG_BEC", "erasure decoder", false, ALG_BEC, false, false, false, true, false, nullptr},
    {"LDPC_ALG_NMSA", "corrected min-sum", true, ALG_MSA, true, false, false, true, true,
     "has no exact-in-fp32 mode (a scale takes values off the grid)"},
    {"LDPC_ALG_QMSA", "fixed-point min-sum", true, ALG_MSA, false, true, false, true, true,
     "quantises its priors itself (ldpc_decoder_set_fixed_point)"},
    {"LDPC_ALG_LMSA", "layered min-sum", true, ALG_LMSA, true, false, true, false, false,
     "has no exact-in-fp32 mode (a scale takes values off the grid)"},
};
constexpr bool alg_known(int alg) { return alg >= 0 && alg < ALG_COUNT; }
constexpr const AlgRow& alg_row(int alg) { return kAlgs[alg]; }
// min-sum family: everything that is keyed on "the rule is compare / negate only" (register tuning, sign-bit shortcuts, table words) treats
// the corrected rule as min-sum
constexpr int alg_family(int alg) { return kAlgs[alg].family; }
constexpr bool alg_is_minsum(int alg) { return alg_family(alg) == ALG_MSA; }
// ABI names of the rows that have `flag` set, for messages: "LDPC_ALG_NMSA, LDPC_ALG_LMSA"
inline std::string alg_names(bool AlgRow::*flag, const char* sep = ", ") {
    std::string out;
    for (const AlgRow& r : kAlgs)
        if (r.*flag) out += (out.empty() ? "" : sep) + std::string(r.name);
    return out;
}
enum DType : int { DT_F32 = 0, DT_F64 = 1, DT_F16 = 2 };  // DT_F16: fp16 STORAGE of the streaming messages, fp32 arithmetic and priors
enum Backend : int { BK_AUTO = 0, BK_STREAM = 1, BK_FUSED = 2 };
enum Channel : int { CH_BIAWGN = 0, CH_BSC = 1, CH_BEC = 2 };
constexpr int CH_RAW_OBSERVATION = 0x100;  // or-ed into the channel id: BI-AWGN writes y itself instead of the LLR -2y/sigma^2

constexpr int TILE = 64;  // frames per tile == wavefront width on gfx950

// error codes returned over the C ABI come from include/ldpc_hip.h (LDPC_E_*); 0 == success
constexpr int LDPC_OK = 0;

void set_error(const char* fmt, ...);
const char* last_error();

#define LDPC_HIP_TRY(expr)                                                                          \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            ::ldpc::set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return LDPC_E_HIP;                                                              \
        }                                                                                           \
    } while (0)

#define LDPC_TRY(expr)            \
    do {                          \
        int _rc = (expr);         \
        if (_rc != 0) return _rc; \
    } while (0)

// Tanner graph resident on one device.
struct Code {
    int device = 0;
    int32_t m = 0, n = 0;
    int64_t E = 0;
    int32_t max_dc = 0, min_dc = 0, max_dv = 0, min_dv = 0;
    bool odd_check = false;  // some check has odd degree (has_odd_check, ldpc_sim.hpp)
    // device arrays
    int32_t* d_row_ptr = nullptr;   // [m+1]
    int32_t* d_edge_var = nullptr;  // [E]  variable of edge k (row-major edge order)
    int32_t* d_edge_chk = nullptr;  // [E]
    int32_t* d_col_ptr = nullptr;   // [n+1]
    int32_t* d_col_edge = nullptr;  // [E]  edges of variable v in ascending edge order
    // host mirrors
    std::vector<int32_t> row_ptr, edge_var, edge_chk, col_ptr, col_edge;
};

// host part of ldpc_code_create: validates the edge list and fills the host mirrors (no device call)
int code_build_host(int32_t m, int32_t n, int64_t E, const int32_t* chk, const int32_t* var, Code* c);

// Growable device buffer owned by a decoder (workspace is kept between calls).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int reserve(size_t need);
    void release();
};

struct FusedPlan;  // ldpc_fused.hip

// Arguments of ONE decode call (ldpc_api.hip builds one per chunk of frames): nothing of a call is kept in the Decoder.
struct DecodeCall {
    const void* priors = nullptr;  // [B, n] LLRs in the decoder's precision (LLR decoders)
    const uint8_t* y0 = nullptr;   // [B, n] received symbols (erasure decoder; optional first syndrome check of the LLR decoders)
    int64_t B = 0;
    int32_t max_iter = 0;
    uint32_t flags = 0;
    uint8_t* xhat = nullptr;   // decisions as bytes [B, n] ...
    uint32_t* bits = nullptr;  // ... or, if set, as packed words [B, ceil(n/32)] straight from the planes (streaming LLR decoders only)
    int32_t* iters = nullptr;
    void* soft = nullptr;  // [B, n] marginals of the last sweep (ldpc_decode_soft)
    hipStream_t stream = nullptr;
    hipEvent_t done_event = nullptr;  // LDS-resident backend: recorded right behind the decode kernel (low-latency host path)
};

// One state set of the streaming decoders: what exists once per set and moves together in a frame repack.
struct TileSet {
    DevBuf edge;    // one line per edge: check -> variable messages (fp32 / fp64), variable -> check messages (fp16 storage, erasure)
    DevBuf node;    // one line per node: marginals per variable (LLR decoders; fp16 storage: only with a soft output), summaries per check (erasure)
    DevBuf prior;   // one line per variable
    DevBuf planes;  // decision (erasure: value + erased) bit planes per variable
    DevBuf live;    // live-frame words per tile
    DevBuf fmap;    // frame index of (tile, lane) once repacked
};

enum BufKind : int {
    BUF_STATE = 0,    // streaming state, sized by the chunk of frames: given back by the chunk-halving retry, counted as re-usable
    BUF_SHARED = 1,   // small tables that live as long as the decoder
    BUF_STAGING = 2,  // staging of the *_host and simulate entry points
};

struct Decoder {
    Code* code = nullptr;
    int alg = ALG_MSA, dtype = DT_F32, backend = BK_AUTO;
    double corr_scale = 1.0, corr_offset = 0.0;  // ALG_NMSA, ALG_LMSA: c2v = sign * max(scale * min - offset, 0) (ldpc_decoder_set_correction); read at every launch
    // ALG_QMSA (ldpc_decoder_set_fixed_point; read at every launch): priors -> clamp(rint(prior * 2^fx_frac), -V, V), V = 2^(fx_bits - 1) - 1;
    // c2v = sign * max(floor(fx_scale * min(m, V)) - fx_offset, 0)
    int fx_bits = 6, fx_frac = 2, fx_offset = 0;
    double fx_scale = 0.8125;
    // ALG_LMSA (ldpc_decoder_set_layers; greedy at create): layer of every check as the caller numbered it; on the device the checks
    // sorted by (layer, index) -- the processing order -- and on the host where each layer begins in that list ([nlayers + 1])
    std::vector<int32_t> layer_of_check, layer_start;
    DevBuf layer_order;
    // streaming workspace: set[0] holds the state when a decode begins, every frame repack moves it to the other set
    TileSet set[2];
    DevBuf c2v16;      // fp16 storage: check -> variable lines, rebuilt by every check pass (not part of a set: a repack does not move them)
    DevBuf rmap;       // folded repack: source (tile, lane) of every frame of the new set
    DevBuf rbase;      // repack plan: first destination slot of every source tile
    DevBuf flags;      // per-tile syndrome flags + the device poll ring behind them (LLR decoders: SweepPolls, ldpc_tiles.hpp)
    DevBuf graph_tab;  // variable-major view of the graph, built once (fp16 storage: edge_vpos; erasure: edge_vpos + chk_of_pos)
    DevBuf gridviol;   // exact-in-fp32 mode: device counter of guard events (LDPC_FLAG_PRIOR_GRID, ldpc_decoder_grid_violations)
    // staging: priors / received symbols / decisions / iteration counts of the *_host and simulate entry points, packed decisions and
    // erased mask of ldpc_decode_host, bit errors per frame of the streaming erasure simulation
    DevBuf h_in, h_y0, h_out, h_iters, h_bits, h_era, sim_errs;
    // THE list of a decoder's device buffers: destroy, the halving retry and the chunk sizing all walk it
    template <class F>
    void for_each_buffer(F&& f) {
        for (TileSet& s : set)
            for (DevBuf* b : {&s.edge, &s.node, &s.prior, &s.planes, &s.live, &s.fmap}) f(*b, BUF_STATE);
        for (DevBuf* b : {&c2v16, &rmap}) f(*b, BUF_STATE);
        for (DevBuf* b : {&rbase, &flags, &graph_tab, &gridviol, &layer_order}) f(*b, BUF_SHARED);
        for (DevBuf* b : {&h_in, &h_y0, &h_out, &h_iters, &h_bits, &h_era, &sim_errs}) f(*b, BUF_STAGING);
    }
    // fused backend
    FusedPlan* fused = nullptr;
    void* pinned = nullptr;  // small page-locked host block (the host side of the poll ring, counters)
    // low-latency host path (ldpc_decode_host, a few frames per call -- the reference's one-frame-per-call loop, src/main.py:37-48):
    // page-locked, device-mapped staging the decode kernel reads priors from and writes decisions to DIRECTLY (no copy engine in the
    // path), a private stream and one event recorded right behind the kernel
    void* lat_pin = nullptr;
    size_t lat_bytes = 0;
    hipStream_t lat_stream = nullptr;
    hipEvent_t lat_event = nullptr;
    // optional per-kernel timing with HIP events recorded on the decode stream (bench.py roofline leg)
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[4] = {0, 0, 0, 0};     // [0] check pass (ALG_LMSA: layer passes), [1] variable pass (ALG_LMSA: decision pass), [2] fused decode kernel, [3] whole streaming decode
    int64_t prof_launches[4] = {0, 0, 0, 0};
    // statistics of the last decode call
    int last_sweeps = 0;
    int last_backend = BK_STREAM;
    int last_repacks = 0;  // frame repacks of the last streaming decode
    int chunk_retries = 0;  // how often decode_dev halved the streaming chunk after a failed reservation (ldpc_decoder_chunk_state)
    int64_t stream_chunk = 0;  // frames per pass through the streaming kernels (0: not decided yet; ldpc_api.hip stream_chunk_frames)
};

// The parameters of a decoder's check rule as a launch hands them to its kernels (the setters are read at every launch):
//   corrected (ALG_NMSA, ALG_LMSA):  c2v = sign * max(scale * min - offset, 0); cap, step, vmax unused
//   fixed point (ALG_QMSA):  step = 2^fx_frac (priors -> levels), vmax = V = 2^(fx_bits - 1) - 1, offset = min(fx_offset, 4096) (beyond V <= 2047
//     every message is 0 already), cap = max(floor(scale * V) - offset, 0): what a saturated minimum sends
// in this order the five are the FX_SCALE .. FX_VMAX words of the LDS-resident kernels.
struct RuleParams {
    double scale = 1.0, offset = 0.0, cap = 0.0, step = 1.0, vmax = 0.0;
};
// LDPC_E_ARG if a fixed-point constant were not exact in fp32 (cannot happen for values ldpc_decoder_set_fixed_point accepts)
int rule_params(const Decoder* d, RuleParams* out);

// LDPC_FLAG_PRIOR_GRID: may this call have it?  (ldpc_api.hip)
int grid_guard_available(const Decoder* d, int bk, uint32_t flags, const char* who);

// event-pair bookkeeping used when Decoder::profile is set
struct ProfSpan {
    int kind;
    hipEvent_t a, b;
};
int prof_event(Decoder* d, size_t idx, hipEvent_t* out);
int prof_collect(Decoder* d, const std::vector<ProfSpan>& spans);

// ---- backends (each returns an LDPC_* code) -------------------------------------------------------
int stream_decode(Decoder* d, const DecodeCall& k);

// ALG_LMSA, host only: the layering `layer_of_check` ([m]; null: greedy -- every check takes the smallest layer none of whose checks
// shares a variable with it) checked and sorted into `of_check` / `sorted` (what Decoder::layer_order mirrors) / `start`.  LDPC_E_ARG, outputs untouched,
// for a negative entry or two checks of one layer that share a variable.
int layering_build(const Code* c, const int32_t* layer_of_check, std::vector<int32_t>* of_check, std::vector<int32_t>* sorted,
                   std::vector<int32_t>* start);

// bit-sliced erasure decoder on the streaming kernels (ldpc_bec_stream.hip)
int becs_stream_decode(Decoder* d, const DecodeCall& k);
int becs_stream_simulate(Decoder* d, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                         uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st);

int stream_simulate_biawgn(Decoder* d, const DecodeCall& k, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0);

int fused_plan_create(Decoder* d);
int fused_plan_host(const Code* c, int alg, int dtype, long moves, const char* out_dir, double* info4);  // host only, no device
void fused_plan_destroy(Decoder* d);
bool fused_supported(const Decoder* d);
bool fused_simulate_supported(const Decoder* d, int channel, double param, int hist_bins);
int fused_simulate(Decoder* d, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                   int32_t max_iter, uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st, int rounds = 1, uint64_t round_stride = 0);
bool fused_simulate_rounds_supported(const Decoder* d);
int fused_info(const Decoder* d, double* out8);
int fused_kernel_name(const Decoder* d, bool sim, char* buf, size_t len);
int fused_decode(Decoder* d, const DecodeCall& k);

// ---- channel / counting kernels -------------------------------------------------------------------
int channel_generate(int channel, int dtype, double param, int codeword, uint64_t seed, uint64_t stream_id,
                     uint64_t frame0, int64_t B, int32_t n, void* priors, uint8_t* y, hipStream_t st);
int channel_generate_words(int channel, int dtype, double param, int codeword, const uint8_t* codebook, int64_t K, uint64_t seed,
                           uint64_t stream_id, uint64_t frame0, int64_t B, int32_t n, void* priors, uint8_t* y, uint8_t* sent, hipStream_t st,
                           const unsigned long long* list = nullptr);
int channel_generate_list(int channel, int dtype, double param, int codeword, uint64_t seed, uint64_t stream_id, const uint64_t* list_dev, int64_t cap,
                          int32_t n, void* priors, hipStream_t st);
int count_errors_words(const uint8_t* xhat, const uint8_t* sent, int sent_per_frame, int codeword, const int32_t* iters, int64_t B, int32_t n,
                       int32_t hist_bins, int64_t* counters, hipStream_t st);
int count_errors_list(const uint8_t* xhat, int codeword, const int32_t* iters, const uint64_t* list_dev, int64_t rows, int32_t n, int32_t hist_bins,
                      int64_t* counters, int64_t counter_stride, uint64_t frame_base, uint64_t round_stride, int64_t nrounds, int64_t* redone2,
                      hipStream_t st);
int count_errors(const uint8_t* xhat, const uint8_t* sent, int codeword, const int32_t* iters, int64_t B, int32_t n,
                 int32_t max_iter_hist, int64_t* counters, hipStream_t st);

// ---- maximum-likelihood decoder of the short codes (ldpc_ml.hip) ------------------------------------
struct MlDecoder;
int ml_create(int device, const uint8_t* codebook, int64_t K, int32_t n, MlDecoder** out);
void ml_destroy(MlDecoder* d);
void ml_info(const MlDecoder* d, int64_t* K, int32_t* n, int32_t* W);
int ml_decode(MlDecoder* d, int channel, int dtype, const double* coef, const void* y, int64_t B, const uint32_t* pick,
              int32_t* index, int32_t* ties, uint32_t* tie_mask, double* best, uint8_t* xhat, hipStream_t st);
int ml_simulate(MlDecoder* d, int channel, int dtype, double param, int codeword, uint64_t seed, uint64_t stream_id,
                uint64_t frame0, int64_t B, int64_t* counters, hipStream_t st);

// ---- ADMM LP decoder (ldpc_admm.hip) -------------------------------------------------------------
struct AdmmDecoder;
int admm_create(Code* code, AdmmDecoder** out);
void admm_destroy(AdmmDecoder* d);
int admm_last_repacks(const AdmmDecoder* d);
int admm_last_backend(const AdmmDecoder* d);
int admm_decode(AdmmDecoder* d, const double* gamma, int64_t B, double mu, double eps, int32_t max_iter, double* x_out, int32_t* iters,
                uint8_t* converged, hipStream_t st);

// packed decisions: bit (v & 31) of word (v >> 5) of frame row f = decision of variable v; W = ceil(n / 32) words per frame
int pack_bits(const uint8_t* xhat, int64_t B, int32_t n, uint32_t* bits, uint32_t* erased, hipStream_t st);
int count_errors_bits(const uint32_t* bits, const uint32_t* erased, const uint32_t* sent_bits, int codeword, const int32_t* iters, int64_t B,
                      int32_t n, int32_t hist_bins, int64_t* counters, hipStream_t st);

int debug_copy4(const void* src, void* dst, int64_t nbytes, hipStream_t st);

constexpr uint32_t FLAG_NO_EARLY_EXIT = 1u;  // run exactly max_iter sweeps (NOT reference behaviour; benchmarking aid)

}  // namespace ldpc

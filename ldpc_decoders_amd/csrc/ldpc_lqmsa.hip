// Layered fixed-point min-sum with the whole frame resident in the LDS as integers (include/ldpc_hip.h, ldpc_lqmsa_*).
//
// One workgroup of NW waves owns one frame for all its sweeps; frames are handed out by an atomic dispenser, so the early exit is per
// frame and nothing is ever repacked.  In the LDS (lqmsa_lds_bytes, ldpc_lqmsa.hpp):
//     marg  int16 [n]            the marginals in levels; the priors are quantised on load (quantise_prior: LDPC_ALG_QMSA's quantiser)
//     c2v   int8  [m][row bytes] the check -> variable messages, one row per check at its position in the processing order
//     ctl   4 words              frame index, two syndrome flags used by alternate sweeps, spare
// Lane = check.  The checks of a layer touch disjoint variables, so within a layer no two lanes touch one marginal; neighbouring
// marginals share a dword, so they are read and written as 16-bit LDS accesses only, and a message row is owned by one lane.  A layer
// ends with a workgroup barrier; with NW = 1 that is the one-wave barrier (a workgroup of 64 threads: the compiler drains the wave's
// LDS queue and emits no cross-wave wait).
// Graph tables, per layering, in global memory (Lqmsa::lay / vtab / deg, rebuilt by lqmsa_set_layers): a layer of c checks is cut into
// ceil(c / 64) wave passes; pass k of the layer goes to wave k mod NW; vtab holds the 16-bit variable indices as [pass][edge][64 lanes].
// The rule itself, a frame's way into and out of the LDS, the frame hand-out and the host-side parameters and refusals are stated in
// ldpc_layered_fx.hpp for this decoder, QCMSA and SLQMSA; this file adds the tables and the walk over them.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ldpc_cn.hpp"
#include "ldpc_layered_fx.hpp"
#include "ldpc_lqmsa.hpp"

namespace ldpc {

struct Lqmsa {
    Code* code = nullptr;
    FixedPoint fx;
    int num_cu = 0, nw = 1, frames_per_cu = 0, row_bytes = 8;
    int64_t lds_bytes = 0;
    std::vector<int32_t> layer_of_check, layer_start;
    int32_t npasses = 0;
    DevBuf lay;   // int32 [nlayers + 1][2]: position of the layer's first check in the processing order, index of its first wave pass
    DevBuf vtab;  // uint16 [wave passes][dc_max][64]: variable of edge j of the check in lane L of the pass
    DevBuf deg;   // uint16 [m]: degree of the check at each position of the processing order
    DevBuf ctl;   // the frame dispenser
    SimStage sim;  // staging of ldpc_lqmsa_simulate
};

namespace {

struct LqArgs {
    const void* priors;
    const uint8_t* y0;
    int64_t B;
    int32_t n, m, row_bytes, dc_max, nlayers, cap, no_early;
    int32_t scale64, offset, vmax;
    double step;
    const int32_t* lay;
    const uint16_t* vtab;
    const uint16_t* deg;
    uint32_t* dispenser;
    uint8_t* xhat;
    uint32_t* bits;
    int32_t* iters;
    int16_t* soft;
};

template <typename T, int NW, bool ROW8>
__global__ __launch_bounds__(64 * NW) void k_lqmsa(const LqArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lq_sm[];
    constexpr int NT = 64 * NW;
    const int n = a.n, m = a.m;
    int16_t* marg = (int16_t*)lq_sm;
    uint8_t* c2v = (uint8_t*)lq_sm + ((size_t)2 * n + 7) / 8 * 8;
    uint32_t* ctl = (uint32_t*)(c2v + (size_t)m * a.row_bytes);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Wd = (n + 31) / 32;
    const T step = (T)a.step, vmax = (T)a.vmax;
    const int32_t* __restrict__ lay = a.lay;
    const uint16_t* __restrict__ deg = a.deg;
    for (;;) {
        const int64_t f = fx_draw_frame(a.dispenser, ctl, tid);
        if (f >= a.B) break;
        fx_load_frame<NT, T>((const T*)a.priors + (size_t)f * n, step, vmax, marg, (uint32_t*)c2v, n, m * (a.row_bytes / 4), tid);
        __syncthreads();
        const uint8_t* __restrict__ yf = a.y0 ? a.y0 + (size_t)f * n : nullptr;
        int it = 0;
        for (; it < a.cap; ++it) {
            if (!a.no_early && (it > 0 || yf)) {  // H x_hat = 0?  x_hat = (marg < 0); before the first sweep the received word
                // every wave scans its own passes and stops at the first one that holds an unsatisfied check: all but a frame's last
                // syndrome cost one pass
                bool bad = false;
                for (int l = 0; l < a.nlayers && !bad; ++l) {
                    const int s0 = lay[2 * l], q0 = lay[2 * l + 1], s1 = lay[2 * l + 2];
                    const int np = (s1 - s0 + 63) >> 6;
                    for (int k = w; k < np && !bad; k += NW) {
                        const int p = s0 + k * 64 + lane;
                        uint32_t par = 0;
                        if (p < s1) {
                            const uint16_t* __restrict__ vt = a.vtab + ((size_t)(q0 + k) * a.dc_max) * 64 + lane;
                            const int d = deg[p];
                            if (it == 0)
                                for (int j = 0; j < d; ++j) par ^= (uint32_t)(yf[vt[j * 64]] & 1u);
                            else
                                for (int j = 0; j < d; ++j) par ^= (uint32_t)(marg[vt[j * 64]] < 0);
                        }
                        bad = __ballot(par != 0u) != 0ull;  // wave-uniform
                    }
                }
                if (!fx_any_unsatisfied(ctl, bad, it, tid, lane)) break;
            }
            for (int l = 0; l < a.nlayers; ++l) {
                const int s0 = lay[2 * l], q0 = lay[2 * l + 1], s1 = lay[2 * l + 2];
                const int np = (s1 - s0 + 63) >> 6;
                for (int k = w; k < np; k += NW) {
                    const int p = s0 + k * 64 + lane;
                    if (p < s1) {  // the check at position p: its row of messages, its deg[p] variables in vt[j * 64]
                        const uint16_t* __restrict__ vt = a.vtab + ((size_t)(q0 + k) * a.dc_max) * 64 + lane;
                        const auto var = [vt](int j) -> uint32_t { return vt[j * 64]; };
                        if constexpr (ROW8)
                            fx_check_row8<8>(marg, (uint2*)(c2v + (size_t)p * 8), deg[p], var, a.scale64, a.offset, a.vmax);
                        else
                            fx_check_loop(marg, c2v + (size_t)p * a.row_bytes, deg[p], var, a.scale64, a.offset, a.vmax);
                    }
                }
                __syncthreads();
            }
        }
        // the frame leaves (ldpc_layered_fx.hpp fx_write_frame, kept inline here: see there).  it == 0: it left at the check of the received
        // word and keeps it (cap >= 1, so y0 was given)
        if (tid == 0) a.iters[f] = it;
        if (a.xhat)
            for (int v = tid; v < n; v += NT) a.xhat[(size_t)f * n + v] = it == 0 ? yf[v] : (uint8_t)(marg[v] < 0);
        if (a.soft)
            for (int v = tid; v < n; v += NT) a.soft[(size_t)f * n + v] = it == 0 ? (int16_t)0 : marg[v];
        if (a.bits)
            for (int v0 = w * 64; v0 < n; v0 += NT) {
                const int v = v0 + lane;
                const bool bit = v < n && (it == 0 ? (yf[v] & 1u) != 0u : marg[v] < 0);
                const unsigned long long b = __ballot(bit);
                if (lane == 0) {
                    uint32_t* out = a.bits + (size_t)f * Wd + (v0 >> 5);
                    out[0] = (uint32_t)b;
                    if ((v0 >> 5) + 1 < Wd) out[1] = (uint32_t)(b >> 32);
                }
            }
    }
}

template <typename T, int NW>
const void* kernel_of(bool row8) {
    return row8 ? (const void*)k_lqmsa<T, NW, true> : (const void*)k_lqmsa<T, NW, false>;
}
template <typename T>
const void* kernel_of(int nw, bool row8) {
    switch (nw) {
        case 1: return kernel_of<T, 1>(row8);
        case 2: return kernel_of<T, 2>(row8);
        case 4: return kernel_of<T, 4>(row8);
        default: return kernel_of<T, 8>(row8);
    }
}

// the tables of a layering (host side), in the order of layering_build's `sorted`
int install(Lqmsa* h, const int32_t* layer_of_check) {
    const Code* c = h->code;
    std::vector<int32_t> of_check, sorted, start;
    LDPC_TRY(layering_build(c, layer_of_check, &of_check, &sorted, &start));
    const int nl = (int)start.size() - 1;
    std::vector<int32_t> lay(2 * ((size_t)nl + 1));
    int64_t passes = 0;
    for (int l = 0; l <= nl; ++l) {
        lay[2 * (size_t)l] = start[(size_t)l];
        lay[2 * (size_t)l + 1] = (int32_t)passes;
        if (l < nl) passes += (start[(size_t)l + 1] - start[(size_t)l] + 63) / 64;
    }
    const size_t dc = (size_t)c->max_dc;
    if (passes * (int64_t)dc * 64 > ((int64_t)1 << 30)) {
        set_error("ldpc_lqmsa_set_layers: %lld wave passes: the layering is too fine for the index tables", (long long)passes);
        return LDPC_E_ARG;
    }
    std::vector<uint16_t> vtab((size_t)passes * dc * 64, 0), deg((size_t)c->m);
    for (int l = 0; l < nl; ++l)
        for (int32_t p = start[(size_t)l]; p < start[(size_t)l + 1]; ++p) {
            const int32_t cc = sorted[(size_t)p], k0 = c->row_ptr[cc], d = c->row_ptr[cc + 1] - k0;
            const size_t q = (size_t)lay[2 * (size_t)l + 1] + (size_t)(p - start[(size_t)l]) / 64, lane = (size_t)(p - start[(size_t)l]) % 64;
            deg[(size_t)p] = (uint16_t)d;
            for (int32_t j = 0; j < d; ++j) vtab[(q * dc + (size_t)j) * 64 + lane] = (uint16_t)c->edge_var[k0 + j];
        }
    // a decode of this handle still in flight reads the old tables
    LDPC_HIP_TRY(hipSetDevice(c->device));
    LDPC_HIP_TRY(hipDeviceSynchronize());
    LDPC_TRY(h->lay.reserve(lay.size() * sizeof(int32_t)));
    LDPC_TRY(h->vtab.reserve(std::max<size_t>(vtab.size(), 1) * sizeof(uint16_t)));
    LDPC_TRY(h->deg.reserve(deg.size() * sizeof(uint16_t)));
    LDPC_HIP_TRY(hipMemcpy(h->lay.p, lay.data(), lay.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!vtab.empty()) LDPC_HIP_TRY(hipMemcpy(h->vtab.p, vtab.data(), vtab.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    LDPC_HIP_TRY(hipMemcpy(h->deg.p, deg.data(), deg.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    h->layer_of_check.swap(of_check);
    h->layer_start.swap(start);
    h->npasses = (int32_t)passes;
    return LDPC_OK;
}

}  // namespace

int lqmsa_create(Code* code, Lqmsa** out) {
    LDPC_TRY(fx_check_degrees("ldpc_lqmsa_create", "check", code->min_dc, code->max_dv, LQMSA_MAX_DV));
    const int64_t need = lqmsa_lds_bytes(code->m, code->n, code->E, code->max_dc);
    if (need > LQMSA_LDS_BYTES || code->n > 65536) {
        set_error("ldpc_lqmsa_create: one frame of this code (m = %d, n = %d, dc_max = %d) needs %lld bytes of LDS, above one CU's %lld (and n <= 65536 "
                  "for the 16-bit index tables); use LDPC_ALG_LMSA (layered min-sum on the streaming kernels) for it",
                  code->m, code->n, code->max_dc, (long long)need, (long long)LQMSA_LDS_BYTES);
        return LDPC_E_UNSUPPORTED;
    }
    LDPC_HIP_TRY(hipSetDevice(code->device));
    Lqmsa* h = new Lqmsa();
    h->code = code;
    h->lds_bytes = need;
    h->row_bytes = lqmsa_row_bytes(code->max_dc);
    const int64_t fit = LQMSA_LDS_BYTES / need;
    h->nw = fx_waves(lqmsa_waves(fit), "LDPC_LQMSA_NW");
    h->frames_per_cu = fx_frames_per_cu(fit, h->nw);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, code->device);
    if (e == hipSuccess) e = fx_allow_lds(kernel_of<float>(h->nw, h->row_bytes == 8), kernel_of<double>(h->nw, h->row_bytes == 8), need);
    if (e != hipSuccess) {
        set_error("ldpc_lqmsa_create: device setup failed: %s", hipGetErrorString(e));
        lqmsa_destroy(h);
        return LDPC_E_HIP;
    }
    h->num_cu = prop.multiProcessorCount;
    int rc = h->ctl.reserve(64);
    if (rc == LDPC_OK) rc = install(h, nullptr);
    if (rc != LDPC_OK) {
        lqmsa_destroy(h);
        return rc;
    }
    *out = h;
    return LDPC_OK;
}

void lqmsa_destroy(Lqmsa* h) {
    if (!h) return;
    for (DevBuf* b : {&h->lay, &h->vtab, &h->deg, &h->ctl}) b->release();
    h->sim.release();
    delete h;
}

int lqmsa_set_fixed_point(Lqmsa* h, int bits, int frac_bits, double scale, int offset) {
    return h->fx.set("ldpc_lqmsa_set_fixed_point", bits, frac_bits, scale, offset);
}

void lqmsa_get_fixed_point(const Lqmsa* h, int* bits, int* frac_bits, double* scale, int* offset) { h->fx.get(bits, frac_bits, scale, offset); }

int lqmsa_set_layers(Lqmsa* h, const int32_t* layer_of_check, int32_t m) {
    if (layer_of_check && m != h->code->m) {
        set_error("ldpc_lqmsa_set_layers: %d entries for a code of %d checks", m, h->code->m);
        return LDPC_E_ARG;
    }
    return install(h, layer_of_check);
}

void lqmsa_get_layers(const Lqmsa* h, int32_t* nlayers, int32_t* layer_of_check) {
    *nlayers = (int32_t)h->layer_start.size() - 1;
    if (layer_of_check) std::copy(h->layer_of_check.begin(), h->layer_of_check.end(), layer_of_check);
}

void lqmsa_info(const Lqmsa* h, double* out4) {
    out4[0] = (double)h->lds_bytes;
    out4[1] = h->nw;
    out4[2] = h->frames_per_cu;
    out4[3] = (double)h->num_cu * h->frames_per_cu;
}

int lqmsa_decode(Lqmsa* h, int dtype, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat,
                 uint32_t* bits, int32_t* iters, int16_t* soft, hipStream_t st) {
    LDPC_TRY(fx_check_decode("ldpc_lqmsa_decode", dtype, flags, B));
    const Code* c = h->code;
    LDPC_HIP_TRY(hipSetDevice(c->device));
    if (B == 0) return LDPC_OK;
    LqArgs a;
    fx_fill_args(a, c, h->fx, h->row_bytes, h->ctl.p, priors, y0, B, max_iter, flags, xhat, bits, iters, soft);
    a.dc_max = c->max_dc;
    a.nlayers = (int32_t)h->layer_start.size() - 1;
    a.lay = (const int32_t*)h->lay.p;
    a.vtab = (const uint16_t*)h->vtab.p;
    a.deg = (const uint16_t*)h->deg.p;
    LDPC_HIP_TRY(hipMemsetAsync(a.dispenser, 0, 4, st));
    const unsigned groups = (unsigned)std::min<int64_t>(B, (int64_t)h->num_cu * h->frames_per_cu);
    const void* kern = dtype == DT_F64 ? kernel_of<double>(h->nw, h->row_bytes == 8) : kernel_of<float>(h->nw, h->row_bytes == 8);
    void* args[] = {(void*)&a};
    LDPC_HIP_TRY(hipLaunchKernel(kern, dim3(groups), dim3(64u * (unsigned)h->nw), args, (size_t)h->lds_bytes, st));
    return LDPC_OK;
}

int lqmsa_simulate(Lqmsa* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                   uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st) {
    return fx_simulate("ldpc_lqmsa_simulate", h->code, h->sim, fx_lds_sim_cap(h->code->n), channel, param, codeword, seed, stream_id, frame0, B,
                       hist_bins, counters, st, [&](const void* pri, const uint8_t* y, int64_t nb, uint32_t* bits, int32_t* iters) {
                           return lqmsa_decode(h, DT_F32, pri, y, nb, max_iter, flags, nullptr, bits, iters, nullptr, st);
                       });
}

}  // namespace ldpc

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
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ldpc_cn.hpp"
#include "ldpc_lqmsa.hpp"

namespace ldpc {

struct Lqmsa {
    Code* code = nullptr;
    int bits = 6, frac = 2, offset = 0;
    double scale = 0.8125;
    bool odd_check = false;
    int num_cu = 0, nw = 1, frames_per_cu = 0, row_bytes = 8;
    int64_t lds_bytes = 0;
    std::vector<int32_t> layer_of_check, layer_start;
    int32_t npasses = 0;
    DevBuf lay;   // int32 [nlayers + 1][2]: position of the layer's first check in the processing order, index of its first wave pass
    DevBuf vtab;  // uint16 [wave passes][dc_max][64]: variable of edge j of the check in lane L of the pass
    DevBuf deg;   // uint16 [m]: degree of the check at each position of the processing order
    DevBuf ctl;   // the frame dispenser
    DevBuf sim_pri, sim_y, sim_bits, sim_iters;  // staging of ldpc_lqmsa_simulate
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

// |c2v| a minimum m <= V sends
__device__ __forceinline__ int lq_mag(int m, int scale64, int offset) {
    const int t = ((scale64 * m) >> 6) - offset;
    return t > 0 ? t : 0;
}

// One check: the row of messages of position p, its `deg` variables in vt[j * 64].  ROW8: the row is 8 bytes, held in registers.
template <bool ROW8>
__device__ __forceinline__ void lq_check(int16_t* __restrict__ marg, uint8_t* __restrict__ c2v, int p, int deg, const uint16_t* __restrict__ vt, int row_bytes,
                                         int scale64, int offset, int V) {
    int min1 = V, min2 = V, arg = -1;  // |v| enters as min(|v|, V), so V is the neutral element
    uint32_t par = 0;
    if constexpr (ROW8) {
        uint2* rowp = (uint2*)(c2v + (size_t)p * 8);
        const uint2 row = *rowp;
        const uint32_t rw[2] = {row.x, row.y};
        int v[8];
        uint32_t vi[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < deg) {
                vi[j] = vt[j * 64];
                v[j] = (int)marg[vi[j]] - (int)(int8_t)(rw[j >> 2] >> (8 * (j & 3)));
                const int a = min(abs(v[j]), V);
                par ^= (uint32_t)(v[j] < 0);
                if (a < min1) {
                    min2 = min1;
                    min1 = a;
                    arg = j;
                } else if (a < min2) {
                    min2 = a;
                }
            }
        }
        const int f1 = lq_mag(min1, scale64, offset), f2 = lq_mag(min2, scale64, offset);
        uint32_t out[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < deg) {
                const int mag = j == arg ? f2 : f1;
                const int c = (par ^ (uint32_t)(v[j] < 0)) ? -mag : mag;
                marg[vi[j]] = (int16_t)(v[j] + c);
                out[j >> 2] |= (uint32_t)(uint8_t)(int8_t)c << (8 * (j & 3));
            }
        }
        *rowp = make_uint2(out[0], out[1]);
    } else {
        uint8_t* row = c2v + (size_t)p * row_bytes;
        for (int j = 0; j < deg; ++j) {
            const int v = (int)marg[vt[j * 64]] - (int)(int8_t)row[j];
            const int a = min(abs(v), V);
            par ^= (uint32_t)(v < 0);
            if (a < min1) {
                min2 = min1;
                min1 = a;
                arg = j;
            } else if (a < min2) {
                min2 = a;
            }
        }
        const int f1 = lq_mag(min1, scale64, offset), f2 = lq_mag(min2, scale64, offset);
        for (int j = 0; j < deg; ++j) {
            const uint32_t vi = vt[j * 64];
            const int v = (int)marg[vi] - (int)(int8_t)row[j];
            const int mag = j == arg ? f2 : f1;
            const int c = (par ^ (uint32_t)(v < 0)) ? -mag : mag;
            marg[vi] = (int16_t)(v + c);
            row[j] = (uint8_t)(int8_t)c;
        }
    }
}

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
        __syncthreads();  // the frame before is written out
        if (tid == 0) {
            ctl[0] = atomicAdd(a.dispenser, 1u);
            ctl[1] = 0u;
            ctl[2] = 0u;
        }
        __syncthreads();
        const int64_t f = ctl[0];
        if (f >= a.B) break;
        const T* __restrict__ pr = (const T*)a.priors + (size_t)f * n;
        for (int v = tid; v < n; v += NT) marg[v] = (int16_t)(int)quantise_prior<T>(pr[v], step, vmax);
        uint32_t* cw = (uint32_t*)c2v;
        for (int i = tid; i < m * (a.row_bytes / 4); i += NT) cw[i] = 0u;
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
                if (bad && lane == 0) ctl[1 + (it & 1)] = 1u;
                __syncthreads();
                const bool any = ctl[1 + (it & 1)] != 0u;
                if (tid == 0) ctl[1 + ((it + 1) & 1)] = 0u;  // last read a sweep ago, next written a sweep (and a layer barrier) from now
                if (!any) break;
            }
            for (int l = 0; l < a.nlayers; ++l) {
                const int s0 = lay[2 * l], q0 = lay[2 * l + 1], s1 = lay[2 * l + 2];
                const int np = (s1 - s0 + 63) >> 6;
                for (int k = w; k < np; k += NW) {
                    const int p = s0 + k * 64 + lane;
                    if (p < s1)
                        lq_check<ROW8>(marg, c2v, p, deg[p], a.vtab + ((size_t)(q0 + k) * a.dc_max) * 64 + lane, a.row_bytes, a.scale64, a.offset, a.vmax);
                }
                __syncthreads();
            }
        }
        // it == 0: the frame left at the check of the received word and keeps it (cap >= 1, so y0 was given)
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
    if (code->min_dc < 2) {
        set_error("ldpc_lqmsa_create: a check of degree %d: layered min-sum needs every check to have degree >= 2", code->min_dc);
        return LDPC_E_UNSUPPORTED;
    }
    if (code->max_dv > LQMSA_MAX_DV) {
        set_error("ldpc_lqmsa_create: a variable of degree %d: the int16 marginals hold V (1 + dv) for dv <= %d", code->max_dv, LQMSA_MAX_DV);
        return LDPC_E_UNSUPPORTED;
    }
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
    for (int32_t c = 0; c < code->m; ++c) h->odd_check |= ((code->row_ptr[c + 1] - code->row_ptr[c]) & 1) != 0;
    const int64_t fit = LQMSA_LDS_BYTES / need;
    h->nw = lqmsa_waves(fit);
    if (const char* env = std::getenv("LDPC_LQMSA_NW")) {  // the tests reach every wave count with it
        const int v = std::atoi(env);
        if (v == 1 || v == 2 || v == 4 || v == 8) h->nw = v;
    }
    h->frames_per_cu = (int)std::min<int64_t>(fit, 32 / h->nw);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, code->device);
    if (e == hipSuccess && need > 64 * 1024) {  // above 64 KiB a workgroup's LDS has to be asked for
        const bool row8 = h->row_bytes == 8;
        e = hipFuncSetAttribute(kernel_of<float>(h->nw, row8), hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
        if (e == hipSuccess) e = hipFuncSetAttribute(kernel_of<double>(h->nw, row8), hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
    }
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
    for (DevBuf* b : {&h->lay, &h->vtab, &h->deg, &h->ctl, &h->sim_pri, &h->sim_y, &h->sim_bits, &h->sim_iters}) b->release();
    delete h;
}

int lqmsa_set_fixed_point(Lqmsa* h, int bits, int frac_bits, double scale, int offset) {
    // (written so that a NaN scale fails; 64 * scale is exact, so the grid test is)
    if (bits < 2 || bits > 8 || frac_bits < -8 || frac_bits > 8 || !(scale > 0.0 && scale <= 1.0) || 64.0 * scale != (double)(long long)(64.0 * scale) ||
        offset < 0) {
        set_error("ldpc_lqmsa_set_fixed_point: 2 <= bits <= 8, -8 <= frac_bits <= 8, scale a multiple of 1/64 in (0, 1] and offset >= 0 are needed "
                  "(bits=%d frac_bits=%d scale=%g offset=%d)", bits, frac_bits, scale, offset);
        return LDPC_E_ARG;
    }
    h->bits = bits;
    h->frac = frac_bits;
    h->scale = scale;
    h->offset = offset;
    return LDPC_OK;
}

void lqmsa_get_fixed_point(const Lqmsa* h, int* bits, int* frac_bits, double* scale, int* offset) {
    *bits = h->bits;
    *frac_bits = h->frac;
    *scale = h->scale;
    *offset = h->offset;
}

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
    if (dtype != DT_F32 && dtype != DT_F64) {
        set_error("ldpc_lqmsa_decode: the priors are LDPC_DTYPE_F32 or LDPC_DTYPE_F64 (got %d)", dtype);
        return LDPC_E_ARG;
    }
    if (flags & ~FLAG_NO_EARLY_EXIT) {
        set_error("ldpc_lqmsa_decode: the only flag is LDPC_FLAG_NO_EARLY_EXIT (got 0x%x)", flags);
        return LDPC_E_UNSUPPORTED;
    }
    if (B > (int64_t)1 << 31) {
        set_error("ldpc_lqmsa_decode: at most 2^31 frames per call (got %lld)", (long long)B);
        return LDPC_E_ARG;
    }
    const Code* c = h->code;
    LDPC_HIP_TRY(hipSetDevice(c->device));
    if (B == 0) return LDPC_OK;
    LqArgs a;
    a.priors = priors;
    a.y0 = y0;
    a.B = B;
    a.n = c->n;
    a.m = c->m;
    a.row_bytes = h->row_bytes;
    a.dc_max = c->max_dc;
    a.nlayers = (int32_t)h->layer_start.size() - 1;
    a.cap = max_iter > 0 ? max_iter : 100000;
    a.no_early = (flags & FLAG_NO_EARLY_EXIT) ? 1 : 0;
    a.scale64 = (int32_t)(64.0 * h->scale);
    a.offset = std::min(h->offset, 1 << 20);  // beyond V every message is 0 already
    a.vmax = (1 << (h->bits - 1)) - 1;
    a.step = std::ldexp(1.0, h->frac);
    a.lay = (const int32_t*)h->lay.p;
    a.vtab = (const uint16_t*)h->vtab.p;
    a.deg = (const uint16_t*)h->deg.p;
    a.dispenser = (uint32_t*)h->ctl.p;
    a.xhat = xhat;
    a.bits = bits;
    a.iters = iters;
    a.soft = soft;
    LDPC_HIP_TRY(hipMemsetAsync(a.dispenser, 0, 4, st));
    const unsigned groups = (unsigned)std::min<int64_t>(B, (int64_t)h->num_cu * h->frames_per_cu);
    const void* kern = dtype == DT_F64 ? kernel_of<double>(h->nw, h->row_bytes == 8) : kernel_of<float>(h->nw, h->row_bytes == 8);
    void* args[] = {(void*)&a};
    LDPC_HIP_TRY(hipLaunchKernel(kern, dim3(groups), dim3(64u * (unsigned)h->nw), args, (size_t)h->lds_bytes, st));
    return LDPC_OK;
}

int lqmsa_simulate(Lqmsa* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                   uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st) {
    if (channel != CH_BIAWGN && channel != CH_BSC) {
        set_error("ldpc_lqmsa_simulate: LDPC_CH_BIAWGN or LDPC_CH_BSC (min-sum has no magnitudes to work on over the erasure channel)");
        return LDPC_E_ARG;
    }
    if (codeword != 0 && codeword != 1) {
        set_error("ldpc_lqmsa_simulate: codeword must be 0 or 1");
        return LDPC_E_ARG;
    }
    if (codeword == 1 && h->odd_check) {
        set_error("ldpc_lqmsa_simulate: codeword 1: the all-ones word is no codeword of this code (a check has odd degree)");
        return LDPC_E_ARG;
    }
    const size_t n = (size_t)h->code->n, W = (n + 31) / 32;
    // the priors of one pass: about 256 MiB, at most 2^17 frames
    int64_t cap = std::min<int64_t>(std::max<int64_t>((int64_t)(((size_t)256 << 20) / (n * sizeof(float))), 1), (int64_t)1 << 17);
    cap = std::min(cap, std::max<int64_t>(B, 1));
    LDPC_HIP_TRY(hipSetDevice(h->code->device));
    LDPC_TRY(h->sim_pri.reserve((size_t)cap * n * sizeof(float)));
    if (channel == CH_BSC) LDPC_TRY(h->sim_y.reserve((size_t)cap * n));
    LDPC_TRY(h->sim_bits.reserve((size_t)cap * W * 4));
    LDPC_TRY(h->sim_iters.reserve((size_t)cap * sizeof(int32_t)));
    uint8_t* y = channel == CH_BSC ? (uint8_t*)h->sim_y.p : nullptr;  // over the BSC the received word takes the iteration-0 check, as upstream
    for (int64_t b0 = 0; b0 < B; b0 += cap) {
        const int64_t nb = std::min(cap, B - b0);
        LDPC_TRY(channel_generate(channel, DT_F32, param, codeword, seed, stream_id, frame0 + (uint64_t)b0, nb, (int32_t)n, h->sim_pri.p, y, st));
        LDPC_TRY(lqmsa_decode(h, DT_F32, h->sim_pri.p, y, nb, max_iter, flags, nullptr, (uint32_t*)h->sim_bits.p, (int32_t*)h->sim_iters.p, nullptr, st));
        LDPC_TRY(count_errors_bits((const uint32_t*)h->sim_bits.p, nullptr, nullptr, codeword, (const int32_t*)h->sim_iters.p, nb, (int32_t)n, hist_bins,
                                   counters, st));
    }
    return LDPC_OK;
}

}  // namespace ldpc

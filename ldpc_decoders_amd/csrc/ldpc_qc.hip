// Layered fixed-point min-sum for quasi-cyclic codes, shift-addressed (include/ldpc_hip.h, ldpc_qc_*).
//
// H is an mb x nb array of Z x Z blocks, each zero or a cyclically shifted identity: check i Z + r meets, in block column j, variable
// j Z + (r + s_ij) mod Z.  A block row is a layer (its Z checks touch disjoint variables), its degree is the same for all its checks, and a
// lane's variable index is its row r plus two wave-uniform scalars: there is no index table and no degree table.  The arithmetic, a frame's
// way in and out and the frame hand-out are those of ldpc_layered_fx.hpp, shared with LQMSA; so is LQMSA's LDS layout (lqmsa_lds_bytes with
// dc_max = the largest block-row degree):
//     marg  int16 [n]            the marginals in levels
//     c2v   int8  [m][row bytes] the check -> variable messages, the row of check c at c, byte j for the block row's j-th nonzero block
//     ctl   4 words              frame index, two syndrome flags used by alternate sweeps, spare
// One workgroup of NW waves owns one frame; lane L of pass k of a block row owns check i Z + 64 k + L, pass k goes to wave k mod NW; a block
// row ends with a workgroup barrier.  Neighbouring lanes touch neighbouring int16 marginals (up to the one wrap), which share a dword, so
// marginals are read and written as 16-bit LDS accesses only.  For Z <= 32 a second kernel, k_qc_pack below, puts several frames into a wave.
// Table (Qc::tab, rebuilt by qc_set_order), in global memory in processing order and read with wave-uniform addresses through the constant
// address space, so every entry arrives by a scalar load: per block row {degree, offset of its edges, i Z, 0}, per edge {j Z, shift}.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>

#include "ldpc_cn.hpp"
#include "ldpc_layered_fx.hpp"
#include "ldpc_qc.hpp"

namespace ldpc {

struct Qc {
    Code* code = nullptr;
    int32_t Z = 1, mb = 0, nb = 0, dc_max = 0;
    FixedPoint fx;
    int num_cu = 0, nw = 1, frames_per_cu = 0, row_bytes = 8;
    int64_t lds_bytes = 0;
    int pack = 1, pack_grid = 0;  // frames per wave (>= 2: k_qc_pack); LDPC_QC_PACK_GRID, 0 = no cap on the packed kernel's grid
    std::vector<int32_t> row_ptr, col, shift;  // the base matrix by block rows: nonzero blocks of block row i are row_ptr[i] .. row_ptr[i + 1]
    std::vector<int32_t> order;                // block row processed at each position
    DevBuf tab;                                // int32: [mb][4] headers in processing order, then [nonzero blocks][2]
    DevBuf ctl;                                // the frame dispenser
    SimStage sim;                              // staging of ldpc_qc_simulate
};

namespace {

typedef const int32_t __attribute__((address_space(4)))* qc_tab_t;  // uniform address + constant address space = scalar load

struct QcArgs {
    const void* priors;
    const uint8_t* y0;
    int64_t B;
    int32_t n, m, Z, mb, row_bytes, cap, no_early;
    int32_t scale64, offset, vmax;
    double step;
    const int32_t* tab;
    uint32_t* dispenser;
    uint8_t* xhat;
    uint32_t* bits;
    int32_t* iters;
    int16_t* soft;
};

// variable of row r in the block {colZ, shift}: e[0] + (r + e[1]) mod Z
__device__ __forceinline__ int qc_var(int r, int Z, int colZ, int shift) {
    const int t = r + shift;
    return colZ + (t < Z ? t : t - Z);
}

// One check of a block row: row r of its Z, the message row `row` of the frame, the `deg` blocks in e[2 j], e[2 j + 1].  deg is wave-uniform: the
// dispatch is a scalar branch.
template <bool ROW8>
__device__ __forceinline__ void qc_check(int16_t* __restrict__ marg, uint8_t* __restrict__ c2v, int row, int r, int Z, int deg, qc_tab_t e, const QcArgs& a) {
    const auto var = [=](int j) { return qc_var(r, Z, e[2 * j], e[2 * j + 1]); };
    if constexpr (ROW8) {
        uint2* rowp = (uint2*)(c2v + (size_t)row * 8);
        switch (deg) {
            case 2: fx_check_row8<2>(marg, rowp, 2, var, a.scale64, a.offset, a.vmax); break;
            case 3: fx_check_row8<3>(marg, rowp, 3, var, a.scale64, a.offset, a.vmax); break;
            case 4: fx_check_row8<4>(marg, rowp, 4, var, a.scale64, a.offset, a.vmax); break;
            case 5: fx_check_row8<5>(marg, rowp, 5, var, a.scale64, a.offset, a.vmax); break;
            case 6: fx_check_row8<6>(marg, rowp, 6, var, a.scale64, a.offset, a.vmax); break;
            case 7: fx_check_row8<7>(marg, rowp, 7, var, a.scale64, a.offset, a.vmax); break;
            default: fx_check_row8<8>(marg, rowp, 8, var, a.scale64, a.offset, a.vmax); break;
        }
    } else {
        fx_check_loop(marg, c2v + (size_t)row * a.row_bytes, deg, var, a.scale64, a.offset, a.vmax);
    }
}

template <typename T, int NW, bool ROW8>
__global__ __launch_bounds__(64 * NW) void k_qc(const QcArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t qc_sm[];
    constexpr int NT = 64 * NW;
    const int n = a.n, m = a.m, Z = a.Z, mb = a.mb;
    int16_t* marg = (int16_t*)qc_sm;
    uint8_t* c2v = (uint8_t*)qc_sm + ((size_t)2 * n + 7) / 8 * 8;
    uint32_t* ctl = (uint32_t*)(c2v + (size_t)m * a.row_bytes);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Wd = (n + 31) / 32;
    const int np = (Z + 63) >> 6;  // wave passes of a block row
    const T step = (T)a.step, vmax = (T)a.vmax;
    const qc_tab_t tab = (qc_tab_t)a.tab;
    for (;;) {
        const int64_t f = fx_draw_frame(a.dispenser, ctl, tid);
        if (f >= a.B) break;
        fx_load_frame<NT, T>((const T*)a.priors + (size_t)f * n, step, vmax, marg, (uint32_t*)c2v, n, m * (a.row_bytes / 4), tid);
        __syncthreads();
        const uint8_t* __restrict__ yf = a.y0 ? a.y0 + (size_t)f * n : nullptr;
        int it = 0;
        for (; it < a.cap; ++it) {
            if (!a.no_early && (it > 0 || yf)) {  // H x_hat = 0?  x_hat = (marg < 0); before the first sweep the received word
                // every wave scans its own passes and stops at the first one that holds an unsatisfied check
                bool bad = false;
                for (int l = 0; l < mb && !bad; ++l) {
                    const int deg = tab[4 * l];
                    const qc_tab_t e = tab + tab[4 * l + 1];
                    for (int k = w; k < np && !bad; k += NW) {
                        const int r = k * 64 + lane;
                        uint32_t par = 0;
                        if (r < Z) {
                            if (it == 0)
                                for (int j = 0; j < deg; ++j) par ^= (uint32_t)(yf[qc_var(r, Z, e[2 * j], e[2 * j + 1])] & 1u);
                            else
                                for (int j = 0; j < deg; ++j) par ^= (uint32_t)(marg[qc_var(r, Z, e[2 * j], e[2 * j + 1])] < 0);
                        }
                        bad = __ballot(par != 0u) != 0ull;  // wave-uniform
                    }
                }
                if (!fx_any_unsatisfied(ctl, bad, it, tid, lane)) break;
            }
            for (int l = 0; l < mb; ++l) {
                const int deg = tab[4 * l];  // wave-uniform: the dispatch below is a scalar branch
                const qc_tab_t e = tab + tab[4 * l + 1];
                const int row0 = tab[4 * l + 2];
                for (int k = w; k < np; k += NW) {
                    const int r = k * 64 + lane;
                    if (r < Z) qc_check<ROW8>(marg, c2v, row0 + r, r, Z, deg, e, a);
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
    return row8 ? (const void*)k_qc<T, NW, true> : (const void*)k_qc<T, NW, false>;
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

// ---- several frames per wave: Z <= 32, a block row is one pass and floor(64 / Z) frames fill the lanes a single frame leaves dark ----
// One workgroup of one wave owns P frame slots.  Lane L serves slot g = L / Z with row r = L - g Z; lanes >= P Z idle.  Slot g keeps its own
// frame image, the layout above, at byte g * stride of the LDS (qc_pack_stride); the table is shared and still read by scalar loads, the
// degree dispatch is still a scalar branch.  The slots are independent: each has its own frame index and sweep count (held by its lanes), its
// syndrome is the wave's ballot under the slot's lane mask, and a slot whose frame has left is served at once -- outputs written, the next
// frame drawn, again for as long as a fresh frame leaves on its received word -- while the others keep their state.  Serving is done by
// the whole wave (64 lanes over a frame's n values), one slot after the other, and the slots served together draw their frames with one
// atomic on the dispenser (one word takes a bounded number of returning atomics per microsecond, and short frames reach that bound).
struct QcPackArgs {
    QcArgs a;
    int32_t P, stride;
};

constexpr uint32_t QC_NO_FRAME = 0xffffffffu;  // frame indices stay below 2^31

template <typename T, bool ROW8>
__global__ __launch_bounds__(64) void k_qc_pack(const QcPackArgs pa) {
    extern __shared__ __attribute__((aligned(16))) uint32_t qc_sm[];
    const QcArgs& a = pa.a;
    const int n = a.n, m = a.m, Z = a.Z, mb = a.mb;
    const int lane = threadIdx.x;
    const size_t c2v_at = ((size_t)2 * n + 7) / 8 * 8;
    const T step = (T)a.step, vmax = (T)a.vmax;
    const qc_tab_t tab = (qc_tab_t)a.tab;
    const bool live = lane < pa.P * Z;
    const int g = live ? lane / Z : 0;  // computed once
    const int r = lane - g * Z;
    const unsigned long long slot0 = (1ull << Z) - 1ull;                 // the lanes of slot 0
    const unsigned long long mine = live ? slot0 << (g * Z) : 0ull;      // the lanes of this lane's slot
    int16_t* const marg = (int16_t*)((uint8_t*)qc_sm + (size_t)g * pa.stride);
    uint8_t* const c2v = (uint8_t*)marg + c2v_at;
    uint32_t f = QC_NO_FRAME;  // the slot's frame and its sweeps so far, the same in all lanes of a slot
    int it = 0;
    bool need = live;  // the slot's frame has left (or it never had one)
    for (;;) {
        // serve the slots whose frame has left; a round: write their frames out, draw as many new ones, check the received words, load
        for (unsigned long long todo = __ballot(need); todo != 0ull;) {
            int k = 0;
            for (unsigned long long t = todo; t != 0ull; ++k) {
                const int lead = __ffsll((long long)t) - 1;
                const int g0 = __builtin_amdgcn_readlane(g, lead);
                const uint32_t f0 = (uint32_t)__builtin_amdgcn_readlane((int)f, lead);
                if (f0 != QC_NO_FRAME)
                    fx_write_frame<64>(a.y0, a.xhat, a.soft, a.bits, a.iters, n, (const int16_t*)((uint8_t*)qc_sm + (size_t)g0 * pa.stride), f0,
                                       __builtin_amdgcn_readlane(it, lead), lane, lane, 0);
                t &= ~(slot0 << (g0 * Z));
            }
            uint32_t drawn = 0u;
            if (lane == 0) drawn = atomicAdd(a.dispenser, (uint32_t)k);  // frames drawn .. drawn + k - 1, in slot order
            drawn = (uint32_t)__builtin_amdgcn_readfirstlane((int)drawn);
            __syncthreads();  // the outputs above have read the images
            unsigned long long again = 0ull;
            for (unsigned long long t = todo; t != 0ull; ++drawn) {
                const int lead = __ffsll((long long)t) - 1;
                const int g0 = __builtin_amdgcn_readlane(g, lead);
                const unsigned long long lanes0 = slot0 << (g0 * Z);
                t &= ~lanes0;
                uint32_t f0 = drawn;
                if ((int64_t)f0 >= a.B) {
                    f0 = QC_NO_FRAME;  // the slot is dead
                } else {
                    bool bad = true;
                    if (!a.no_early && a.y0) {  // H y0 = 0?  Then the frame leaves before its priors are read, and the slot draws again
                        const uint8_t* __restrict__ yf = a.y0 + (size_t)f0 * n;
                        bad = false;
                        for (int l = 0; l < mb && !bad; ++l) {
                            const int deg = tab[4 * l];
                            const qc_tab_t e = tab + tab[4 * l + 1];
                            uint32_t par = 0;
                            if (lane < Z)
                                for (int j = 0; j < deg; ++j) par ^= (uint32_t)(yf[qc_var(lane, Z, e[2 * j], e[2 * j + 1])] & 1u);
                            bad = __ballot(par != 0u) != 0ull;  // wave-uniform
                        }
                    }
                    if (bad) {
                        int16_t* const marg0 = (int16_t*)((uint8_t*)qc_sm + (size_t)g0 * pa.stride);
                        fx_load_frame<64, T>((const T*)a.priors + (size_t)f0 * n, step, vmax, marg0, (uint32_t*)((uint8_t*)marg0 + c2v_at), n,
                                             m * (a.row_bytes / 4), lane);
                    } else {
                        again |= lanes0;  // written out with 0 sweeps in the next round
                    }
                }
                if ((mine >> lead) & 1ull) {  // the lanes of slot g0
                    f = f0;
                    it = 0;
                }
            }
            todo = again;
        }
        const bool active = f != QC_NO_FRAME;
        if (__ballot(active) == 0ull) break;
        __syncthreads();  // the new images are in place
        for (int l = 0; l < mb; ++l) {
            const int deg = tab[4 * l];  // wave-uniform: the dispatch below is a scalar branch
            const qc_tab_t e = tab + tab[4 * l + 1];
            const int row0 = tab[4 * l + 2];
            if (active) qc_check<ROW8>(marg, c2v, row0 + r, r, Z, deg, e, a);
            __syncthreads();  // one wave: orders the block rows' LDS accesses, no hardware barrier
        }
        if (active) ++it;
        // who leaves: at the cap without a look, else when H x_hat = 0, x_hat = (marg < 0); a slot's verdict is the ballot under its mask
        const bool look = active && it < a.cap && !a.no_early;
        bool bad = false;
        unsigned long long open = __ballot(look);  // lanes of slots not yet known to hold an unsatisfied check
        for (int l = 0; l < mb && open != 0ull; ++l) {
            const int deg = tab[4 * l];
            const qc_tab_t e = tab + tab[4 * l + 1];
            uint32_t par = 0;
            if (look && !bad)
                for (int j = 0; j < deg; ++j) par ^= (uint32_t)(marg[qc_var(r, Z, e[2 * j], e[2 * j + 1])] < 0);
            bad = bad || (__ballot(par != 0u) & mine) != 0ull;
            open = __ballot(look && !bad);
        }
        need = active && (it >= a.cap || (look && !bad));
    }
}

template <typename T>
const void* pack_kernel_of(bool row8) {
    return row8 ? (const void*)k_qc_pack<T, true> : (const void*)k_qc_pack<T, false>;
}

// the table of a processing order (host side) and its upload
int install(Qc* h, const std::vector<int32_t>& order) {
    const Code* c = h->code;
    const size_t mb = (size_t)h->mb;
    std::vector<int32_t> tab(4 * mb + 2 * h->col.size());
    size_t at = 4 * mb;
    for (size_t l = 0; l < mb; ++l) {
        const int32_t i = order[l], k0 = h->row_ptr[(size_t)i], k1 = h->row_ptr[(size_t)i + 1];
        tab[4 * l] = k1 - k0;
        tab[4 * l + 1] = (int32_t)at;
        tab[4 * l + 2] = i * h->Z;
        tab[4 * l + 3] = 0;
        for (int32_t k = k0; k < k1; ++k) {
            tab[at++] = h->col[(size_t)k] * h->Z;
            tab[at++] = h->shift[(size_t)k];
        }
    }
    // a decode of this handle still in flight reads the old table
    LDPC_HIP_TRY(hipSetDevice(c->device));
    LDPC_HIP_TRY(hipDeviceSynchronize());
    LDPC_TRY(h->tab.reserve(std::max<size_t>(tab.size(), 1) * sizeof(int32_t)));
    if (!tab.empty()) LDPC_HIP_TRY(hipMemcpy(h->tab.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    h->order = order;
    return LDPC_OK;
}

// the base matrix of `code` for the lifting size Z into h (row_ptr / col / shift), O(E + mb + nb); LDPC_E_UNSUPPORTED names the first block
// that is neither zero nor one shifted identity
int detect(const Code* code, int32_t Z, Qc* h) {
    const int32_t mb = code->m / Z, nb = code->n / Z;
    std::vector<int32_t> sh((size_t)nb, -1), cnt((size_t)nb, 0), seen_in((size_t)nb, -1), touched;
    h->row_ptr.assign(1, 0);
    h->col.clear();
    h->shift.clear();
    for (int32_t i = 0; i < mb; ++i) {
        touched.clear();
        for (int32_t r = 0; r < Z; ++r) {
            const int32_t c = i * Z + r;
            for (int32_t k = code->row_ptr[c]; k < code->row_ptr[c + 1]; ++k) {
                const int32_t v = code->edge_var[k], j = v / Z, s = (v % Z - r + Z) % Z;
                bool ok = seen_in[(size_t)j] != c;  // a second one of this block in the row
                seen_in[(size_t)j] = c;
                if (ok && cnt[(size_t)j] == 0) {
                    sh[(size_t)j] = s;
                    touched.push_back(j);
                } else if (ok) {
                    ok = sh[(size_t)j] == s;
                }
                if (!ok) {
                    set_error("ldpc_qc_create: block (%d, %d) of the %d x %d base at Z = %d is neither zero nor one cyclically shifted identity (row %d of "
                              "the block); use ldpc_lqmsa_create (LQMSA, any layering) for a code without this structure", i, j, mb, nb, Z, r);
                    return LDPC_E_UNSUPPORTED;
                }
                ++cnt[(size_t)j];
            }
        }
        std::sort(touched.begin(), touched.end());
        for (int32_t j : touched) {
            if (cnt[(size_t)j] != Z) {
                set_error("ldpc_qc_create: block (%d, %d) of the %d x %d base at Z = %d holds %d ones, a shifted identity holds %d; use "
                          "ldpc_lqmsa_create (LQMSA, any layering) for a code without this structure", i, j, mb, nb, Z, cnt[(size_t)j], Z);
                return LDPC_E_UNSUPPORTED;
            }
            h->col.push_back(j);
            h->shift.push_back(sh[(size_t)j]);
            cnt[(size_t)j] = 0;
            sh[(size_t)j] = -1;
        }
        h->row_ptr.push_back((int32_t)h->col.size());
    }
    return LDPC_OK;
}

}  // namespace

int qc_create(Code* code, int32_t Z, Qc** out) {
    if (Z < 1 || code->m % Z != 0 || code->n % Z != 0) {
        set_error("ldpc_qc_create: the lifting size Z = %d must be >= 1 and divide m = %d and n = %d", Z, code->m, code->n);
        return LDPC_E_ARG;
    }
    Qc* h = new Qc();
    h->code = code;
    h->Z = Z;
    h->mb = code->m / Z;
    h->nb = code->n / Z;
    int rc = detect(code, Z, h);
    if (rc != LDPC_OK) {
        delete h;
        return rc;
    }
    int32_t dmin = code->m ? INT32_MAX : 0;
    for (int32_t i = 0; i < h->mb; ++i) {
        const int32_t d = h->row_ptr[(size_t)i + 1] - h->row_ptr[(size_t)i];
        dmin = std::min(dmin, d);
        h->dc_max = std::max(h->dc_max, d);
    }
    const int64_t need = lqmsa_lds_bytes(code->m, code->n, code->E, h->dc_max);
    rc = fx_check_degrees("ldpc_qc_create", "block row", dmin, code->max_dv, LQMSA_MAX_DV);
    if (rc == LDPC_OK && need > LQMSA_LDS_BYTES) {
        set_error("ldpc_qc_create: one frame of this code (m = %d, n = %d, largest block-row degree %d) needs %lld bytes of LDS, above one CU's %lld; "
                  "use LDPC_ALG_LMSA (layered min-sum on the streaming kernels) for it",
                  code->m, code->n, h->dc_max, (long long)need, (long long)LQMSA_LDS_BYTES);
        rc = LDPC_E_UNSUPPORTED;
    }
    if (rc != LDPC_OK) {
        delete h;
        return rc;
    }
    hipError_t e = hipSetDevice(code->device);
    h->lds_bytes = need;
    h->row_bytes = lqmsa_row_bytes(h->dc_max);
    const int64_t fit = LQMSA_LDS_BYTES / need;
    h->nw = fx_waves(qc_waves(fit, Z), "LDPC_QC_NW");  // (the wave table of the rate tool reaches every wave count with it too)
    h->frames_per_cu = fx_frames_per_cu(fit, h->nw);
    if (const char* env = std::getenv("LDPC_QC_PACK_GRID")) h->pack_grid = std::max(std::atoi(env), 0);  // the tests put chosen frames into one wave's slots
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, code->device);
    if (e == hipSuccess) e = fx_allow_lds(kernel_of<float>(h->nw, h->row_bytes == 8), kernel_of<double>(h->nw, h->row_bytes == 8), need);
    if (e != hipSuccess) {
        set_error("ldpc_qc_create: device setup failed: %s", hipGetErrorString(e));
        qc_destroy(h);
        return LDPC_E_HIP;
    }
    h->num_cu = prop.multiProcessorCount;
    rc = h->ctl.reserve(64);
    if (rc == LDPC_OK) {
        std::vector<int32_t> natural((size_t)h->mb);
        std::iota(natural.begin(), natural.end(), 0);
        rc = install(h, natural);
    }
    if (rc != LDPC_OK) {
        qc_destroy(h);
        return rc;
    }
    *out = h;
    return LDPC_OK;
}

void qc_destroy(Qc* h) {
    if (!h) return;
    for (DevBuf* b : {&h->tab, &h->ctl}) b->release();
    h->sim.release();
    delete h;
}

int qc_set_fixed_point(Qc* h, int bits, int frac_bits, double scale, int offset) {
    return h->fx.set("ldpc_qc_set_fixed_point", bits, frac_bits, scale, offset);
}

void qc_get_fixed_point(const Qc* h, int* bits, int* frac_bits, double* scale, int* offset) { h->fx.get(bits, frac_bits, scale, offset); }

void qc_get_base(const Qc* h, int32_t* mb, int32_t* nb, int32_t* Z, int32_t* shifts) {
    *mb = h->mb;
    *nb = h->nb;
    *Z = h->Z;
    if (!shifts) return;
    std::fill(shifts, shifts + (size_t)h->mb * (size_t)h->nb, -1);
    for (int32_t i = 0; i < h->mb; ++i)
        for (int32_t k = h->row_ptr[(size_t)i]; k < h->row_ptr[(size_t)i + 1]; ++k) shifts[(size_t)i * (size_t)h->nb + (size_t)h->col[(size_t)k]] = h->shift[(size_t)k];
}

int qc_set_order(Qc* h, const int32_t* order, int32_t mb) {
    std::vector<int32_t> next((size_t)h->mb);
    if (!order) {
        std::iota(next.begin(), next.end(), 0);
        return install(h, next);
    }
    if (mb != h->mb) {
        set_error("ldpc_qc_set_order: %d entries for a base of %d block rows", mb, h->mb);
        return LDPC_E_ARG;
    }
    std::vector<char> seen((size_t)h->mb, 0);
    for (int32_t l = 0; l < mb; ++l) {
        if (order[l] < 0 || order[l] >= mb || seen[(size_t)order[l]]) {
            set_error("ldpc_qc_set_order: entry %d (%d): the order is a permutation of 0 .. %d", l, order[l], mb - 1);
            return LDPC_E_ARG;
        }
        seen[(size_t)order[l]] = 1;
        next[(size_t)l] = order[l];
    }
    return install(h, next);
}

void qc_get_order(const Qc* h, int32_t* mb, int32_t* order) {
    *mb = h->mb;
    if (order) std::copy(h->order.begin(), h->order.end(), order);
}

// workgroups of k_qc_pack one CU holds at P frames per wave
static int pack_groups_per_cu(const Qc* h, int P) { return (int)std::min<int64_t>(LQMSA_LDS_BYTES / (P * qc_pack_stride(h->lds_bytes, h->Z)), 32); }

int qcpack_set(Qc* h, int32_t P) {
    const int64_t stride = qc_pack_stride(h->lds_bytes, h->Z);
    if (P == 0) P = qc_pack(h->Z, h->lds_bytes);
    if (P < 1 || (P >= 2 && ((int64_t)P * h->Z > 64 || P * stride > LQMSA_LDS_BYTES))) {
        set_error("ldpc_qcpack_set: %d frames per wave at Z = %d with %lld bytes from frame to frame (%lld per frame): the frames of a wave take "
                  "P Z <= 64 lanes and P times those bytes <= %lld of LDS; 0 takes the rule's %d, 1 is one frame per workgroup",
                  P, h->Z, (long long)stride, (long long)h->lds_bytes, (long long)LQMSA_LDS_BYTES, qc_pack(h->Z, h->lds_bytes));
        return LDPC_E_ARG;
    }
    if (P >= 2 && P * stride > 64 * 1024) {
        LDPC_HIP_TRY(hipSetDevice(h->code->device));
        LDPC_HIP_TRY(fx_allow_lds(pack_kernel_of<float>(h->row_bytes == 8), pack_kernel_of<double>(h->row_bytes == 8), LQMSA_LDS_BYTES));
    }
    h->pack = P;
    return LDPC_OK;
}

void qcpack_get(const Qc* h, int32_t* frames_per_wave, int32_t* rule_pick) {
    *frames_per_wave = h->pack;
    *rule_pick = qc_pack(h->Z, h->lds_bytes);
}

void qc_info(const Qc* h, double* out4) {
    out4[0] = (double)h->lds_bytes;
    if (h->pack >= 2) {
        const int per_cu = pack_groups_per_cu(h, h->pack);
        out4[1] = 1;
        out4[2] = (double)h->pack * per_cu;
        out4[3] = (double)h->num_cu * per_cu;
        return;
    }
    out4[1] = h->nw;
    out4[2] = h->frames_per_cu;
    out4[3] = (double)h->num_cu * h->frames_per_cu;
}

int qc_decode(Qc* h, int dtype, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat, uint32_t* bits,
              int32_t* iters, int16_t* soft, hipStream_t st) {
    LDPC_TRY(fx_check_decode("ldpc_qc_decode", dtype, flags, B));
    const Code* c = h->code;
    LDPC_HIP_TRY(hipSetDevice(c->device));
    if (B == 0) return LDPC_OK;
    QcArgs a;
    fx_fill_args(a, c, h->fx, h->row_bytes, h->ctl.p, priors, y0, B, max_iter, flags, xhat, bits, iters, soft);
    a.Z = h->Z;
    a.mb = h->mb;
    a.tab = (const int32_t*)h->tab.p;
    LDPC_HIP_TRY(hipMemsetAsync(a.dispenser, 0, 4, st));
    if (h->pack >= 2) {
        QcPackArgs pa;
        pa.a = a;
        pa.P = h->pack;
        pa.stride = (int32_t)qc_pack_stride(h->lds_bytes, h->Z);
        int64_t groups = std::min<int64_t>((B + pa.P - 1) / pa.P, (int64_t)h->num_cu * pack_groups_per_cu(h, pa.P));
        if (h->pack_grid > 0) groups = std::min<int64_t>(groups, h->pack_grid);
        const void* kern = dtype == DT_F64 ? pack_kernel_of<double>(h->row_bytes == 8) : pack_kernel_of<float>(h->row_bytes == 8);
        void* args[] = {(void*)&pa};
        LDPC_HIP_TRY(hipLaunchKernel(kern, dim3((unsigned)groups), dim3(64u), args, (size_t)pa.P * (size_t)pa.stride, st));
        return LDPC_OK;
    }
    const unsigned groups = (unsigned)std::min<int64_t>(B, (int64_t)h->num_cu * h->frames_per_cu);
    const void* kern = dtype == DT_F64 ? kernel_of<double>(h->nw, h->row_bytes == 8) : kernel_of<float>(h->nw, h->row_bytes == 8);
    void* args[] = {(void*)&a};
    LDPC_HIP_TRY(hipLaunchKernel(kern, dim3(groups), dim3(64u * (unsigned)h->nw), args, (size_t)h->lds_bytes, st));
    return LDPC_OK;
}

int qc_simulate(Qc* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st) {
    return fx_simulate("ldpc_qc_simulate", h->code, h->sim, fx_lds_sim_cap(h->code->n), channel, param, codeword, seed, stream_id, frame0, B,
                       hist_bins, counters, st, [&](const void* pri, const uint8_t* y, int64_t nb, uint32_t* bits, int32_t* iters) {
                           return qc_decode(h, DT_F32, pri, y, nb, max_iter, flags, nullptr, bits, iters, nullptr, st);
                       });
}

}  // namespace ldpc

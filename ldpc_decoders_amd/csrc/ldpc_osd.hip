// Ordered-statistics post-processing (BP+OSD) of the LLR decoders: the frames belief propagation leaves without a codeword are decoded
// again from its soft output, one wave per frame.  No upstream counterpart: it adds to BPA.decode (src/bpa.py:17-63).
//
// The contract is in include/ldpc_hip.h (ldpc_osd_*) and DESIGN.md section 17; tests/osd_oracle.py states it in numpy.  Here:
//   1. k_osd_list, one wave per frame: the hard decisions of `post` as packed words, every check evaluated from row_ptr / edge_var; a frame
//      whose syndrome is zero is finished (pick = -1, cost = -1), the others are appended to a device list through an atomic counter.
//   2. k_osd_solve, one wave (= one workgroup) per listed frame, the whole frame in a slab of dynamic LDS:
//        sort:       the 64-bit keys (bits of fp32 |post| << 32 | variable), padded with all-ones to a power of two, through a bitonic
//                    network; position p holds variable pi[p], pos[] is the inverse.  The key slots then take the weights (double)|prior| in
//                    sorted order (slot p is read and rewritten by the same lane).
//        matrix:     H with column pos[v], word-major M[w][row], lane l owning rows l, l + 64, ...: the layout and the pivot / Gauss-Jordan
//                    loop of k_bec_ml_solve (ldpc_bec_ml.hip), without a right-hand side.  rowof[p] = pivot row of position p or -1 (free).
//                    The column scan stops once the rank reaches rank(H) (computed once by osd_create): the other rows are zero by then.
//        candidates: candidate 0 = h on the free positions, each pivot position the XOR of its row's free bits.  Candidate t flips free
//                    position f = flist[t - 1] and with it every pivot position whose row has a 1 in column f.  Lane l scores candidate
//                    64 r + l in round r, walking p = 0 .. n-1 in order so that the fp64 sum has the contract's order.
//        pick:       a wave-wide minimum on (cost, t); the winner's word goes to the packed output in variable order.
#include <climits>
#include <new>

#include "ldpc_osd.hpp"
#include "ldpc_sim.hpp"

namespace ldpc {

struct Osd {
    Code* code = nullptr;
    int num_cu = 0, rank = 0, groups = 0;  // rank(H); workgroups of k_osd_solve = num_cu * (slabs that fit one CU's LDS)
    int64_t slab = 0;                      // bytes of LDS one frame takes
    DevBuf ctr, list, marg, bits, pri, y, xh, iters, pick;
};

namespace {

constexpr int64_t CHUNK = (int64_t)1 << 17;  // frames per pass: bounds the workspace (and what ldpc_decode_soft takes)

__device__ __forceinline__ float osd_rho(float a) { return a != a ? 0.0f : fabsf(a); }
__device__ __forceinline__ float osd_rho(double a) { return a != a ? 0.0f : (float)fabs(a); }
__device__ __forceinline__ double osd_weight(float a) { return a != a ? 0.0 : (double)fabsf(a); }
__device__ __forceinline__ double osd_weight(double a) { return a != a ? 0.0 : fabs(a); }

// hard decisions of post as packed words, syndrome of every check; four frames per workgroup, one wave each, W words of LDS per wave
template <typename T>
__global__ __launch_bounds__(256) void k_osd_list(const T* __restrict__ post, uint32_t* __restrict__ out, int32_t* __restrict__ pick,
                                                  double* __restrict__ cost, int64_t B, int n, int m, const int32_t* __restrict__ row_ptr,
                                                  const int32_t* __restrict__ edge_var, int32_t* __restrict__ list, int32_t* __restrict__ ctr) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = (n + 31) >> 5;
    uint32_t* hb = lds + wave * W;
    const int64_t f = (int64_t)blockIdx.x * 4 + wave;
    const bool active = f < B;  // wave-uniform
    for (int v0 = 0; v0 < n; v0 += 64) {
        const int v = v0 + lane;
        const bool bit = active && v < n && post[f * n + v] < (T)0;
        const uint64_t bal = __ballot(bit);
        if (lane == 0) {
            hb[v0 >> 5] = (uint32_t)bal;
            if ((v0 >> 5) + 1 < W) hb[(v0 >> 5) + 1] = (uint32_t)(bal >> 32);
        }
    }
    __syncthreads();
    bool bad = false;
    if (active)
        for (int c = lane; c < m; c += 64) {
            uint32_t par = 0;
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
                const int v = edge_var[e];
                par ^= hb[v >> 5] >> (v & 31);
            }
            bad |= (par & 1u) != 0;
        }
    const bool fails = __ballot(bad) != 0;
    if (!active) return;
    for (int w = lane; w < W; w += 64) out[f * W + w] = hb[w];
    if (lane == 0) {
        if (fails) {
            list[atomicAdd(&ctr[0], 1)] = (int32_t)f;
        } else {
            pick[f] = -1;
            if (cost) cost[f] = -1.0;
        }
    }
}

// one wave per listed frame; osd_lds_words(m, n) words of dynamic LDS
template <typename T>
__global__ __launch_bounds__(64) void k_osd_solve(const T* __restrict__ post, const T* __restrict__ prior, uint32_t* __restrict__ out,
                                                  int32_t* __restrict__ pick, double* __restrict__ cost, int n, int m, int rank_h,
                                                  const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var,
                                                  const int32_t* __restrict__ list, const int32_t* __restrict__ count, int order, int depth) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1;
    const int S = (n + 31) >> 5, RP = (m + 63) & ~63, KC = RP >> 6;
    const int NP = (int)osd_sort_keys(n);
    uint64_t* keys = (uint64_t*)lds;       // [NP] sort keys ...
    double* ws = (double*)lds;             // ... then [n] weights (double)|prior| in sorted order
    uint32_t* M = lds + 2 * NP;            // [S][RP]: bit p of M[p >> 5][i] = H[row i][variable pi[p]]
    int32_t* pi = (int32_t*)(M + S * RP);  // [n] variable at sorted position p
    int32_t* pos = pi + n;                 // [n] position of variable v
    int32_t* rowof = pos + n;              // [n] pivot row of position p, -1: free
    int32_t* flist = rowof + n;            // [n] the free positions, ascending
    uint32_t* pmask = (uint32_t*)(flist + n);  // [S] pivot positions
    uint32_t* hpos = pmask + S;                // [S] h in position order
    uint32_t* gpos = hpos + S;                 // [S] g in position order
    uint32_t* x0 = gpos + S;                   // [S] candidate 0
    uint32_t* d0 = x0 + S;                     // [S] candidate 0 XOR g: where it pays its weight
    const int cnt = *count;
    for (int it = blockIdx.x; it < cnt; it += gridDim.x) {
        const int f = list[it];
        const T* pf = post + (int64_t)f * n;
        const T* qf = prior + (int64_t)f * n;
        uint32_t* of = out + (int64_t)f * S;
        __syncthreads();  // the previous frame's reads of the slab are done
        for (int i = lane; i < NP; i += 64)
            keys[i] = i < n ? ((uint64_t)__float_as_uint(osd_rho(pf[i])) << 32) | (uint32_t)i : ~0ull;
        __syncthreads();
        // bitonic network, ascending
        for (int k = 2; k <= NP; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = lane; i < (NP >> 1); i += 64) {
                    const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
                    const uint64_t ka = keys[a], kb = keys[b];
                    if ((ka > kb) == ((a & k) == 0)) {
                        keys[a] = kb;
                        keys[b] = ka;
                    }
                }
                __syncthreads();
            }
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int p = p0 + lane;
            bool hb = false, gb = false;
            if (p < n) {
                const int v = (int)(uint32_t)keys[p];
                const T a = qf[v];
                pi[p] = v;
                pos[v] = p;
                rowof[p] = -1;
                ws[p] = osd_weight(a);  // the slot of keys[p]: read above, by this lane
                hb = pf[v] < (T)0;
                gb = a < (T)0;
            }
            const uint64_t bh = __ballot(hb), bg = __ballot(gb);
            if (lane == 0) {
                const int w = p0 >> 5;
                hpos[w] = (uint32_t)bh;
                gpos[w] = (uint32_t)bg;
                pmask[w] = 0;
                if (w + 1 < S) {
                    hpos[w + 1] = (uint32_t)(bh >> 32);
                    gpos[w + 1] = (uint32_t)(bg >> 32);
                    pmask[w + 1] = 0;
                }
            }
        }
        __syncthreads();
        for (int c0 = 0; c0 < RP; c0 += 64) {
            const int i = c0 + lane;
            for (int w = 0; w < S; ++w) M[w * RP + i] = 0;
            if (i < m)
                for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
                    const int col = pos[edge_var[e]];
                    M[(col >> 5) * RP + i] ^= 1u << (col & 31);
                }
        }
        __syncthreads();
        // Gauss-Jordan over the positions in ascending order: the loop of k_bec_ml_solve
        uint64_t used = 0;  // bit k: row 64 k + lane is a pivot row
        int rank = 0;
        for (int j = 0; j < n && rank < rank_h; ++j) {
            const int w = j >> 5;
            const uint32_t bit = 1u << (j & 31);
            const uint32_t* Mw = M + w * RP;
            int piv = -1;
            for (int k = 0; k < KC; ++k) {
                const bool hit = (Mw[k * 64 + lane] & bit) && !((used >> k) & 1);
                const uint64_t bal = __ballot(hit);
                if (bal) {
                    piv = k * 64 + __builtin_ctzll(bal);
                    break;
                }
            }
            if (piv < 0) continue;  // free position
            ++rank;
            if (lane == (piv & 63)) used |= 1ull << (piv >> 6);
            if (lane == 0) {
                pmask[w] |= bit;
                rowof[j] = piv;
            }
            for (int k = 0; k < KC; ++k) {
                const int i = k * 64 + lane;
                if (i != piv && (Mw[i] & bit))
                    for (int ww = w; ww < S; ++ww) M[ww * RP + i] ^= M[ww * RP + piv];
            }
            __syncthreads();
        }
        __syncthreads();
        // candidate 0 and the list of free positions
        int nf = 0;
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int p = p0 + lane;
            bool xb = false, fr = false;
            if (p < n) {
                const int r = rowof[p];
                fr = r < 0;
                if (fr) {
                    xb = ((hpos[p >> 5] >> (p & 31)) & 1u) != 0;
                } else {  // a pivot row is 0 in every other pivot position
                    uint32_t acc = 0;
                    for (int ww = 0; ww < S; ++ww) acc ^= M[ww * RP + r] & hpos[ww] & ~pmask[ww];
                    xb = (__popc(acc) & 1) != 0;
                }
            }
            const uint64_t bx = __ballot(xb), bf = __ballot(fr);
            if (fr) flist[nf + __popcll(bf & below)] = p;
            nf += __popcll(bf);
            if (lane == 0) {
                const int w = p0 >> 5;
                x0[w] = (uint32_t)bx;
                d0[w] = (uint32_t)bx ^ gpos[w];
                if (w + 1 < S) {
                    x0[w + 1] = (uint32_t)(bx >> 32);
                    d0[w + 1] = (uint32_t)(bx >> 32) ^ gpos[w + 1];
                }
            }
        }
        __syncthreads();
        // score: candidate t in lane t & 63 of round t >> 6
        const int last = order == 1 ? (depth < nf ? depth : nf) : 0;
        double best = 0.0;
        int bt = INT_MAX;
        for (int t0 = 0; t0 <= last; t0 += 64) {
            const int t = t0 + lane;
            const bool act = t <= last;
            const int fp = act && t > 0 ? flist[t - 1] : -1;
            const uint32_t* Mf = M + (fp >= 0 ? (fp >> 5) * RP : 0);
            const uint32_t fbit = fp >= 0 ? 1u << (fp & 31) : 0u;
            double c = 0.0;
            for (int p = 0; p < n; ++p) {
                const bool diff = ((d0[p >> 5] >> (p & 31)) & 1u) != 0;
                const int r = rowof[p];
                const bool flip = p == fp || (r >= 0 && (Mf[r] & fbit) != 0);
                if (diff != flip) c += ws[p];
            }
            if (act && (bt == INT_MAX || c < best)) {  // t grows from round to round: equal cost keeps the smaller t
                best = c;
                bt = t;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const double oc = __shfl_xor(best, d);
            const int ot = __shfl_xor(bt, d);
            if (ot != INT_MAX && (bt == INT_MAX || oc < best || (oc == best && ot < bt))) {
                best = oc;
                bt = ot;
            }
        }
        // the winner in variable order
        const int fw = bt > 0 ? flist[bt - 1] : -1;
        const uint32_t* Mf = M + (fw >= 0 ? (fw >> 5) * RP : 0);
        const uint32_t fbit = fw >= 0 ? 1u << (fw & 31) : 0u;
        for (int v0 = 0; v0 < n; v0 += 64) {
            const int v = v0 + lane;
            bool xb = false;
            if (v < n) {
                const int p = pos[v], r = rowof[p];
                const bool flip = p == fw || (r >= 0 && (Mf[r] & fbit) != 0);
                xb = (((x0[p >> 5] >> (p & 31)) & 1u) != 0) != flip;
            }
            const uint64_t bx = __ballot(xb);
            if (lane == 0) {
                of[v0 >> 5] = (uint32_t)bx;
                if ((v0 >> 5) + 1 < S) of[(v0 >> 5) + 1] = (uint32_t)(bx >> 32);
            }
        }
        if (lane == 0) {
            pick[f] = bt;
            if (cost) cost[f] = best;
        }
    }
}

// a frame that left at the iteration-0 check of y0 never swept (its marginals are 0): its soft output is its priors
template <typename T>
__global__ __launch_bounds__(256) void k_osd_unswept(T* __restrict__ marg, const T* __restrict__ prior, const int32_t* __restrict__ iters, int64_t B,
                                                     int n) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= B * n) return;
    if (iters[t / n] == 0) marg[t] = prior[t];
}

__global__ __launch_bounds__(256) void k_osd_unpack(const uint32_t* __restrict__ bits, int64_t B, int n, uint8_t* __restrict__ xhat) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= B * n) return;
    const int64_t f = t / n;
    const int v = (int)(t - f * n);
    xhat[t] = (uint8_t)((bits[f * ((n + 31) / 32) + (v >> 5)] >> (v & 31)) & 1u);
}

// rank of H over GF(2) on the host (once per handle): rows as 64-bit words
int host_rank(const Code* c) {
    const size_t words = ((size_t)c->n + 63) / 64;
    std::vector<uint64_t> a((size_t)c->m * words, 0);
    for (int32_t i = 0; i < c->m; ++i)
        for (int32_t e = c->row_ptr[i]; e < c->row_ptr[i + 1]; ++e) a[i * words + (c->edge_var[e] >> 6)] ^= 1ull << (c->edge_var[e] & 63);
    int rank = 0;
    for (int32_t j = 0; j < c->n && rank < c->m; ++j) {
        const size_t w = (size_t)j >> 6;
        const uint64_t bit = 1ull << (j & 63);
        int32_t piv = -1;
        for (int32_t i = rank; i < c->m; ++i)
            if (a[i * words + w] & bit) {
                piv = i;
                break;
            }
        if (piv < 0) continue;
        for (size_t ww = 0; ww < words; ++ww) std::swap(a[piv * words + ww], a[rank * words + ww]);
        for (int32_t i = rank + 1; i < c->m; ++i)
            if (a[i * words + w] & bit)
                for (size_t ww = w; ww < words; ++ww) a[i * words + ww] ^= a[rank * words + ww];
        ++rank;
    }
    return rank;
}

int check_order(const char* who, int32_t order, int64_t depth) {
    if ((order != 0 && order != 1) || depth < 0) {
        set_error("%s: order must be 0 or 1 and depth >= 0 (got order=%d, depth=%lld)", who, order, (long long)depth);
        return LDPC_E_ARG;
    }
    return LDPC_OK;
}

// what may run in front of the post-processor: an fp32 / fp64 LLR decoder of the handle's own code
int check_decoder(const char* who, const Osd* h, const Decoder* d) {
    if (!d || d->code != h->code) {
        set_error("%s: the decoder must be one of the code this handle was created for", who);
        return LDPC_E_ARG;
    }
    if (!alg_row(d->alg).llr || d->dtype == DT_F16) {
        set_error("%s: needs the soft output of an fp32 or fp64 LDPC_ALG_MSA / SPA / NMSA / QMSA / LMSA decoder (the erasure decoder has none, fp16 "
                  "storage keeps none in the decoder's type)", who);
        return LDPC_E_UNSUPPORTED;
    }
    return LDPC_OK;
}

template <typename T>
int solve_t(Osd* h, const T* post, const T* prior, int64_t B, int order, int depth, uint32_t* out_bits, int32_t* pick, double* cost, hipStream_t st) {
    const Code* c = h->code;
    const int W = (c->n + 31) / 32;
    int32_t* ctr = (int32_t*)h->ctr.p;
    for (int64_t b0 = 0; b0 < B; b0 += CHUNK) {
        const int64_t nb = B - b0 < CHUNK ? B - b0 : CHUNK;
        const T* po = post + b0 * c->n;
        const T* pr = prior + b0 * c->n;
        uint32_t* ob = out_bits + b0 * W;
        int32_t* pk = pick + b0;
        double* co = cost ? cost + b0 : nullptr;
        LDPC_HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(k_osd_list<T>, dim3((unsigned)((nb + 3) / 4)), dim3(256), (size_t)(4 * W * 4), st, po, ob, pk, co, nb, c->n, c->m,
                           c->d_row_ptr, c->d_edge_var, (int32_t*)h->list.p, ctr);
        LDPC_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_osd_solve<T>, dim3((unsigned)h->groups), dim3(64), (size_t)h->slab, st, po, pr, ob, pk, co, c->n, c->m, h->rank,
                           c->d_row_ptr, c->d_edge_var, (const int32_t*)h->list.p, (const int32_t*)ctr, order, depth);
        LDPC_HIP_TRY(hipGetLastError());
    }
    return LDPC_OK;
}

}  // namespace

int osd_create(Code* code, Osd** out) {
    if (!code || !out) {
        set_error("ldpc_osd_create: bad arguments");
        return LDPC_E_ARG;
    }
    const int64_t need = osd_lds_words(code->m, code->n) * 4;
    if (need > OSD_LDS_BYTES || ((int64_t)code->m + 63) / 64 * 64 > OSD_MAX_ROWS) {
        set_error("ldpc_osd_create: m x n = %d x %d: one frame (sort keys, matrix, permutations) needs %lld bytes of LDS, above the limit of "
                  "one CU's 160 KiB (at most %d checks)", code->m, code->n, (long long)need, OSD_MAX_ROWS);
        return LDPC_E_ARG;
    }
    LDPC_HIP_TRY(hipSetDevice(code->device));
    Osd* h = new Osd();
    h->code = code;
    h->slab = need;
    h->rank = host_rank(code);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, code->device) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_osd_solve<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OSD_LDS_BYTES) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_osd_solve<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OSD_LDS_BYTES) != hipSuccess) {
        set_error("ldpc_osd_create: device query / LDS attribute failed");
        osd_destroy(h);
        return LDPC_E_HIP;
    }
    h->num_cu = prop.multiProcessorCount;
    h->groups = h->num_cu * (int)(OSD_LDS_BYTES / need);
    int rc = h->ctr.reserve(sizeof(int32_t));
    if (rc == LDPC_OK) rc = h->list.reserve((size_t)CHUNK * sizeof(int32_t));
    if (rc != LDPC_OK) {
        osd_destroy(h);
        return rc;
    }
    *out = h;
    return LDPC_OK;
}

void osd_destroy(Osd* h) {
    if (!h) return;
    for (DevBuf* b : {&h->ctr, &h->list, &h->marg, &h->bits, &h->pri, &h->y, &h->xh, &h->iters, &h->pick}) b->release();
    delete h;
}

int osd_solve(Osd* h, int dtype, const void* post, const void* prior, int64_t B, int32_t order, int64_t depth, uint32_t* out_bits, int32_t* pick,
              double* cost, hipStream_t st) {
    LDPC_TRY(check_order("ldpc_osd_solve", order, depth));
    if (dtype != DT_F32 && dtype != DT_F64) {
        set_error("ldpc_osd_solve: post and prior are LDPC_DTYPE_F32 or LDPC_DTYPE_F64");
        return LDPC_E_UNSUPPORTED;
    }
    LDPC_HIP_TRY(hipSetDevice(h->code->device));
    const int dep = (int)(depth < h->code->n ? depth : h->code->n);  // there are at most n free positions
    return dtype == DT_F64 ? solve_t(h, (const double*)post, (const double*)prior, B, order, dep, out_bits, pick, cost, st)
                           : solve_t(h, (const float*)post, (const float*)prior, B, order, dep, out_bits, pick, cost, st);
}

// BP + solve of one chunk (<= 2^17 frames); the words land in h->bits, BP's bytes in xhat (overwritten by the caller's unpack, if any)
static int bp_solve(Osd* h, ldpc_decoder_t dec, const void* priors, const uint8_t* y0, int64_t nb, int32_t max_iter, uint32_t flags, int32_t order,
                    int64_t depth, uint8_t* xhat, int32_t* iters, int32_t* pick, hipStream_t st) {
    const Decoder* d = (const Decoder*)dec;
    const size_t n = (size_t)h->code->n, W = (n + 31) / 32, esz = d->dtype == DT_F64 ? 8 : 4;
    LDPC_TRY(h->marg.reserve((size_t)nb * n * esz));
    LDPC_TRY(h->bits.reserve((size_t)nb * W * 4));
    LDPC_TRY(ldpc_decode_soft(dec, priors, y0, nb, max_iter, flags, xhat, iters, h->marg.p, st));
    if (y0) {
        const unsigned blocks = (unsigned)((nb * (int64_t)n + 255) / 256);
        if (d->dtype == DT_F64)
            hipLaunchKernelGGL(k_osd_unswept<double>, dim3(blocks), dim3(256), 0, st, (double*)h->marg.p, (const double*)priors, iters, nb, (int)n);
        else
            hipLaunchKernelGGL(k_osd_unswept<float>, dim3(blocks), dim3(256), 0, st, (float*)h->marg.p, (const float*)priors, iters, nb, (int)n);
        LDPC_HIP_TRY(hipGetLastError());
    }
    return osd_solve(h, d->dtype, h->marg.p, priors, nb, order, depth, (uint32_t*)h->bits.p, pick, nullptr, st);
}

int osd_decode(Osd* h, ldpc_decoder_t dec, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags, int32_t order,
               int64_t depth, uint8_t* xhat, int32_t* iters, int32_t* pick, hipStream_t st) {
    LDPC_TRY(check_order("ldpc_osd_decode", order, depth));
    LDPC_TRY(check_decoder("ldpc_osd_decode", h, (const Decoder*)dec));
    const size_t n = (size_t)h->code->n, esz = ((const Decoder*)dec)->dtype == DT_F64 ? 8 : 4;
    LDPC_HIP_TRY(hipSetDevice(h->code->device));
    for (int64_t b0 = 0; b0 < B; b0 += CHUNK) {
        const int64_t nb = B - b0 < CHUNK ? B - b0 : CHUNK;
        LDPC_TRY(bp_solve(h, dec, (const char*)priors + (size_t)b0 * n * esz, y0 ? y0 + (size_t)b0 * n : nullptr, nb, max_iter, flags, order, depth,
                          xhat + (size_t)b0 * n, iters + b0, pick + b0, st));
        hipLaunchKernelGGL(k_osd_unpack, dim3((unsigned)((nb * (int64_t)n + 255) / 256)), dim3(256), 0, st, (const uint32_t*)h->bits.p, nb, (int)n,
                           xhat + (size_t)b0 * n);
        LDPC_HIP_TRY(hipGetLastError());
    }
    return LDPC_OK;
}

int osd_simulate(Osd* h, ldpc_decoder_t dec, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                 int32_t max_iter, uint32_t flags, int32_t order, int64_t depth, int32_t hist_bins, int64_t* counters, hipStream_t st) {
    LDPC_TRY(check_order("ldpc_osd_simulate", order, depth));
    LDPC_TRY(check_decoder("ldpc_osd_simulate", h, (const Decoder*)dec));
    if (LDPC_FLAG_PRIOR_GRID_OF(flags) >= 0) {
        set_error("ldpc_osd_simulate: no prior grid (the exact-in-fp32 mode belongs to ldpc_simulate)");
        return LDPC_E_UNSUPPORTED;
    }
    const bool bsc = channel == CH_BSC;
    const int dtype = ((const Decoder*)dec)->dtype;
    const size_t n = (size_t)h->code->n, esz = dtype == DT_F64 ? 8 : 4;
    return sim_passes(
        SimCall{"ldpc_osd_simulate", h->code, codeword, frame0, B, hist_bins, counters, st},
        bsc || channel == CH_BIAWGN ? nullptr : "LDPC_CH_BIAWGN or LDPC_CH_BSC (over the erasure channel ldpc_bec_ml_* is the ML decoder)", CHUNK,
        [&](int64_t cap) -> int {
            LDPC_TRY(h->pri.reserve((size_t)cap * n * esz));
            if (bsc) LDPC_TRY(h->y.reserve((size_t)cap * n));
            LDPC_TRY(h->xh.reserve((size_t)cap * n));
            LDPC_TRY(h->iters.reserve((size_t)cap * sizeof(int32_t)));
            return h->pick.reserve((size_t)cap * sizeof(int32_t));
        },
        [&](uint64_t first, int64_t nb, const uint32_t*& bits, const int32_t*& iters) -> int {
            uint8_t* y = bsc ? (uint8_t*)h->y.p : nullptr;
            LDPC_TRY(channel_generate(channel, dtype, param, codeword, seed, stream_id, first, nb, (int32_t)n, h->pri.p, y, st));
            LDPC_TRY(bp_solve(h, dec, h->pri.p, y, nb, max_iter, flags, order, depth, (uint8_t*)h->xh.p, (int32_t*)h->iters.p, (int32_t*)h->pick.p, st));
            bits = (const uint32_t*)h->bits.p;  // (reserved by bp_solve)
            iters = (const int32_t*)h->iters.p;
            return LDPC_OK;
        });
}

}  // namespace ldpc

// Maximum-likelihood decoding over the BEC for codes without a code book: GF(2) elimination of the residual system, one wave per frame.
//
// The reference's rule (src/bec.py:21-36 with math_utils.arg_max_rand, src/math_utils.py:72-74): every codeword that agrees with the
// unerased symbols is equally likely, one is picked uniformly.  Here:
//   1. peel: the erasure decoder (LDPC_ALG_BEC, max_iter <= 0) runs to its stopping-set exit; what stays erased is the residual set R.
//   2. k_bec_ml_list copies the peeled words to the output and lists the frames with R != {} (device-side compaction: a frame that
//      peeling finished costs one read of its mask).
//   3. k_bec_ml_solve, one wave (= one workgroup) per listed frame, the frame's system in a slab of LDS:
//        columns = R in ascending variable order, rows = the checks that touch R in H's row order, right-hand side = XOR of each row's
//        known bits, stored word-major (M[w][row]) so that the 64 lanes, one row each, read consecutive dwords.
//        Gauss-Jordan: column by column, the pivot is the first row not yet used that has a 1 there (a ballot per 64 rows); every other
//        row with a 1 takes the pivot row's words from the pivot's word onwards.  The reduced form does not depend on the pivot choice.
//        Free columns (no pivot), ascending: free column number t takes bit t of Philox4x32-10 keyed by (seed, stream id, global frame
//        index), block 0xC0000000 + (t >> 7), word (t >> 5) & 3, bit t & 31.  A pivot column takes its row's right-hand side XOR the
//        row's free bits.  nullity = |R| - rank, -1 when a row without pivot keeps a right-hand side of 1 (the sent word was no codeword).
//   Two slab sizes: 32 KiB (5 waves per CU; every frame below about eps = 0.5 of the n = 1200 codes) and the whole 160 KiB of a CU for
//   the frames the first pass set aside.  bec_ml_create refuses a code whose worst case (every bit erased) does not fit 160 KiB.
#include <climits>
#include <new>

#include "ldpc_bec_ml.hpp"
#include "ldpc_sim.hpp"
#include "ldpc_rng.hpp"

namespace ldpc {

struct BecMl {
    Code* code = nullptr;
    ldpc_decoder_t peel = nullptr;  // the erasure decoder whose stopping-set exit leaves the residual set
    int num_cu = 0;
    DevBuf bits, era, iters, y, ctr, list, ovf, nul;
};

namespace {

constexpr uint32_t FREE_BLOCK0 = 0xC0000000u;
constexpr int64_t SMALL_LDS_BYTES = 32 * 1024;
constexpr int SMALL_PER_CU = (int)(BEC_ML_LDS_BYTES / SMALL_LDS_BYTES);
constexpr int64_t CHUNK = (int64_t)1 << 17;  // frames per pass: bounds the workspace

__device__ __forceinline__ uint32_t pick4(const Philox4& r, int i) {
    return i == 0 ? r.w[0] : i == 1 ? r.w[1] : i == 2 ? r.w[2] : r.w[3];
}

// copy the peeled words to the output, list the frames that keep erasures; the others are finished with nullity 0
__global__ __launch_bounds__(256) void k_bec_ml_list(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ era, uint32_t* out,
                                                     int32_t* __restrict__ nul, int64_t B, int W, int32_t* __restrict__ list,
                                                     int32_t* __restrict__ ctr) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= B) return;
    uint32_t any = 0;
    for (int w = 0; w < W; ++w) {
        any |= era[f * W + w];
        out[f * W + w] = bits[f * W + w];
    }
    if (any)
        list[atomicAdd(&ctr[0], 1)] = (int32_t)f;
    else
        nul[f] = 0;
}

// one wave per listed frame; `slab` bytes of dynamic LDS.  Frames whose system does not fit go to ovf_list (NULL on the 160 KiB pass,
// where bec_ml_create guarantees the fit)
__global__ __launch_bounds__(64) void k_bec_ml_solve(uint32_t* __restrict__ out, const uint32_t* __restrict__ era, int32_t* __restrict__ nul,
                                                     int n, int m, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ edge_var,
                                                     const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                     int32_t* __restrict__ ovf_list, int32_t* __restrict__ ovf_count, int64_t slab,
                                                     uint64_t seed, uint32_t stream, uint64_t frame0) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1;
    const int W = (n + 31) >> 5;
    uint32_t* emask = lds;        // [W] residual set
    uint32_t* dec = lds + W;      // [W] peeled decisions
    int32_t* pref = (int32_t*)(lds + 2 * W);  // [W] erased bits before word w = column of its first erased bit
    const int cnt = *count;
    for (int it = blockIdx.x; it < cnt; it += gridDim.x) {
        const int f = list[it];
        const uint32_t* ef = era + (int64_t)f * W;
        uint32_t* of = out + (int64_t)f * W;
        __syncthreads();  // the previous frame's reads of the slab are done
        int nc = 0;
        for (int w0 = 0; w0 < W; w0 += 64) {
            const int w = w0 + lane;
            const uint32_t e = w < W ? ef[w] : 0u;
            const int c = __popc(e);
            int s = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(s, d);
                if (lane >= d) s += t;
            }
            if (w < W) {
                emask[w] = e;
                dec[w] = of[w];
                pref[w] = nc + s - c;
            }
            nc += __shfl(s, 63);
        }
        __syncthreads();
        // rows: the checks that touch R, counted first (the slab must hold them)
        int rows = 0;
        for (int c0 = 0; c0 < m; c0 += 64) {
            const int c = c0 + lane;
            bool touch = false;
            if (c < m)
                for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
                    const int v = edge_var[e];
                    touch |= ((emask[v >> 5] >> (v & 31)) & 1u) != 0;
                }
            rows += __popcll(__ballot(touch));
        }
        const int S = (nc + 32) >> 5, RP = (rows + 63) & ~63, KC = RP >> 6;
        if (RP > BEC_ML_MAX_ROWS || bec_ml_lds_words(n, nc, rows) * 4 > slab) {
            if (lane == 0) {
                if (ovf_list)
                    ovf_list[atomicAdd(ovf_count, 1)] = f;
                else
                    nul[f] = INT_MIN;  // unreachable: bec_ml_create checked the worst case against the 160 KiB slab
            }
            continue;
        }
        uint32_t* pmask = lds + 3 * W;              // [S] pivot columns
        uint32_t* xfree = pmask + S;                // [S] values of the free columns
        uint32_t* xpiv = xfree + S;                 // [S] values of the pivot columns
        uint32_t* M = xpiv + S;                     // [S][RP]: bit j of M[j >> 5][i] = H[row i][column j]; column nc = right-hand side
        for (int w = lane; w < S; w += 64) pmask[w] = xfree[w] = xpiv[w] = 0;
        for (int i = rows + lane; i < RP; i += 64)
            for (int w = 0; w < S; ++w) M[w * RP + i] = 0;
        int r0 = 0;
        for (int c0 = 0; c0 < m; c0 += 64) {
            const int c = c0 + lane;
            bool touch = false;
            int e0 = 0, e1 = 0;
            if (c < m) {
                e0 = row_ptr[c];
                e1 = row_ptr[c + 1];
                for (int e = e0; e < e1; ++e) {
                    const int v = edge_var[e];
                    touch |= ((emask[v >> 5] >> (v & 31)) & 1u) != 0;
                }
            }
            const uint64_t bal = __ballot(touch);
            if (touch) {
                const int i = r0 + __popcll(bal & below);
                for (int w = 0; w < S; ++w) M[w * RP + i] = 0;
                uint32_t rhs = 0;
                for (int e = e0; e < e1; ++e) {
                    const int v = edge_var[e];
                    const uint32_t em = emask[v >> 5], b = 1u << (v & 31);
                    if (em & b) {
                        const int col = pref[v >> 5] + __popc(em & (b - 1));
                        M[(col >> 5) * RP + i] ^= 1u << (col & 31);
                    } else {
                        rhs ^= (dec[v >> 5] >> (v & 31)) & 1u;
                    }
                }
                M[(nc >> 5) * RP + i] ^= rhs << (nc & 31);
            }
            r0 += __popcll(bal);
        }
        __syncthreads();
        // Gauss-Jordan over the columns in ascending order
        uint64_t used = 0;  // bit k: row 64 k + lane is a pivot row
        int rank = 0;
        for (int j = 0; j < nc; ++j) {
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
            if (piv < 0) continue;  // free column
            ++rank;
            if (lane == (piv & 63)) used |= 1ull << (piv >> 6);
            if (lane == 0) pmask[w] |= bit;
            for (int k = 0; k < KC; ++k) {
                const int i = k * 64 + lane;
                if (i != piv && (Mw[i] & bit))
                    for (int ww = w; ww < S; ++ww) M[ww * RP + i] ^= M[ww * RP + piv];
            }
            __syncthreads();
        }
        // free columns: number t in ascending order takes bit t of the frame's tie-break stream
        const uint64_t gframe = frame0 + (uint64_t)f;
        int tbase = 0;
        for (int j0 = 0; j0 < nc; j0 += 64) {
            const int j = j0 + lane;
            const bool fr = j < nc && !((pmask[j >> 5] >> (j & 31)) & 1u);
            const uint64_t bal = __ballot(fr);
            bool val = false;
            if (fr) {
                const int t = tbase + __popcll(bal & below);
                const Philox4 r = philox_word_block(seed, stream, gframe, FREE_BLOCK0 + (uint32_t)(t >> 7));
                val = ((pick4(r, (t >> 5) & 3) >> (t & 31)) & 1u) != 0;
            }
            const uint64_t vb = __ballot(val);
            if (lane == 0) {
                xfree[j0 >> 5] = (uint32_t)vb;
                if ((j0 >> 5) + 1 < S) xfree[(j0 >> 5) + 1] = (uint32_t)(vb >> 32);
            }
            tbase += __popcll(bal);
        }
        __syncthreads();
        // pivot columns: right-hand side XOR the row's free bits (a pivot row is 0 in every other pivot column); a row without pivot
        // is 0 in every column, a right-hand side of 1 there makes the system inconsistent
        bool bad = false;
        for (int k = 0; k < KC; ++k) {
            const int i = k * 64 + lane;
            const uint32_t rhs = (M[(nc >> 5) * RP + i] >> (nc & 31)) & 1u;
            if ((used >> k) & 1) {
                uint32_t acc = 0;
                int pc = -1;
                for (int ww = 0; ww < S; ++ww) {
                    const uint32_t row = M[ww * RP + i];
                    acc ^= row & xfree[ww];
                    const uint32_t pv = row & pmask[ww];  // exactly one pivot column: this row's
                    if (pv) pc = ww * 32 + __builtin_ctz(pv);
                }
                if (((__popc(acc) & 1) ^ rhs) && pc >= 0) atomicOr(&xpiv[pc >> 5], 1u << (pc & 31));
            } else if (rhs) {
                bad = true;
            }
        }
        const bool inconsistent = __ballot(bad) != 0;
        __syncthreads();
        for (int w = lane; w < W; w += 64) {
            uint32_t e = emask[w], x = dec[w];
            int col = pref[w];
            while (e) {
                const int b = __builtin_ctz(e);
                e &= e - 1;
                if (((xfree[col >> 5] | xpiv[col >> 5]) >> (col & 31)) & 1u) x |= 1u << b;
                ++col;
            }
            of[w] = x;
        }
        if (lane == 0) nul[f] = inconsistent ? -1 : nc - rank;
    }
}

__global__ __launch_bounds__(256) void k_bec_ml_unpack(const uint32_t* __restrict__ bits, int64_t B, int n, uint8_t* __restrict__ xhat) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= B * n) return;
    const int64_t f = t / n;
    const int v = (int)(t - f * n);
    xhat[t] = (uint8_t)((bits[f * ((n + 31) / 32) + (v >> 5)] >> (v & 31)) & 1u);
}

}  // namespace

int bec_ml_create(Code* code, BecMl** out) {
    if (!code || !out) {
        set_error("ldpc_bec_ml_create: bad arguments");
        return LDPC_E_ARG;
    }
    const int64_t need = bec_ml_lds_words(code->n, code->n, code->m) * 4;
    if (need > BEC_ML_LDS_BYTES || ((int64_t)code->m + 63) / 64 * 64 > BEC_ML_MAX_ROWS) {
        set_error("ldpc_bec_ml_create: m x n = %d x %d: the worst-case system (every bit erased) needs %lld bytes of LDS, above the limit "
                  "of one CU's 160 KiB (m * n <= 1310720 bits; at most %d checks)", code->m, code->n, (long long)need, BEC_ML_MAX_ROWS);
        return LDPC_E_ARG;
    }
    LDPC_HIP_TRY(hipSetDevice(code->device));
    BecMl* h = new BecMl();
    h->code = code;
    hipDeviceProp_t prop;
    int rc = LDPC_OK;
    if (hipGetDeviceProperties(&prop, code->device) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_bec_ml_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BEC_ML_LDS_BYTES) != hipSuccess) {
        set_error("ldpc_bec_ml_create: device query / LDS attribute failed");
        rc = LDPC_E_HIP;
    }
    if (rc == LDPC_OK) {
        h->num_cu = prop.multiProcessorCount;
        rc = ldpc_decoder_create((ldpc_code_t)code, LDPC_ALG_BEC, LDPC_DTYPE_F32, LDPC_BACKEND_AUTO, &h->peel);
    }
    if (rc != LDPC_OK) {
        bec_ml_destroy(h);
        return rc;
    }
    *out = h;
    return LDPC_OK;
}

void bec_ml_destroy(BecMl* h) {
    if (!h) return;
    if (h->peel) ldpc_decoder_destroy(h->peel);
    for (DevBuf* b : {&h->bits, &h->era, &h->iters, &h->y, &h->ctr, &h->list, &h->ovf, &h->nul}) b->release();
    delete h;
}

int bec_ml_solve(BecMl* h, const uint32_t* bits, const uint32_t* erased, int64_t B, uint64_t seed, uint64_t stream_id, uint64_t frame0,
                 uint32_t* out_bits, int32_t* nullity, hipStream_t st) {
    const Code* c = h->code;
    const int W = (c->n + 31) / 32;
    LDPC_HIP_TRY(hipSetDevice(c->device));
    LDPC_TRY(h->ctr.reserve(2 * sizeof(int32_t)));
    LDPC_TRY(h->list.reserve((size_t)CHUNK * sizeof(int32_t)));
    LDPC_TRY(h->ovf.reserve((size_t)CHUNK * sizeof(int32_t)));
    int32_t* ctr = (int32_t*)h->ctr.p;
    for (int64_t b0 = 0; b0 < B; b0 += CHUNK) {
        const int64_t nb = B - b0 < CHUNK ? B - b0 : CHUNK;
        const uint32_t* bi = bits + b0 * W;
        const uint32_t* er = erased + b0 * W;
        uint32_t* ob = out_bits + b0 * W;
        int32_t* nu = nullity + b0;
        LDPC_HIP_TRY(hipMemsetAsync(ctr, 0, 2 * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_bec_ml_list, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, bi, er, ob, nu, nb, W, (int32_t*)h->list.p, ctr);
        LDPC_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_bec_ml_solve, dim3((unsigned)(h->num_cu * SMALL_PER_CU)), dim3(64), (size_t)SMALL_LDS_BYTES, st, ob, er, nu, c->n,
                           c->m, c->d_row_ptr, c->d_edge_var, (const int32_t*)h->list.p, ctr, (int32_t*)h->ovf.p, ctr + 1, SMALL_LDS_BYTES, seed,
                           (uint32_t)stream_id, frame0 + (uint64_t)b0);
        LDPC_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_bec_ml_solve, dim3((unsigned)h->num_cu), dim3(64), (size_t)BEC_ML_LDS_BYTES, st, ob, er, nu, c->n, c->m,
                           c->d_row_ptr, c->d_edge_var, (const int32_t*)h->ovf.p, ctr + 1, (int32_t*)nullptr, (int32_t*)nullptr,
                           BEC_ML_LDS_BYTES, seed, (uint32_t)stream_id, frame0 + (uint64_t)b0);
        LDPC_HIP_TRY(hipGetLastError());
    }
    return LDPC_OK;
}

// peel + solve of one chunk of symbols; the resolved words land in h->bits
static int peel_solve(BecMl* h, const uint8_t* y, int64_t nb, uint64_t seed, uint64_t stream_id, uint64_t frame0, int32_t* nullity,
                      hipStream_t st) {
    const size_t W = ((size_t)h->code->n + 31) / 32;
    LDPC_TRY(h->bits.reserve((size_t)nb * W * 4));
    LDPC_TRY(h->era.reserve((size_t)nb * W * 4));
    LDPC_TRY(h->iters.reserve((size_t)nb * 4));
    uint32_t* bits = (uint32_t*)h->bits.p;
    LDPC_TRY(ldpc_decode_bits(h->peel, nullptr, y, nb, 0, 0, bits, (uint32_t*)h->era.p, (int32_t*)h->iters.p, st));
    return bec_ml_solve(h, bits, (const uint32_t*)h->era.p, nb, seed, stream_id, frame0, bits, nullity, st);
}

int bec_ml_decode(BecMl* h, const uint8_t* y, int64_t B, uint64_t seed, uint64_t stream_id, uint64_t frame0, uint8_t* xhat, int32_t* nullity,
                  hipStream_t st) {
    const int n = h->code->n;
    LDPC_HIP_TRY(hipSetDevice(h->code->device));
    for (int64_t b0 = 0; b0 < B; b0 += CHUNK) {
        const int64_t nb = B - b0 < CHUNK ? B - b0 : CHUNK;
        LDPC_TRY(peel_solve(h, y + b0 * n, nb, seed, stream_id, frame0 + (uint64_t)b0, nullity + b0, st));
        hipLaunchKernelGGL(k_bec_ml_unpack, dim3((unsigned)((nb * n + 255) / 256)), dim3(256), 0, st, (const uint32_t*)h->bits.p, nb, n,
                           xhat + b0 * n);
        LDPC_HIP_TRY(hipGetLastError());
    }
    return LDPC_OK;
}

int bec_ml_simulate(BecMl* h, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int64_t* counters,
                    hipStream_t st) {
    const int n = h->code->n;
    return sim_passes(
        SimCall{"ldpc_bec_ml_simulate", h->code, codeword, frame0, B, 0, counters, st}, nullptr, CHUNK,
        [&](int64_t cap) -> int {
            LDPC_TRY(h->y.reserve((size_t)cap * n));
            return h->nul.reserve((size_t)cap * sizeof(int32_t));
        },
        [&](uint64_t first, int64_t nb, const uint32_t*& bits, const int32_t*&) -> int {
            LDPC_TRY(channel_generate(CH_BEC, DT_F32, param, codeword, seed, stream_id, first, nb, n, nullptr, (uint8_t*)h->y.p, st));
            LDPC_TRY(peel_solve(h, (const uint8_t*)h->y.p, nb, seed, stream_id, first, (int32_t*)h->nul.p, st));
            bits = (const uint32_t*)h->bits.p;  // (reserved by peel_solve)
            return LDPC_OK;
        });
}

}  // namespace ldpc

// Host entry points of the ordered-statistics post-processor of the LLR decoders (ldpc_osd.hip), called by ldpc_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldpc_common.hpp"

namespace ldpc {

struct Osd;
// number of sort keys: the power of two >= n (the bitonic network of k_osd_solve; the padding keys are all-ones and sort last)
__host__ __device__ inline int64_t osd_sort_keys(int32_t n) {
    int64_t np = 1;
    while (np < n) np <<= 1;
    return np;
}
// LDS words one frame takes: the 64-bit sort keys [2 NP] (later the weights in sorted order), the matrix [S x RP] (S = words of n bits,
// RP = rows rounded up to 64), pi / its inverse / the pivot row of every position / the list of free positions [4 n], and five bit masks
// in position order [5 S]: pivot positions, h, g, candidate 0, candidate 0 XOR g.  The same formula: ldpc_decoders_amd/bpa.py osd_lds_bytes
__host__ __device__ inline int64_t osd_lds_words(int32_t m, int32_t n) {
    const int64_t S = (n + 31) / 32, RP = ((int64_t)m + 63) / 64 * 64;
    return 2 * osd_sort_keys(n) + S * RP + 4 * (int64_t)n + 5 * S;
}
constexpr int64_t OSD_LDS_BYTES = 160 * 1024;  // one CU's LDS
constexpr int32_t OSD_MAX_ROWS = 4096;         // 64 row chunks of 64: one uint64 "pivot row" mask per lane

int osd_create(Code* code, Osd** out);
void osd_destroy(Osd* h);
int osd_solve(Osd* h, int dtype, const void* post, const void* prior, int64_t B, int32_t order, int64_t depth, uint32_t* out_bits, int32_t* pick,
              double* cost, hipStream_t st);
int osd_decode(Osd* h, ldpc_decoder_t dec, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags, int32_t order,
               int64_t depth, uint8_t* xhat, int32_t* iters, int32_t* pick, hipStream_t st);
int osd_simulate(Osd* h, ldpc_decoder_t dec, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                 int32_t max_iter, uint32_t flags, int32_t order, int64_t depth, int32_t hist_bins, int64_t* counters, hipStream_t st);

}  // namespace ldpc

// Host entry points of the layered fixed-point min-sum decoder (ldpc_lqmsa.hip), called by ldpc_api.hip, and its LDS size rule.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldpc_common.hpp"

namespace ldpc {

struct Lqmsa;
constexpr int64_t LQMSA_LDS_BYTES = 160 * 1024;  // one CU's LDS
constexpr int LQMSA_MAX_DV = 255;                // |marginal| <= V (1 + dv) <= 127 * 256 < 2^15
// bytes of one check's row of int8 messages: 8 up to degree 8 (one 64-bit LDS access), the degree rounded up to whole dwords above it.
// A row never shares a dword with another row, so the lane that owns the check may write it in any width.
__host__ __device__ inline int32_t lqmsa_row_bytes(int32_t dc_max) { return dc_max <= 8 ? 8 : (dc_max + 3) / 4 * 4; }
// LDS bytes one frame takes: the int16 marginals [n] (rounded up to 8 bytes), one message row per check, 16 bytes of frame state (frame
// index, the two syndrome flags, spare).  E is not used by this layout (E <= m * row bytes).  The same formula: include/ldpc_hip.h,
// ldpc_decoders_amd/layered.py lqmsa_lds_bytes.  A frame fits iff the result is <= LQMSA_LDS_BYTES.
__host__ __device__ inline int64_t lqmsa_lds_bytes(int32_t m, int32_t n, int64_t E, int32_t dc_max) {
    (void)E;
    return (2 * (int64_t)n + 7) / 8 * 8 + (int64_t)m * lqmsa_row_bytes(dc_max) + 16;
}
// waves per frame from the frames one CU's LDS holds: the CU is to hold as many waves as it can, up to 32 -- min(frames, 32 / W) * W --
// with the smallest W in {1, 2, 4, 8} that reaches the most: 1 from 32 frames on, 2 from 16, 4 from 8, 8 below
__host__ __device__ inline int lqmsa_waves(int64_t frames_per_cu) {
    int best = 1;
    int64_t most = 0;
    for (int w = 1; w <= 8; w *= 2) {
        const int64_t waves = (frames_per_cu < 32 / w ? frames_per_cu : 32 / w) * w;
        if (waves > most) {
            most = waves;
            best = w;
        }
    }
    return best;
}

int lqmsa_create(Code* code, Lqmsa** out);
void lqmsa_destroy(Lqmsa* h);
int lqmsa_set_fixed_point(Lqmsa* h, int bits, int frac_bits, double scale, int offset);
void lqmsa_get_fixed_point(const Lqmsa* h, int* bits, int* frac_bits, double* scale, int* offset);
int lqmsa_set_layers(Lqmsa* h, const int32_t* layer_of_check, int32_t m);
void lqmsa_get_layers(const Lqmsa* h, int32_t* nlayers, int32_t* layer_of_check);
int lqmsa_decode(Lqmsa* h, int dtype, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat,
                 uint32_t* bits, int32_t* iters, int16_t* soft, hipStream_t st);
int lqmsa_simulate(Lqmsa* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                   uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st);
void lqmsa_info(const Lqmsa* h, double* out4);

}  // namespace ldpc

// Host entry points of the quasi-cyclic layered fixed-point min-sum decoder (ldpc_qc.hip), called by ldpc_api.hip, and its wave rule.  The
// LDS layout and size rule are LQMSA's (ldpc_lqmsa.hpp: lqmsa_lds_bytes with dc_max = the largest block-row degree, LQMSA_LDS_BYTES).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldpc_common.hpp"
#include "ldpc_lqmsa.hpp"

namespace ldpc {

struct Qc;
// waves per frame: lqmsa_waves(frames one CU's LDS holds), capped at the smallest of 1, 2, 4, 8 that is >= ceil(Z / 64) -- a block row has
// ceil(Z / 64) wave passes, more waves than passes would idle.  The same rule: include/ldpc_hip.h, ldpc_decoders_amd/qc.py qc_waves.
__host__ __device__ inline int qc_waves(int64_t frames_per_cu, int32_t Z) {
    const int64_t passes = ((int64_t)Z + 63) / 64;
    int cap = 1;
    while (cap < 8 && cap < passes) cap *= 2;
    const int w = lqmsa_waves(frames_per_cu);
    return w < cap ? w : cap;
}

int qc_create(Code* code, int32_t Z, Qc** out);
void qc_destroy(Qc* h);
int qc_set_fixed_point(Qc* h, int bits, int frac_bits, double scale, int offset);
void qc_get_fixed_point(const Qc* h, int* bits, int* frac_bits, double* scale, int* offset);
void qc_get_base(const Qc* h, int32_t* mb, int32_t* nb, int32_t* Z, int32_t* shifts);
int qc_set_order(Qc* h, const int32_t* order, int32_t mb);
void qc_get_order(const Qc* h, int32_t* mb, int32_t* order);
int qc_decode(Qc* h, int dtype, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat, uint32_t* bits,
              int32_t* iters, int16_t* soft, hipStream_t st);
int qc_simulate(Qc* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st);
void qc_info(const Qc* h, double* out4);

}  // namespace ldpc

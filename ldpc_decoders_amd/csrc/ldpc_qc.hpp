// Host entry points of the quasi-cyclic layered fixed-point min-sum decoder (ldpc_qc.hip), called by ldpc_api.hip, its wave rule and the
// rule for several frames per wave.  The LDS layout and size rule are LQMSA's (ldpc_lqmsa.hpp: lqmsa_lds_bytes with dc_max = the largest
// block-row degree, LQMSA_LDS_BYTES).
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

// Several frames per wave (k_qc_pack, Z <= 32).  Bytes from one frame slot's image to the next: at least the frame's bytes, a multiple of
// 16, and congruent to 2 Z rounded up to 16 modulo the 128 bytes of the 32 banks -- Z neighbouring int16 marginals span at most that many
// bytes, so the slots that share a 32-lane group read one block column on disjoint banks.  The same function: include/ldpc_hip.h,
// ldpc_decoders_amd/qc.py qc_pack_stride.
__host__ __device__ inline int64_t qc_pack_stride(int64_t lds_bytes_per_frame, int32_t Z) {
    const int64_t want = (2 * (int64_t)Z + 15) / 16 * 16 % 128, s = (lds_bytes_per_frame + 15) / 16 * 16;
    return s + (want - s % 128 + 128) % 128;
}
// frames per wave: 1 above Z = 32, else as many as the lanes and one CU's LDS take.  The same rule: include/ldpc_hip.h,
// ldpc_decoders_amd/qc.py qc_pack.
__host__ __device__ inline int qc_pack(int32_t Z, int64_t lds_bytes_per_frame) {
    if (Z > 32) return 1;
    const int64_t lanes = 64 / Z, fit = LQMSA_LDS_BYTES / qc_pack_stride(lds_bytes_per_frame, Z);
    const int64_t p = lanes < fit ? lanes : fit;
    return p < 1 ? 1 : (int)p;
}

int qc_create(Code* code, int32_t Z, Qc** out);
int qcpack_set(Qc* h, int32_t frames_per_wave);
void qcpack_get(const Qc* h, int32_t* frames_per_wave, int32_t* rule_pick);
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

// Host entry points of the ML erasure decoder for codes without a code book (ldpc_bec_ml.hip), called by ldpc_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldpc_common.hpp"

namespace ldpc {

struct BecMl;
// LDS words one frame's system takes: residual mask, decisions, column prefix counts [3 W], pivot-column mask, free values, pivot
// values [3 S], the matrix [S x RP] (S = words of nc + 1 bits: the columns and the right-hand side; RP = rows rounded up to 64)
__host__ __device__ inline int64_t bec_ml_lds_words(int32_t n, int32_t nc, int32_t rows) {
    const int64_t W = (n + 31) / 32, S = (nc + 32) / 32, RP = ((int64_t)rows + 63) / 64 * 64;
    return 3 * W + 3 * S + S * RP;
}
constexpr int64_t BEC_ML_LDS_BYTES = 160 * 1024;  // one CU's LDS: the worst case (every bit erased, every check a row) must fit
constexpr int32_t BEC_ML_MAX_ROWS = 4096;         // 64 row chunks of 64: one uint64 "pivot row" mask per lane

int bec_ml_create(Code* code, BecMl** out);
void bec_ml_destroy(BecMl* h);
int bec_ml_solve(BecMl* h, const uint32_t* bits, const uint32_t* erased, int64_t B, uint64_t seed, uint64_t stream_id, uint64_t frame0,
                 uint32_t* out_bits, int32_t* nullity, hipStream_t st);
int bec_ml_decode(BecMl* h, const uint8_t* y, int64_t B, uint64_t seed, uint64_t stream_id, uint64_t frame0, uint8_t* xhat, int32_t* nullity,
                  hipStream_t st);
int bec_ml_simulate(BecMl* h, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int64_t* counters,
                    hipStream_t st);

}  // namespace ldpc

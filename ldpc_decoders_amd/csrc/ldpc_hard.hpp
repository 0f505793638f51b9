// Host entry points of the bit-sliced Gallager-B hard-decision decoder (ldpc_hard.hip), called by ldpc_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldpc_common.hpp"

namespace ldpc {

struct Hard;
constexpr int HARD_SLAB = 32;                    // frames per slab == bits of a plane word
constexpr int HARD_SUPER = 64 * HARD_SLAB;       // frames per supertile of the streaming kernels: one wave lane per slab
constexpr int HARD_MAX_DV = 63;                  // the vertical counters of the variable pass have six planes
constexpr int64_t HARD_LDS_BYTES = 160 * 1024;   // one CU's LDS
// LDS bytes one slab takes in the LDS-resident kernel: y [n], x [n], v2c [E] (variable-major), the check parities [m], 4 words of slab
// state (slab index, live mask, unsatisfied mask, spare).  The same formula: include/ldpc_hip.h, ldpc_decoders_amd/hard.py hard_lds_bytes
__host__ __device__ inline int64_t hard_lds_bytes(int32_t m, int32_t n, int64_t E) { return 4 * (2 * (int64_t)n + E + (int64_t)m + 4); }

int hard_create(Code* code, int backend, Hard** out);
void hard_destroy(Hard* h);
int hard_set_threshold(Hard* h, int t);
int hard_get_threshold(const Hard* h);
int hard_decode(Hard* h, const uint8_t* y, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat, uint32_t* bits, int32_t* iters, hipStream_t st);
int hard_simulate(Hard* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                  uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st);
int hard_last_backend(const Hard* h);
void hard_info(const Hard* h, double* out4);

}  // namespace ldpc

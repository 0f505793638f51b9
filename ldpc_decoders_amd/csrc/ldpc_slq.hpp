// Host entry points of the streaming layered fixed-point min-sum decoder (ldpc_slq.hip), called by ldpc_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldpc_common.hpp"

namespace ldpc {

struct Slq;
constexpr int SLQ_MAX_DV = 255;  // |marginal| <= V (1 + dv) <= 127 * 256 < 2^15
// Bytes of integer state one frame keeps in HBM: n int16 marginals and E int8 messages (the decision planes add n / 8).
__host__ __device__ inline int64_t slq_state_bytes(int32_t n, int64_t E) { return 2 * (int64_t)n + E; }
// The workspace bound: the state tiles of a chunk of frames plus a repack target of the same size stay within it (a decode of more frames
// runs chunk after chunk); ldpc_slq_simulate's fp32 prior chunk has a bound of its own, a third of it.  LDPC_SLQ_WORKSPACE_MB overrides.
constexpr int64_t SLQ_WORKSPACE_BYTES = (int64_t)24 << 30;

int slq_create(Code* code, Slq** out);
void slq_destroy(Slq* h);
int slq_set_fixed_point(Slq* h, int bits, int frac_bits, double scale, int offset);
void slq_get_fixed_point(const Slq* h, int* bits, int* frac_bits, double* scale, int* offset);
int slq_set_layers(Slq* h, const int32_t* layer_of_check, int32_t m);
void slq_get_layers(const Slq* h, int32_t* nlayers, int32_t* layer_of_check);
int slq_decode(Slq* h, int dtype, const void* priors, const uint8_t* y0, int64_t B, int32_t max_iter, uint32_t flags, uint8_t* xhat, uint32_t* bits,
               int32_t* iters, int16_t* soft, hipStream_t st);
int slq_simulate(Slq* h, int channel, double param, int codeword, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, int32_t max_iter,
                 uint32_t flags, int32_t hist_bins, int64_t* counters, hipStream_t st);
void slq_info(const Slq* h, double* out4);
void slq_profile(Slq* h, int enable, double* ms3, int64_t* launches3, int reset);
void slq_last_stats(const Slq* h, int32_t* out3);

}  // namespace ldpc

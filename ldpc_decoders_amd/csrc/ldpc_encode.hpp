// Host entry points of the GF(2) encoder and the channel of a given word per frame (ldpc_encode.hip), called by ldpc_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldpc {

struct Encoder;
// P: [k, r] bytes in {0,1}, row-major (c[par_pos] = u . P mod 2); info_pos [k] / par_pos [r] partition 0 .. n-1
int encoder_create(int device, int32_t n, int32_t k, int32_t r, const int32_t* info_pos, const int32_t* par_pos, const uint8_t* P, Encoder** out);
void encoder_destroy(Encoder* e);
// out = {nt, cgroups, kgroups, chunks of k_info}: what encode / encode_random launch with
int encoder_info(const Encoder* e, int32_t out[4]);
int encode(Encoder* e, const uint8_t* u, int64_t B, uint8_t* sent, hipStream_t st);
int encode_random(Encoder* e, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B, uint8_t* sent, hipStream_t st);
int channel_sent(int channel, int dtype, double param, const uint8_t* sent, uint64_t seed, uint64_t stream_id, uint64_t frame0, int64_t B,
                 int32_t n, void* priors, uint8_t* y, hipStream_t st);

}  // namespace ldpc

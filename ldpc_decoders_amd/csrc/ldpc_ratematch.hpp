// Punctured and shortened transmission (csrc/ldpc_ratematch.hip): the channel of a transmission pattern and the tally that leaves the
// shortened bits out.  The contract is the ldpc_channel_pattern / ldpc_count_errors_pattern block of include/ldpc_hip.h.
#pragma once
#include "ldpc_common.hpp"

namespace ldpc {

enum { KIND_SENT = 0, KIND_PUNCTURED = 1, KIND_SHORTENED = 2 };  // one byte per variable (ratematch.Pattern.kind)

int channel_pattern(int channel, int dtype, double param, const uint8_t* sent, int codeword, const uint8_t* kind, double short_llr, uint64_t seed,
                    uint64_t stream_id, uint64_t frame0, int64_t B, int32_t n, void* priors, uint8_t* y, hipStream_t st);
int count_errors_pattern(const uint8_t* xhat, const uint8_t* sent, int codeword, const uint8_t* kind, const int32_t* iters, int64_t B, int32_t n,
                         int32_t hist_bins, int64_t* counters, hipStream_t st);

}  // namespace ldpc

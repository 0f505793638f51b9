// Incremental-redundancy HARQ (csrc/ldpc_harq.hip): the transmission that adds its copies into a per-frame soft buffer, the syndrome of
// the decisions as the acknowledgement, and the tally that knows when a frame leaves.  The contract is the ldpc_harq_* block of
// include/ldpc_hip.h.
#pragma once
#include "ldpc_common.hpp"

namespace ldpc {

constexpr int HARQ_MAX_TX = 16;  // transmissions of one schedule (ratematch.Harq)

int harq_transmit(int channel, int dtype, double param, const uint8_t* sent, int64_t sent_rows, int codeword, const uint8_t* kind, const uint8_t* cnt,
                  const uint8_t* first, double short_llr, uint64_t seed, uint64_t stream_id, uint64_t frame0, const int64_t* src, const int64_t* orig,
                  const void* soft_old, int64_t old_rows, int64_t B_out, int32_t n, void* soft_new, hipStream_t st);
int harq_syndrome(const Code* c, const uint8_t* xhat, int64_t B, uint8_t* fail, hipStream_t st);
int harq_tally(const uint8_t* xhat, const uint8_t* sent, int64_t sent_rows, int codeword, const uint8_t* kind, const int32_t* iters, const uint8_t* fail,
               const int64_t* orig, int64_t B, int32_t n, int32_t hist_bins, int32_t t, int32_t T, int64_t tx_bits, int64_t* counters, hipStream_t st);

}  // namespace ldpc

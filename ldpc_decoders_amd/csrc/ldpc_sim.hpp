// The Monte-Carlo pass of the handle families, stated once: ldpc_hard_simulate, ldpc_osd_simulate, ldpc_bec_ml_simulate and, through fx_simulate
// (ldpc_layered_fx.hpp), ldpc_lqmsa_simulate, ldpc_qc_simulate and ldpc_slq_simulate.  Refuse a word that is no codeword, clamp the pass, reserve the
// staging, then per pass generate -> decode -> count.  A family supplies its pass-size rule, its channel refusal, where its staging lives and
// "generate and decode these frames into packed words".  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "ldpc_common.hpp"

namespace ldpc {

// does a check have odd degree: Code::odd_check, filled by code_build_host, read by the second refusal of sim_passes
inline bool has_odd_check(const std::vector<int32_t>& row_ptr) {
    bool odd = false;
    for (size_t c = 0; c + 1 < row_ptr.size(); ++c) odd |= ((row_ptr[c + 1] - row_ptr[c]) & 1) != 0;
    return odd;
}

// staging of a *_simulate whose decoder reads fp32 priors and / or the received bytes and writes packed words
struct SimStage {
    DevBuf pri, y, bits, iters;
    int reserve(int64_t cap, size_t n, bool with_pri, bool with_y) {
        if (with_pri) LDPC_TRY(pri.reserve((size_t)cap * n * sizeof(float)));
        if (with_y) LDPC_TRY(y.reserve((size_t)cap * n));
        LDPC_TRY(bits.reserve((size_t)cap * ((n + 31) / 32) * 4));
        return iters.reserve((size_t)cap * sizeof(int32_t));
    }
    void release() {
        for (DevBuf* b : {&pri, &y, &bits, &iters}) b->release();
    }
};

// LDPC_SIM_PASS_FRAMES=<positive integer>, read at every call: lowers the pass of every family to that many frames (never raises it; anything
// else is ignored).  Every decode takes a ragged last pass, so every value is valid; the tests reach the second and the last pass with it.
inline int64_t sim_pass_frames(int64_t rule) {
    if (const char* env = std::getenv("LDPC_SIM_PASS_FRAMES")) {
        char* end = nullptr;
        const long long v = std::strtoll(env, &end, 10);
        if (end != env && *end == '\0' && v > 0) rule = std::min<int64_t>(rule, v);
    }
    return rule;
}

// what every *_simulate is called with
struct SimCall {
    const char* entry;  // the entry point the messages name
    const Code* code;
    int codeword;
    uint64_t frame0;
    int64_t B;
    int32_t hist_bins;
    int64_t* counters;
    hipStream_t st;
};

// Frames [frame0, frame0 + B) in passes of at most `cap` frames (the family's rule; at most 2^17, at most B, at most LDPC_SIM_PASS_FRAMES).
// channel_refusal: the family's sentence where the channel is not one of its own, else null.  reserve(cap) sizes the staging for the largest
// pass; pass(first_frame, nb, bits, iters) generates and decodes nb frames and says where their packed words and iteration counts (or null) lie.
template <class Reserve, class Pass>
int sim_passes(const SimCall& c, const char* channel_refusal, int64_t cap, Reserve&& reserve, Pass&& pass) {
    if (channel_refusal) {
        set_error("%s: %s", c.entry, channel_refusal);
        return LDPC_E_ARG;
    }
    if (c.codeword != 0 && c.codeword != 1) {
        set_error("%s: codeword must be 0 or 1", c.entry);
        return LDPC_E_ARG;
    }
    if (c.codeword == 1 && c.code->odd_check) {
        set_error("%s: codeword 1: the all-ones word is no codeword of this code (a check has odd degree)", c.entry);
        return LDPC_E_ARG;
    }
    cap = std::min(std::min<int64_t>(sim_pass_frames(cap), (int64_t)1 << 17), std::max<int64_t>(c.B, 1));
    LDPC_HIP_TRY(hipSetDevice(c.code->device));
    LDPC_TRY(reserve(cap));
    for (int64_t b0 = 0; b0 < c.B; b0 += cap) {
        const int64_t nb = std::min(cap, c.B - b0);
        const uint32_t* bits = nullptr;
        const int32_t* iters = nullptr;
        LDPC_TRY(pass(c.frame0 + (uint64_t)b0, nb, bits, iters));
        LDPC_TRY(count_errors_bits(bits, nullptr, nullptr, c.codeword, iters, nb, c.code->n, c.hist_bins, c.counters, c.st));
    }
    return LDPC_OK;
}

}  // namespace ldpc

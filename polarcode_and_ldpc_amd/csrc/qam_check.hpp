// The parameter checks of the Gray-mapped QAM modem and of its block-fading channel (qam.hip), device-free: plain
// C++, no HIP.  The definitions: include/polarldpc.h at pl_qam_check and at pl_qam_fading_check.
#pragma once
#include <stdint.h>

#include <string>

namespace pl {

struct QamStatus {
    int code = 0;  // PL_OK or PL_EINVAL
    std::string msg;
};

constexpr int64_t kQamMaxE = (int64_t)1 << 30;

// The conditions in the header's order: m in {2, 4, 6, 8}, then 1 <= E <= 2^30; the message names the
// first one violated.  On success *S = ceil(E / m) and *scale = 1 / sqrt(2 (4^(m/2) - 1) / 3); either
// pointer may be null.
QamStatus qam_check(int32_t m, int64_t E, int64_t* S, double* scale);

// ---- block Rayleigh fading; the definition: include/polarldpc.h at pl_qam_fading_check ----
constexpr int64_t kQamMaxCoherence = (int64_t)1 << 30;
constexpr uint32_t SALT_FADE = 0xFADE9A3Au;  // the coefficients' salt in the stream contract

// qam_check's two conditions in its order, then 1 <= coherence <= 2^30; the message names the first one
// violated.  On success *S = ceil(E / m) and *Q = ceil(S / coherence); either pointer may be null.
QamStatus qam_fading_check(int32_t m, int64_t E, int64_t coherence, int64_t* S, int64_t* Q);

}  // namespace pl

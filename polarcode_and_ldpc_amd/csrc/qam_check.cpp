// The QAM modem's parameter check (qam_check.hpp): no HIP, no device call.
#include "qam_check.hpp"

#include <cmath>

#include "../../include/polarldpc.h"

namespace pl {

QamStatus qam_check(int32_t m, int64_t E, int64_t* S, double* scale) {
    if (m != 2 && m != 4 && m != 6 && m != 8)
        return {PL_EINVAL, "m = " + std::to_string(m) + " must be 2, 4, 6 or 8 bits per symbol"};
    if (E < 1 || E > kQamMaxE) return {PL_EINVAL, "E = " + std::to_string(E) + " outside 1 .. 2^30"};
    const int h = m / 2;
    const int64_t D = 2 * (((int64_t)1 << (2 * h)) - 1) / 3;  // 2, 10, 42, 170: exact
    if (S) *S = (E + m - 1) / m;
    if (scale) *scale = 1.0 / std::sqrt((double)D);
    return {};
}

QamStatus qam_fading_check(int32_t m, int64_t E, int64_t coherence, int64_t* S, int64_t* Q) {
    int64_t s = 0;
    QamStatus st = qam_check(m, E, &s, nullptr);
    if (st.code) return st;
    if (coherence < 1 || coherence > kQamMaxCoherence)
        return {PL_EINVAL, "coherence = " + std::to_string(coherence) + " outside 1 .. 2^30"};
    if (S) *S = s;
    if (Q) *Q = (s + coherence - 1) / coherence;  // s <= 2^30 and coherence <= 2^30: no overflow
    return {};
}

}  // namespace pl

// qam_check (csrc/qam_check.cpp) under AddressSanitizer + UBSan, stand-alone: every m in a
// range around the four valid ones and E around its two limits, valid or not.  A valid
// pair must give S = ceil(E / m) and scale = 1 / sqrt(2 (4^(m/2) - 1) / 3); an invalid one
// PL_EINVAL with a message that names the first condition violated, and untouched outputs.
// Null output pointers are allowed.  Compiled with qam_check.cpp alone: no HIP, no library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/polarldpc.h"
#include "../../polarcode_and_ldpc_amd/csrc/qam_check.hpp"

static long g_valid = 0, g_refused = 0;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static int one(int32_t m, int64_t E) {
    int64_t S = -77;
    double scale = -77.0;
    const pl::QamStatus st = pl::qam_check(m, E, &S, &scale);
    const bool m_ok = m == 2 || m == 4 || m == 6 || m == 8;
    const bool e_ok = E >= 1 && E <= ((int64_t)1 << 30);
    if (!m_ok || !e_ok) {
        CHECK(st.code == PL_EINVAL && !st.msg.empty());
        CHECK(S == -77 && scale == -77.0);
        // the first violated condition is the one named
        CHECK(st.msg.compare(0, 4, m_ok ? "E = " : "m = ") == 0);
        CHECK(pl::qam_check(m, E, nullptr, nullptr).code == PL_EINVAL);
        ++g_refused;
        return 0;
    }
    CHECK(st.code == PL_OK && st.msg.empty());
    CHECK(S == (E + m - 1) / m && S * m >= E && (S - 1) * m < E);
    int64_t D = 0;  // sum of a^2 + b^2 over the levels, over 4^h points: 2 (4^h - 1) / 3
    const int h = m / 2, L = 1 << h;
    for (int a = -(L - 1); a < L; a += 2) D += 2 * (int64_t)a * a;
    CHECK(D % L == 0);
    D /= L;
    CHECK(3 * D == 2 * (((int64_t)1 << (2 * h)) - 1));
    CHECK(scale == 1.0 / std::sqrt((double)D));
    CHECK(pl::qam_check(m, E, nullptr, nullptr).code == PL_OK);
    int64_t S2 = 0;
    CHECK(pl::qam_check(m, E, &S2, nullptr).code == PL_OK && S2 == S);
    ++g_valid;
    return 0;
}

int main() {
    const int64_t top = (int64_t)1 << 30;
    const int64_t Es[] = {std::numeric_limits<int64_t>::min(), -top, -1, 0, 1, 2, 3, 5, 7, 8, 9, 1000, top - 1, top, top + 1,
                          (int64_t)1 << 31, ((int64_t)1 << 31) + 1, (int64_t)1 << 32, std::numeric_limits<int64_t>::max()};
    const int32_t ms[] = {std::numeric_limits<int32_t>::min(), -8, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 64,
                          std::numeric_limits<int32_t>::max()};
    for (int32_t m : ms)
        for (int64_t E : Es)
            if (one(m, E)) return 1;
    if (g_valid != 4 * 10 || g_refused == 0) {
        std::printf("FAILED: %ld valid, %ld refused\n", g_valid, g_refused);
        return 1;
    }
    std::printf("all checks passed: %ld valid, %ld refused\n", g_valid, g_refused);
    return 0;
}

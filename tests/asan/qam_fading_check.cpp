// qam_fading_check (csrc/qam_check.cpp) under AddressSanitizer + UBSan, stand-alone: m around the four valid
// ones, E and the coherence length around their limits, valid or not.  A valid triple must give S = ceil(E / m)
// and Q = ceil(S / coherence); an invalid one PL_EINVAL with a message that names the first condition violated,
// in the order m, E, coherence, and untouched outputs.  Null output pointers are allowed.  Compiled with
// qam_check.cpp alone: no HIP, no library.
#include <cstdint>
#include <cstdio>
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

static int one(int32_t m, int64_t E, int64_t Lc) {
    const int64_t top = (int64_t)1 << 30;
    int64_t S = -77, Q = -77;
    const pl::QamStatus st = pl::qam_fading_check(m, E, Lc, &S, &Q);
    const bool m_ok = m == 2 || m == 4 || m == 6 || m == 8;
    const bool e_ok = E >= 1 && E <= top;
    const bool c_ok = Lc >= 1 && Lc <= top;
    if (!m_ok || !e_ok || !c_ok) {
        CHECK(st.code == PL_EINVAL && !st.msg.empty());
        CHECK(S == -77 && Q == -77);
        const char* first = !m_ok ? "m = " : !e_ok ? "E = " : "coherence = ";
        CHECK(st.msg.rfind(first, 0) == 0);
        CHECK(pl::qam_fading_check(m, E, Lc, nullptr, nullptr).code == PL_EINVAL);
        ++g_refused;
        return 0;
    }
    CHECK(st.code == PL_OK && st.msg.empty());
    int64_t S0 = 0;
    CHECK(pl::qam_check(m, E, &S0, nullptr).code == PL_OK && S == S0);
    CHECK(Q >= 1 && Q <= S && (Q - 1) * Lc < S && (S <= Lc ? Q == 1 : Q * Lc >= S));
    CHECK(pl::qam_fading_check(m, E, Lc, nullptr, nullptr).code == PL_OK);
    int64_t Q2 = 0, S2 = 0;
    CHECK(pl::qam_fading_check(m, E, Lc, nullptr, &Q2).code == PL_OK && Q2 == Q);
    CHECK(pl::qam_fading_check(m, E, Lc, &S2, nullptr).code == PL_OK && S2 == S);
    ++g_valid;
    return 0;
}

int main() {
    static_assert(pl::SALT_FADE == 0xFADE9A3Au, "the coefficients' salt");
    const int64_t top = (int64_t)1 << 30;
    const int64_t lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::max();
    const int64_t Es[] = {lo, -1, 0, 1, 2, 7, 8, 9, 1000, top - 1, top, top + 1, (int64_t)1 << 32, hi};
    const int64_t Ls[] = {lo, -top, -1, 0, 1, 2, 3, 124, 125, 126, 499, 500, 501, top - 1, top, top + 1, (int64_t)1 << 31, hi};
    const int32_t ms[] = {std::numeric_limits<int32_t>::min(), -2, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16,
                          std::numeric_limits<int32_t>::max()};
    for (int32_t m : ms)
        for (int64_t E : Es)
            for (int64_t Lc : Ls)
                if (one(m, E, Lc)) return 1;
    if (g_valid != 4 * 8 * 11 || g_refused == 0) {
        std::printf("FAILED: %ld valid, %ld refused\n", g_valid, g_refused);
        return 1;
    }
    std::printf("all checks passed: %ld valid, %ld refused\n", g_valid, g_refused);
    return 0;
}

// rate_match_check (csrc/ldpc_plan.cpp) under AddressSanitizer + UBSan, stand-alone:
// every parameter set of a few small codes, valid or not.  A valid one must give
// the derived fields of the selection loop written out here (include/polarldpc.h,
// pl_rate_match); an invalid one PL_EINVAL with a message and untouched derived
// fields.  Compiled with ldpc_plan.cpp alone: no HIP, no library.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/polarldpc.h"
#include "../../polarcode_and_ldpc_amd/csrc/ldpc_plan.hpp"

static long g_valid = 0, g_refused = 0;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static int one(int mb, int nb, int z, int punctured, int F, int ncb_in, int start, int E) {
    pl_rate_match rm;
    std::memset(&rm, 0x5A, sizeof rm);
    rm.mb = mb; rm.nb = nb; rm.z = z; rm.punctured = punctured; rm.fillers = F; rm.ncb = ncb_in; rm.start = start; rm.E = E;
    const pl_rate_match before = rm;
    const pl::PlanStatus st = pl::rate_match_check(&rm);
    const int kb = nb - mb, n = nb * z, k = kb * z, P = punctured * z;
    const int ncb = ncb_in < 0 ? n - P : ncb_in;
    const bool ok = mb >= 1 && nb >= 1 && z >= 1 && kb >= 1 && punctured >= 0 && punctured < kb && F >= 0 && F <= k - P &&
                    ncb >= k - P && ncb <= n - P && start >= 0 && start < ncb && E >= 1 && ncb - F >= 1;
    if (!ok) {
        CHECK(st.code == PL_EINVAL && !st.msg.empty());
        CHECK(std::memcmp(&rm, &before, sizeof rm) == 0);
        ++g_refused;
        return 0;
    }
    CHECK(st.code == PL_OK);
    // the loop
    std::vector<int> pos, count((size_t)n, 0);
    for (int t = 0, j = 0; t < E; ++j) {
        const int b = (start + j) % ncb;
        if (b >= k - P - F && b < k - P) continue;
        pos.push_back(P + b);
        ++t;
    }
    int hi = 0, reps = 0, M = 0, c0 = -1;
    for (int p : pos) { hi = p > hi ? p : hi; reps = ++count[(size_t)p] > reps ? count[(size_t)p] : reps; }
    for (int b = 0; b < ncb; ++b) {
        if (b >= k - P - F && b < k - P) continue;
        if (P + b == pos[0]) c0 = M;
        ++M;
    }
    CHECK(rm.n == n && rm.k == k && rm.P == P && rm.ncb == ncb);
    CHECK(rm.M == M && rm.c0 == c0 && rm.hi == hi && rm.max_reps == reps);
    const int lo = k - P - F;
    for (int t = 0; t < E; ++t) {  // the closed form
        const int c = (c0 + t) % M;
        CHECK(P + (c < lo ? c : c + F) == pos[(size_t)t]);
    }
    ++g_valid;
    return 0;
}

int main() {
    const int codes[][3] = {{1, 2, 1}, {1, 3, 2}, {2, 4, 3}, {3, 5, 2}, {2, 3, 4}, {2, 2, 3}, {3, 2, 1}, {0, 2, 2}, {1, 2, 0}};
    for (const auto& c : codes) {
        const int mb = c[0], nb = c[1], z = c[2], kb = nb - mb, n = nb * z, k = kb * z;
        for (int punctured = -1; punctured <= kb + 1; ++punctured)
            for (int F = -1; F <= k + 1; ++F)
                for (int ncb = -1; ncb <= n + 1; ++ncb)
                    for (int start = -1; start <= n + 1; ++start)
                        for (int E : {-1, 0, 1, 2, n / 2, n - 1, n, n + 1, 2 * n + 5, 3 * n})
                            if (one(mb, nb, z, punctured, F, ncb, start, E)) return 1;
    }
    CHECK(pl::rate_match_check(nullptr).code == PL_EINVAL);
    // the 32-bit edge: n = 2^31 - 1 passes, 2^31 is refused; E up to INT32_MAX
    pl_rate_match big{};
    big.mb = 1; big.nb = 2147483647; big.z = 1; big.ncb = -1; big.E = 2147483647;
    CHECK(pl::rate_match_check(&big).code == PL_OK && big.n == 2147483647 && big.M == big.n && big.hi == big.n - 1 && big.max_reps == 1);
    big.nb = 65536; big.z = 32768;
    CHECK(pl::rate_match_check(&big).code == PL_EINVAL);
    CHECK(g_valid > 1000 && g_refused > 1000);
    std::printf("all checks passed (%ld valid, %ld refused)\n", g_valid, g_refused);
    return 0;
}

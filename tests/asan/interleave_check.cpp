// ilv_check and ilv_pos (csrc/interleave_check.{hpp,cpp}) under AddressSanitizer + UBSan, stand-alone:
// the refusals in the definition's order with untouched outputs, and the index function -- the code the
// kernels run -- against the definition's loops at every small E and, at the largest sizes, against a
// count of the valid cells before a column taken from the row starts.  Compiled with
// interleave_check.cpp alone: no HIP, no library.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/polarldpc.h"
#include "../../polarcode_and_ldpc_amd/csrc/interleave_check.hpp"

static long g_valid = 0, g_refused = 0, g_index = 0;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                        \
        }                                                                    \
    } while (0)

// the row starts and lengths of the array e is written into
static void rows_of(int kind, int rows, int64_t E, int64_t dim, std::vector<int64_t>* st, std::vector<int64_t>* len) {
    const int64_t n = kind == PL_ILV_RECT ? rows : dim;
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i) {
        st->push_back(k);
        len->push_back(kind == PL_ILV_RECT ? dim : dim - i);
        k += len->back();
    }
    (void)E;
}

// the definition as loops: fill the cells, read the columns
static int small(int kind, int rows, int64_t E) {
    pl::IlvParams p;
    CHECK(pl::ilv_check(kind, rows, E, &p).code == PL_OK);
    std::vector<int64_t> st, len;
    rows_of(kind, rows, E, p.dim, &st, &len);
    std::vector<int64_t> pos((size_t)E, -1);
    int64_t out = 0;
    for (int64_t c = 0; c < p.dim; ++c)
        for (size_t i = 0; i < st.size(); ++i)
            if (c < len[i] && st[i] + c < E) pos[(size_t)(st[i] + c)] = out++;
    CHECK(out == E);
    for (int64_t k = 0; k < E; ++k) {
        CHECK((int64_t)pl::ilv_pos(kind, p, (uint32_t)k) == pos[(size_t)k]);
        ++g_index;
    }
    return 0;
}

// valid cells before column c of row i's cell, row by row, plus the row index
static int large(int kind, int rows, int64_t E) {
    pl::IlvParams p;
    CHECK(pl::ilv_check(kind, rows, E, &p).code == PL_OK);
    if (kind == PL_ILV_TRI) {
        const int64_t T = p.dim;
        CHECK(T * (T + 1) / 2 >= E && (T - 1) * T / 2 < E);
    } else {
        CHECK((int64_t)p.dim * rows >= E && ((int64_t)p.dim - 1) * rows < E);
    }
    std::vector<int64_t> st, len;
    rows_of(kind, rows, E, p.dim, &st, &len);
    std::vector<int64_t> ks;
    for (int64_t k = 0; k < 64 && k < E; ++k) ks.push_back(k), ks.push_back(E - 1 - k);
    uint64_t x = 0x9E3779B97F4A7C15ull ^ (uint64_t)E;
    for (int j = 0; j < 512; ++j) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        ks.push_back((int64_t)((x >> 20) % (uint64_t)E));
    }
    for (int64_t k : ks) {
        const size_t i = (size_t)(std::upper_bound(st.begin(), st.end(), k) - st.begin()) - 1;
        const int64_t c = k - st[i];
        int64_t before = 0;
        for (size_t r = 0; r < st.size(); ++r) {
            const int64_t cells = std::max<int64_t>(0, std::min(len[r], E - st[r]));
            before += std::min(c, cells);
        }
        CHECK((int64_t)pl::ilv_pos(kind, p, (uint32_t)k) == before + (int64_t)i);
        ++g_index;
    }
    return 0;
}

static int one(int32_t kind, int32_t rows, int64_t E) {
    pl::IlvParams p;
    p.E = p.dim = p.Rf = p.q = p.a = 77u;
    const pl::IlvStatus st = pl::ilv_check(kind, rows, E, &p);
    const bool kind_ok = kind == PL_ILV_RECT || kind == PL_ILV_TRI;
    const bool e_ok = E >= 1 && E <= ((int64_t)1 << 30);
    const bool rows_ok = kind == PL_ILV_RECT ? rows >= 1 && rows <= 64 : rows == 0;
    if (!kind_ok || !e_ok || !rows_ok) {
        CHECK(st.code == PL_EINVAL && !st.msg.empty());
        CHECK(p.E == 77u && p.dim == 77u && p.Rf == 77u && p.q == 77u && p.a == 77u);
        // the first violated condition is the one named
        CHECK(st.msg.compare(0, 4, !kind_ok ? "kind" : !e_ok ? "E = " : "rows") == 0);
        CHECK(pl::ilv_check(kind, rows, E, nullptr).code == PL_EINVAL);
        ++g_refused;
        return 0;
    }
    CHECK(st.code == PL_OK && st.msg.empty() && p.E == (uint32_t)E);
    CHECK(pl::ilv_check(kind, rows, E, nullptr).code == PL_OK);
    ++g_valid;
    return E <= 700 ? small(kind, rows, E) : large(kind, rows, E);
}

int main() {
    const int64_t top = (int64_t)1 << 30;
    const int64_t t1 = 1000 * 1001 / 2, t2 = (int64_t)46340 * 46341 / 2;
    const int64_t Es[] = {std::numeric_limits<int64_t>::min(), -top, -1, 0, 1, 2, 3, 5, 6, 7, 10, 63, 64, 65, 300, 599,
                          600, t1 - 1, t1, t1 + 1, t2 - 1, t2, t2 + 1, top - 1, top, top + 1, (int64_t)1 << 31,
                          ((int64_t)1 << 32) + 5, std::numeric_limits<int64_t>::max()};
    const int32_t kinds[] = {std::numeric_limits<int32_t>::min(), -1, 0, 1, 2, 3, std::numeric_limits<int32_t>::max()};
    const int32_t rows[] = {std::numeric_limits<int32_t>::min(), -1, 0, 1, 2, 3, 4, 6, 8, 10, 63, 64, 65, 256,
                            std::numeric_limits<int32_t>::max()};
    for (int32_t kind : kinds)
        for (int32_t r : rows)
            for (int64_t E : Es)
                if (one(kind, r, E)) return 1;
    // every small E, as the host tests: TRI 1 .. 600, RECT 1 .. 300 with their rows
    for (int64_t E = 1; E <= 600; ++E)
        if (small(PL_ILV_TRI, 0, E)) return 1;
    for (int64_t E = 1; E <= 300; ++E)
        for (int32_t r : {1, 2, 3, 4, 6, 8, 10, 64})
            if (small(PL_ILV_RECT, r, E)) return 1;
    // the integer square root at its edges: squares, and one to either side, up to (2 46341 + 1)^2
    for (uint64_t r : {0ull, 1ull, 2ull, 3ull, 1000ull, 65535ull, 65536ull, 92681ull, 92682ull, 92683ull}) {
        CHECK(pl::ilv_isqrt(r * r) == r && pl::ilv_isqrt(r * r + 1) == (r == 0 ? 1 : r));
        if (r > 0) CHECK(pl::ilv_isqrt(r * r - 1) == r - 1);
    }
    if (g_valid != 21 * (1 + 9) || g_refused == 0) {
        std::printf("FAILED: %ld valid, %ld refused\n", g_valid, g_refused);
        return 1;
    }
    std::printf("all checks passed: %ld valid, %ld refused, %ld positions\n", g_valid, g_refused, g_index);
    return 0;
}

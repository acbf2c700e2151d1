// The quasi-cyclic encoder's plan builder (csrc/ldpc_plan.cpp,
// qc_encoder_plan_build) under AddressSanitizer + UBSan, compiled together with
// this file alone: no HIP, no library.  Every refusal must come back with its
// code and a message, the shift array is read within [mb][nb] only, and the
// stream of a valid plan parses back, front to back, to the base matrix, with
// the synchronisation flags the documented rule gives.
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/polarldpc.h"
#include "../../polarcode_and_ldpc_amd/csrc/ldpc_plan.hpp"

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// A base of the structure: message column j has dv blocks in rows (j + k) mod mb
// of shift (3 j + 5 k) mod z; a core of g rows with x = 1, shifts (a, b) = (2 mod z,
// 5 mod z); extension row i has the diagonal shift (7 i) mod z and one more block
// in parity column (chained ? i - 1 : 0) of shift (i + 1) mod z, where that column exists.
// So a chained extension asks for a synchronisation per row that has such a block, and an
// unchained one for none behind a core (p_0 is visible since the core's own) and for one, in
// row 1, without a core.
static std::vector<int32_t> base(int mb, int nb, int z, int dv, int g, bool chained) {
    const int kb = nb - mb;
    std::vector<int32_t> s((size_t)mb * nb, -1);
    auto at = [&](int i, int j) -> int32_t& { return s[(size_t)i * nb + j]; };
    for (int j = 0; j < kb; ++j)
        for (int k = 0; k < dv; ++k) at((j + k) % mb, j) = (3 * j + 5 * k) % z;
    if (g > 0) {
        at(0, kb) = at(g - 1, kb) = 2 % z;
        at(1, kb) = 5 % z;
        for (int t = 1; t < g; ++t) at(t - 1, kb + t) = at(t, kb + t) = 0;
    }
    for (int i = g; i < mb; ++i) {
        at(i, kb + i) = (7 * i) % z;
        if (i > 0) at(i, kb + (chained ? i - 1 : 0)) = (i + 1) % z;
    }
    return s;
}

static bool refused(int code, const pl::PlanStatus& st) { return st.code == code && !st.msg.empty(); }

int main() {
    pl::QcEncHostPlan hp;
    struct Shape { int mb, nb, z, dv, g, chained, subwave, fpw, threads, n_sync; };
    const Shape shapes[] = {
        {4, 8, 1, 3, 4, 1, 1, 64, 256, 1},   {4, 8, 7, 3, 4, 1, 1, 9, 256, 1},    {4, 8, 27, 3, 4, 1, 1, 2, 256, 1},
        {4, 8, 64, 3, 4, 1, 1, 1, 256, 1},   {4, 8, 96, 3, 4, 1, 0, 1, 128, 1},   {6, 10, 7, 3, 4, 1, 1, 9, 256, 3},
        {6, 10, 7, 3, 4, 0, 1, 9, 256, 1},   {8, 12, 65, 3, 4, 1, 0, 1, 128, 5},  {8, 12, 65, 3, 4, 0, 0, 1, 128, 1},
        {4, 8, 96, 3, 0, 1, 0, 1, 128, 3},   {4, 8, 27, 3, 0, 0, 1, 2, 256, 1},   {3, 5, 2, 2, 3, 1, 1, 32, 256, 1},
        {7, 12, 33, 3, 3, 1, 1, 1, 256, 5},  {3, 5, 1024, 2, 3, 1, 0, 1, 1024, 1}, {46, 68, 384, 3, 4, 0, 0, 1, 384, 1},
        {1, 2, 5, 1, 0, 1, 1, 12, 256, 0}};
    for (const Shape& sh : shapes) {
        const std::vector<int32_t> s = base(sh.mb, sh.nb, sh.z, sh.dv, sh.g, sh.chained != 0);
        const pl::PlanStatus st = pl::qc_encoder_plan_build(sh.mb, sh.nb, sh.z, s.data(), &hp);
        EXPECT(st.code == PL_OK);
        if (st.code != PL_OK) {
            std::fprintf(stderr, "  (%d, %d, %d, g %d): %s\n", sh.mb, sh.nb, sh.z, sh.g, st.msg.c_str());
            continue;
        }
        const pl::QcEncGeom& q = hp.geom;
        const int kb = sh.nb - sh.mb;
        EXPECT(q.g == sh.g && q.kb == kb && q.k == kb * sh.z && q.n == sh.nb * sh.z);
        EXPECT(q.subwave == sh.subwave && q.fpw == sh.fpw && q.threads == sh.threads);
        EXPECT(q.frame_bytes % 16 == 0 && q.frame_bytes >= (sh.nb + sh.g) * sh.z && q.frame_bytes < (sh.nb + sh.g) * sh.z + 16);
        EXPECT(q.lds_bytes == q.frame_bytes * q.fpw * q.fpb && q.lds_bytes <= pl::kQcEncLdsMax && q.fpb >= 1 && q.fpb <= 4);
        EXPECT(hp.n_sync == sh.n_sync);
        if (sh.g > 0) EXPECT(hp.x == 1 && hp.a == 2 % sh.z && hp.b == 5 % sh.z);
        // the stream parses back to the base matrix
        const std::vector<int32_t>& t = hp.tables;
        size_t at = 4;
        EXPECT(t.size() >= 4 && t[0] == sh.g && t[1] == hp.x && t[2] == hp.a && t[3] == hp.b);
        std::vector<int32_t> back((size_t)sh.mb * sh.nb, -1);
        auto B = [&](int i, int j) -> int32_t& { return back[(size_t)i * sh.nb + j]; };
        for (int i = 0; i < sh.g && at < t.size(); ++i) {
            const int d = t[at];
            for (int j = 0; j < d; ++j) {
                const int col = t[at + 1 + 2 * j];
                EXPECT(col >= 0 && col < kb && (j == 0 || col > t[at - 1 + 2 * j]));
                if (col >= 0 && col < kb) B(i, col) = t[at + 2 + 2 * j];
            }
            at += 1 + 2 * (size_t)d;
        }
        if (sh.g > 0) {
            B(0, kb) = B(sh.g - 1, kb) = hp.a;
            B(hp.x, kb) = hp.b;
            for (int c = 1; c < sh.g; ++c) B(c - 1, kb + c) = B(c, kb + c) = 0;
        }
        int syncs = sh.g > 0 ? 1 : 0;
        for (int i = sh.g; i < sh.mb && at + 2 < t.size(); ++i) {
            B(i, kb + i) = t[at];
            EXPECT(t[at + 1] == 0 || t[at + 1] == 1);
            syncs += t[at + 1];
            const int d = t[at + 2];
            for (int j = 0; j < d; ++j) {
                const int col = t[at + 3 + 2 * j];
                EXPECT(col >= 0 && col < kb + i && (j == 0 || col > t[at + 1 + 2 * j]));
                if (col >= 0 && col < kb + i) B(i, col) = t[at + 4 + 2 * j];
            }
            at += 3 + 2 * (size_t)d;
        }
        EXPECT(at == t.size() && back == s && syncs == hp.n_sync);
    }

    // refusals
    const std::vector<int32_t> good = base(6, 10, 7, 3, 4, true);  // kb = 4
    auto with = [&](int i, int j, int v) {
        std::vector<int32_t> b = good;
        b[(size_t)i * 10 + j] = v;
        return b;
    };
    auto build = [&](int mb, int nb, int z, const std::vector<int32_t>& s) {
        return pl::qc_encoder_plan_build(mb, nb, z, s.data(), &hp);
    };
    EXPECT(build(6, 10, 7, good).code == PL_OK);
    EXPECT(refused(PL_EINVAL, build(0, 10, 7, good)));
    EXPECT(refused(PL_EINVAL, build(6, 0, 7, good)));
    EXPECT(refused(PL_EINVAL, build(6, 10, 0, good)));
    EXPECT(refused(PL_EINVAL, build(6, 10, -3, good)));
    EXPECT(refused(PL_EINVAL, pl::qc_encoder_plan_build(6, 10, 7, nullptr, &hp)));
    EXPECT(refused(PL_EINVAL, build(6, 6, 7, good)));   // kb = 0, before any shift is read
    EXPECT(refused(PL_EINVAL, build(10, 6, 7, good)));  // kb < 0
    const std::vector<int32_t> two = {0, 0};
    EXPECT(refused(PL_EINVAL, build(1, 2, 1 << 30, two)));  // nb z = 2^31
    for (int bad : {-2, 7, INT32_MAX, INT32_MIN}) EXPECT(refused(PL_EINVAL, build(6, 10, 7, with(1, 2, bad))));
    EXPECT(refused(PL_EUNSUPPORTED, build(1, 2, 1025, two)));
    EXPECT(refused(PL_EINVAL, build(1, 2, 1025, std::vector<int32_t>{0, 1025})));  // EINVAL comes first
    EXPECT(build(1, 2, 1024, two).code == PL_OK);
    // the structure
    EXPECT(refused(PL_EUNSUPPORTED, build(6, 10, 7, with(3, 4, 3))));   // unequal first / last shift of column kb
    EXPECT(refused(PL_EUNSUPPORTED, build(6, 10, 7, with(1, 6, 3))));   // a dual-diagonal shift
    EXPECT(refused(PL_EUNSUPPORTED, build(6, 10, 7, with(2, 4, 2))));   // a fourth block in column kb
    EXPECT(refused(PL_EUNSUPPORTED, build(6, 10, 7, with(1, 4, -1))));  // two blocks in column kb
    EXPECT(refused(PL_EUNSUPPORTED, build(6, 10, 7, with(4, 9, 1))));   // right of an extension diagonal
    EXPECT(refused(PL_EUNSUPPORTED, build(6, 10, 7, with(5, 9, -1))));  // no diagonal block in the last row
    EXPECT(refused(PL_EUNSUPPORTED, build(6, 10, 7, with(0, 9, 1))));   // a core row reaching into the extension
    EXPECT(refused(PL_EUNSUPPORTED, build(6, 10, 7, with(2, 6, -1))));  // a dual-diagonal block missing
    {  // g = 2
        std::vector<int32_t> b(15, -1);
        for (int i = 0; i < 3; ++i) b[(size_t)i * 5] = 1, b[(size_t)i * 5 + 1] = 2;
        b[2] = b[3] = b[5 + 3] = b[5 + 2] = b[10 + 4] = 0;
        const pl::PlanStatus st = build(3, 5, 7, b);
        EXPECT(refused(PL_EUNSUPPORTED, st) && st.msg.find("g = 2") != std::string::npos);
    }
    {  // LDS: 161 block columns of 1024 bits; one fewer fits exactly
        std::vector<int32_t> b(2 * 161, -1);
        b[0] = b[161] = 0;
        b[161 - 2] = b[161 + 161 - 1] = 0;
        EXPECT(refused(PL_EUNSUPPORTED, build(2, 161, 1024, b)));
        std::vector<int32_t> c(2 * 160, -1);
        c[0] = c[160] = 0;
        c[160 - 2] = c[160 + 160 - 1] = 0;
        EXPECT(build(2, 160, 1024, c).code == PL_OK && hp.geom.lds_bytes == 160 * 1024);
        // z <= 64: the wavefront's frames count together (2 x 81952 bytes; 2 x 81920 fit exactly)
        std::vector<int32_t> d(2 * 2561, -1);
        d[0] = d[2561] = 0;
        d[2561 - 2] = d[2561 + 2561 - 1] = 0;
        EXPECT(refused(PL_EUNSUPPORTED, build(2, 2561, 32, d)));
        std::vector<int32_t> e(2 * 2560, -1);
        e[0] = e[2560] = 0;
        e[2560 - 2] = e[2560 + 2560 - 1] = 0;
        EXPECT(build(2, 2560, 32, e).code == PL_OK && hp.geom.fpw == 2 && hp.geom.fpb == 1 &&
               hp.geom.lds_bytes == 160 * 1024);
    }

    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("all checks passed");
    return 0;
}

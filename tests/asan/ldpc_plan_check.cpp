// The host-side LDPC planner (csrc/ldpc_plan.cpp) under AddressSanitizer +
// UBSan, compiled together with this file alone: no HIP, no library.  Bad
// arguments must come back as PL_EINVAL / PL_EUNSUPPORTED with their message --
// a row_ptr that is not monotone before any col_idx entry is read -- and one
// valid plan per kernel family is built so that every table write is seen.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
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

struct Csr {
    int m, n;
    std::vector<int32_t> rp, ci;
};

// (dv, dc)-regular H without repeated edges: variable v, edge k joins check
// (v + k * stride) mod m, the variables taken in a shuffled order
static Csr regular_code(int n, int dv, int dc) {
    const int m = n * dv / dc, stride = m / dv;
    std::vector<int> perm(n);
    for (int v = 0; v < n; ++v) perm[v] = v;
    std::mt19937 rng(n);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<std::vector<int32_t>> rows(m);
    for (int v = 0; v < n; ++v)
        for (int k = 0; k < dv; ++k) rows[(v + k * stride) % m].push_back(perm[v]);
    Csr h{m, n, {0}, {}};
    for (auto& r : rows) {
        std::sort(r.begin(), r.end());
        h.ci.insert(h.ci.end(), r.begin(), r.end());
        h.rp.push_back((int32_t)h.ci.size());
    }
    return h;
}

static pl::PlanStatus flooding(const Csr& h, int algo, int max_iter, pl::LdpcHostPlan* hp,
                               const pl::LdpcPlanOptions& opt = {}) {
    return pl::ldpc_plan_build(h.m, h.n, h.rp.data(), h.ci.data(), algo, max_iter, 1, 0.75, opt, hp);
}
static pl::PlanStatus layered(const Csr& h, const std::vector<std::vector<int32_t>>& layers, int max_iter,
                              pl::LmsHostPlan* hp) {
    std::vector<int32_t> lp = {0}, lr;
    for (const auto& l : layers) {
        lr.insert(lr.end(), l.begin(), l.end());
        lp.push_back((int32_t)lr.size());
    }
    return pl::lms_plan_build(h.m, h.n, h.rp.data(), h.ci.data(), (int)layers.size(), lp.data(), lr.data(), max_iter, 1,
                              0.75, {}, hp);
}
static bool refused(const pl::PlanStatus& st, int code, const char* what) {
    return st.code == code && st.msg.find(what) != std::string::npos;
}

int main() {
    pl::LdpcHostPlan hp;
    pl::LmsHostPlan lhp;
    const std::vector<std::vector<int32_t>> two = {{0}, {1}};
    // row_ptr past the end or descending: refused before col_idx is read there
    // (col_idx has exactly E = row_ptr[m] entries, so a read past it is a heap overflow)
    for (int32_t mid : {7, 1000}) {
        const Csr bad{2, 8, {0, mid, 6}, {0, 1, 2, 3, 4, 5}};
        EXPECT(refused(flooding(bad, PL_LDPC_BP, 20, &hp), PL_EINVAL, "monotone"));
        EXPECT(refused(flooding(bad, PL_LDPC_MS, 20, &hp), PL_EINVAL, "monotone"));
        EXPECT(refused(layered(bad, two, 5, &lhp), PL_EINVAL, "monotone"));
    }
    // the LDPC cases of capi_args.cpp
    const Csr ok{2, 4, {0, 3, 6}, {0, 1, 2, 1, 2, 3}};
    EXPECT(refused(flooding(ok, 7, 20, &hp), PL_EINVAL, "algo"));
    EXPECT(refused(flooding(ok, PL_LDPC_BP, 0, &hp), PL_EINVAL, "max_iter"));
    EXPECT(pl::ldpc_plan_build(2, 4, nullptr, ok.ci.data(), PL_LDPC_BP, 20, 1, 1.0, {}, &hp).code == PL_EINVAL);
    EXPECT(refused(flooding(Csr{2, 4, {0, 3, 6}, {0, 1, 4, 1, 2, 3}}, PL_LDPC_BP, 20, &hp), PL_EINVAL, "out of range"));
    EXPECT(refused(flooding(Csr{2, 4, {0, 3, 6}, {0, 2, 1, 1, 2, 3}}, PL_LDPC_BP, 20, &hp), PL_EINVAL, "ascend"));
    EXPECT(refused(flooding(Csr{2, 4, {1, 3, 6}, ok.ci}, PL_LDPC_BP, 20, &hp), PL_EINVAL, "row_ptr[0]"));
    const Csr deg1{2, 4, {0, 1, 5}, {0, 0, 1, 2, 3}};
    EXPECT(refused(flooding(deg1, PL_LDPC_MS, 20, &hp), PL_EUNSUPPORTED, "degree-1"));
    EXPECT(flooding(deg1, PL_LDPC_BP, 20, &hp).code == PL_OK);
    EXPECT(flooding(ok, PL_LDPC_BP, 20, &hp).code == PL_OK && pl::ldpc_kernel_code(hp.geom) == 1);
    // layered rules (tests/test_ldpc_layered_host.py): rows 0 and 1 share column 1
    const Csr lh{4, 6, {0, 2, 4, 6, 8}, {0, 1, 1, 2, 2, 3, 4, 5}};
    EXPECT(layered(lh, {{0, 3}, {1}, {2}}, 5, &lhp).code == PL_OK && lhp.geom.wave == 1 && lhp.geom.mw == 1);
    EXPECT(lhp.tables.size() == 5 + 8 + 4 + 4 && lhp.dev(lhp.tables.data()).layer_rows[3] == 2);
    EXPECT(refused(layered(lh, {{0, 3}, {1}, {1}}, 5, &lhp), PL_EINVAL, "row 1 repeats"));
    EXPECT(refused(layered(lh, {{0, 3}, {1}, {2}, {0}}, 5, &lhp), PL_EINVAL, "exactly once"));
    EXPECT(refused(layered(lh, {{0, 3}, {1}}, 5, &lhp), PL_EINVAL, "exactly once"));
    EXPECT(refused(layered(lh, {{0, 1}, {2, 3}}, 5, &lhp), PL_EINVAL, "share column 1"));
    EXPECT(refused(layered(lh, {{0, 3}, {1}, {2}}, -1, &lhp), PL_EINVAL, "max_iter"));
    const Csr l1{4, 6, {0, 2, 3, 5, 7}, {0, 1, 3, 2, 3, 4, 5}};
    EXPECT(refused(layered(l1, {{0, 1, 3}, {2}}, 5, &lhp), PL_EUNSUPPORTED, "degree-1"));
    EXPECT(layered(l1, {{0, 1, 3}, {2}}, 0, &lhp).code == PL_OK);  // no iteration evaluates the check

    // one valid plan per kernel family; the device pointers stay inside the table buffer
    struct Want { int n, algo, code; };
    for (const Want w : {Want{504, PL_LDPC_MS, 2}, Want{504, PL_LDPC_BP, 7}, Want{1000, PL_LDPC_BP, 7},
                         Want{2048, PL_LDPC_MS, 8}, Want{2048, PL_LDPC_BP, 1}}) {
        const Csr h = regular_code(w.n, 3, 6);
        EXPECT(flooding(h, w.algo, 20, &hp).code == PL_OK && pl::ldpc_kernel_code(hp.geom) == w.code);
        const pl::LdpcDev d = hp.dev(hp.tables.data());
        const int32_t* end = hp.tables.data() + hp.tables.size();
        EXPECT(d.var_cp + hp.geom.E <= end && d.row_ptr[hp.geom.m] == hp.geom.E);
        if (w.code == 7) EXPECT(d.var_tpos + 256 * 7 * pl::kLdpcRegVariants[hp.geom.reg_variant - 1].vpt + hp.geom.npad <= end);
        if (w.code == 8) EXPECT(reinterpret_cast<const int32_t*>(d.ms_vw) + 8 * h.n + 4 * h.m == end);
    }
    pl::LdpcPlanOptions compact;
    compact.kernel = pl::kLdpcKernelCompact;
    EXPECT(flooding(regular_code(2048, 3, 6), PL_LDPC_MS, 20, &hp, compact).code == PL_OK &&
           pl::ldpc_kernel_code(hp.geom) == 5);
    {
        const Csr h = regular_code(504, 3, 6);  // a layered plan on the block mapping: one layer per 84 rows
        std::vector<std::vector<int32_t>> layers(3);
        for (int c = 0; c < h.m; ++c) layers[c / 84].push_back(c);
        EXPECT(layered(h, layers, 20, &lhp).code == PL_OK && lhp.geom.wave == 0 && lhp.geom.max_layer == 84);
    }
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ldpc planner: all checks passed\n");
    return 0;
}

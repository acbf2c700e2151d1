// LDPC plan construction on the host (ldpc_plan.hpp): no device call, no
// environment read.  Flooding plans: CSR checks, the degree sort and adjacency
// tables, kernel selection, the degree-grouped BP tables, the (3,6) min-sum
// address words, all packed into one vector.  Layered plans: layer checks and
// the kernel geometry.  Quasi-cyclic layered plans: base-matrix checks, the
// geometry and the per-layer (block column, shift) stream.  Quasi-cyclic encoder
// plans: the core-plus-extension structure of the parity part and the encoder's stream.
#include "ldpc_plan.hpp"

#include <algorithm>

#include "../../include/polarldpc.h"

namespace pl {

static PlanStatus refuse(int code, std::string msg) { return {code, std::move(msg)}; }

PlanStatus csr_validate(int m, int n, const int32_t* row_ptr, const int32_t* col_idx, CsrInfo* info) {
    if (m < 0 || n < 1 || !row_ptr || (!col_idx && row_ptr[m] > 0)) return refuse(PL_EINVAL, "bad H");
    const int E = row_ptr[m];
    if (row_ptr[0] != 0 || E < 0) return refuse(PL_EINVAL, "row_ptr[0] must be 0");
    // row_ptr monotone and within [0, E] before any col_idx entry is read
    for (int c = 0; c < m; ++c)
        if (row_ptr[c + 1] < row_ptr[c] || row_ptr[c + 1] > E) return refuse(PL_EINVAL, "row_ptr not monotone");
    info->E = E;
    info->maxdc = 0;
    info->deg1 = false;
    for (int c = 0; c < m; ++c) {
        const int d = row_ptr[c + 1] - row_ptr[c];
        info->maxdc = std::max(info->maxdc, d);
        info->deg1 |= d == 1;
        for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
            if (col_idx[e] < 0 || col_idx[e] >= n) return refuse(PL_EINVAL, "column index out of range");
            if (e > row_ptr[c] && col_idx[e] <= col_idx[e - 1]) return refuse(PL_EINVAL, "columns must ascend");
        }
    }
    return {};
}

uint64_t plan_tables_digest(const std::vector<int32_t>& tables) {
    uint64_t h = 14695981039346656037ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(tables.data());
    for (size_t i = 0; i < tables.size() * sizeof(int32_t); ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// ---- flooding plans ----

// The code's graph in device edge order.
struct Adjacency {
    std::vector<int32_t> row_ptr, col_idx;  // checks sorted by degree
    std::vector<int32_t> edge_chk;          // edge -> (sorted) check
    std::vector<int32_t> var_ptr, var_edge; // per variable its edges, by ascending ORIGINAL check
    int maxdv = 0;
    int degree(int c) const { return row_ptr[c + 1] - row_ptr[c]; }
    int pos(int e) const { return e - row_ptr[edge_chk[e]]; }  // position of edge e in its check
};

// Device edge order: checks sorted by degree (stable), so the lanes of a
// wavefront run check loops of equal length; columns stay ascending within a
// check (the reference's product order).  No result depends on the check
// order: var_edge lists each variable's edges by ascending ORIGINAL check
// index, the order of the reference's np.sum over them (decoder.py:110-116).
static Adjacency build_adjacency(int m, int n, int E, const int32_t* row_ptr, const int32_t* col_idx) {
    Adjacency a;
    a.var_ptr.assign(n + 1, 0);
    for (int e = 0; e < E; ++e) a.var_ptr[col_idx[e] + 1]++;
    for (int v = 0; v < n; ++v) a.var_ptr[v + 1] += a.var_ptr[v];
    for (int v = 0; v < n; ++v) a.maxdv = std::max(a.maxdv, a.var_ptr[v + 1] - a.var_ptr[v]);
    std::vector<int32_t> order(m);
    for (int c = 0; c < m; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        return (row_ptr[x + 1] - row_ptr[x]) < (row_ptr[y + 1] - row_ptr[y]);
    });
    a.row_ptr.assign(m + 1, 0);
    a.col_idx.resize(E);
    a.edge_chk.resize(E);
    a.var_edge.resize(E);
    std::vector<int32_t> new_edge(E);  // new_edge[original edge]
    for (int k = 0; k < m; ++k) {
        const int c = order[k];
        a.row_ptr[k + 1] = a.row_ptr[k] + (row_ptr[c + 1] - row_ptr[c]);
        for (int e = row_ptr[c], j = a.row_ptr[k]; e < row_ptr[c + 1]; ++e, ++j) {
            a.col_idx[j] = col_idx[e];
            new_edge[e] = j;
            a.edge_chk[j] = k;
        }
    }
    std::vector<int32_t> fill(a.var_ptr.begin(), a.var_ptr.end() - 1);
    for (int e = 0; e < E; ++e) a.var_edge[fill[col_idx[e]]++] = new_edge[e];  // original check order
    return a;
}

// Which kernel family decodes the code; sets every selection field of g but
// grp / fpg / tl / npad (build_grp_tables: that choice needs the padded layout).
static void select_kernel(LdpcGeom& g, const Adjacency& a, const LdpcPlanOptions& opt) {
    const int m = g.m, n = g.n, E = g.E;
    bool const_dv = true;
    for (int v = 0; v < n && const_dv; ++v) const_dv = (a.var_ptr[v + 1] - a.var_ptr[v]) == g.maxdv;
    g.regular = const_dv;
    for (int c = 0; c < m && g.regular; ++c) g.regular = a.degree(c) == g.maxdc;
    // generic kernel (ldpc_decode_kernel): T, C in LDS while they fit, else in the workspace
    g.threads = E <= 4096 ? 256 : 1024;
    g.use_global = ldpc_generic_lds(E, m, n) > kLdpcGenericLdsMax ? 1 : 0;
    g.lds_bytes = (int)ldpc_align16(g.use_global ? ldpc_small_lds(m, n) : ldpc_generic_lds(E, m, n));
    // check-per-thread kernel (ldpc_check_kernel): diagnostic build only
    g.check_kernel = !g.use_global && opt.kernel == kLdpcKernelCheck ? 1 : 0;
    // register-cached kernel: constant variable degree < 8, LDS-resident state
    g.reg_variant = 0;
    if (!g.use_global && !g.check_kernel && opt.kernel != kLdpcKernelGeneric) {
        if (const_dv && g.maxdv < 8 && E < 65536) g.reg_variant = ldpc_reg_variant(g.maxdv, E, n);
        if (g.reg_variant) {
            g.threads = 256;
            g.lds_bytes = (int)ldpc_reg_lds(E, m, n, g.reg_variant);
        }
    }
    // min-sum codes whose T/C arrays exceed LDS: compressed check state in LDS
    g.compact = 0;
    if (g.use_global && g.algo == PL_LDPC_MS && g.maxdc <= 15 && opt.kernel != kLdpcKernelGeneric &&
        ldpc_compact_lds(m, n) <= kLdpcCompactLdsMax) {
        g.compact = 1;
        g.use_global = 0;
        g.threads = 1024;
        g.lds_bytes = (int)ldpc_compact_lds(m, n);
    }
    // (3,6)-regular min-sum of n = 2048 / 4096 / 8192 (the BASELINE n = 8192 code):
    // ldpc_ms36_kernel (the compact override keeps ldpc_ms_compact_kernel)
    g.ms36 = 0;
    if (g.compact && g.regular && g.maxdv == 3 && g.maxdc == 6 && 2 * m == n && ldpc_ms36_lds(n) > 0 &&
        opt.kernel != kLdpcKernelCompact) {
        g.ms36 = n / 1024;
        g.lds_bytes = ldpc_ms36_lds(n);
    }
    if (g.check_kernel) {
        g.threads = 256;
        g.lds_bytes = (int)ldpc_check_lds(E, n);
    }
}

// ldpc_bp_grp_kernel's variable -> thread-slot map (slot q = 256 j + tid;
// nslots >= n, -1 = empty).  The variable pass stores T'[tpos] (ds_write_b64:
// lane groups of 16, bank pair tpos mod 16) and reads C'[tpos] (ds_read_b64:
// lane groups of 32, element (tl + tpos) mod 32) for each of its DV edges; a
// group's cost is, per edge k, the largest number of its lanes on one bank.
// Greedy fill (each slot takes the unplaced variable that adds the fewest
// same-bank lanes to its two groups), then hill climbing over slot swaps
// (deterministic xorshift, sideways moves kept).  Any map gives the same
// decoding; only the LDS conflicts change (MI355X_MICROARCH.md, LDS).
static std::vector<int> ldpc_var_slots(int n, int dv, const std::vector<int32_t>& tp, int tl, int nslots) {
    std::vector<int> vm(nslots, -1);
    {
        std::vector<char> used(n, 0);
        std::vector<int> wcnt((size_t)dv * 16), rcnt((size_t)dv * 32);
        const int empty = nslots - n;  // empty slots go to the end of the last groups
        for (int q = 0; q < nslots - empty; ++q) {
            if ((q & 15) == 0) std::fill(wcnt.begin(), wcnt.end(), 0);
            if ((q & 31) == 0) std::fill(rcnt.begin(), rcnt.end(), 0);
            int best = -1, bc = 1 << 30;
            for (int v = 0; v < n; ++v) {
                if (used[v]) continue;
                int c = 0;
                for (int k = 0; k < dv; ++k) {
                    const int t = tp[(size_t)v * dv + k];
                    c += wcnt[(size_t)k * 16 + t % 16] + rcnt[(size_t)k * 32 + (t + tl) % 32];
                }
                if (c < bc) { bc = c; best = v; if (c == 0) break; }
            }
            used[best] = 1;
            vm[q] = best;
            for (int k = 0; k < dv; ++k) {
                const int t = tp[(size_t)best * dv + k];
                ++wcnt[(size_t)k * 16 + t % 16];
                ++rcnt[(size_t)k * 32 + (t + tl) % 32];
            }
        }
    }
    auto gcost = [&](int start, int size, int mod, int add) {
        int c = 0;
        for (int k = 0; k < dv; ++k) {
            int cnt[32] = {0}, mx = 0;
            for (int q = start; q < start + size; ++q) {
                const int v = vm[q];
                if (v < 0) continue;
                const int b = (tp[(size_t)v * dv + k] + add) % mod;
                mx = std::max(mx, ++cnt[b]);
            }
            c += mx;
        }
        return c;
    };
    auto groups_cost = [&](int a, int b) {
        const int wa = a & ~15, wb = b & ~15, ra = a & ~31, rb = b & ~31;
        int c = gcost(wa, 16, 16, 0) + gcost(ra, 32, 32, tl);
        if (wb != wa) c += gcost(wb, 16, 16, 0);
        if (rb != ra) c += gcost(rb, 32, 32, tl);
        return c;
    };
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const int iters = 40 * nslots;
    for (int it = 0; it < iters; ++it) {
        const int a = (int)(rnd() % (uint64_t)nslots), b = (int)(rnd() % (uint64_t)nslots);
        if (a == b || (vm[a] < 0 && vm[b] < 0)) continue;
        const int before = groups_cost(a, b);
        std::swap(vm[a], vm[b]);
        if (groups_cost(a, b) > before) std::swap(vm[a], vm[b]);
    }
    return vm;
}

// BP on a reg variant: degree-grouped check products (ldpc_bp_grp_kernel).
// Slot s holds edges 64 s .. 64 s + 63 (degree-sorted, check-major); D_s =
// the largest check degree among them; check c's inputs sit at T' offset
// off[c] (even), padded with 1.0 to the largest D_s of the slots holding its
// edges.  The reg override keeps ldpc_reg_kernel's per-lane products.  Sets
// g.grp / fpg / tl / npad / lds_bytes and fills grp_meta and var_tpos (with
// its pad list) when the padded layout fits.
static void build_grp_tables(LdpcGeom& g, const Adjacency& a, const LdpcPlanOptions& opt,
                             std::vector<int32_t>& grp_meta, std::vector<int32_t>& var_tpos) {
    g.grp = 0;
    g.tl = 0;
    if (!g.reg_variant || g.algo != PL_LDPC_BP || g.maxdc > 15 || opt.kernel == kLdpcKernelReg) return;
    const int m = g.m, n = g.n, E = g.E, dv = g.maxdv;
    const LdpcRegVariant& var = kLdpcRegVariants[g.reg_variant - 1];
    const int slots = 4 * var.ept;
    std::vector<int> dslot(slots, 0), dpad(m, 0), off(m + 1, 0);
    for (int e = 0; e < E; ++e) dslot[e / 64] = std::max(dslot[e / 64], a.degree(a.edge_chk[e]));
    for (int e = 0; e < E; ++e) dpad[a.edge_chk[e]] = std::max(dpad[a.edge_chk[e]], dslot[e / 64]);
    for (int c = 0; c < m; ++c) off[c + 1] = off[c] + ((dpad[c] + 1) & ~1);
    // T', C' positions [0, off[m]) hold the checks, [off[m], off[m] + 16) is a sink
    // for the lanes of a slot past the last edge (they read it and store into it)
    const int sink = off[m], tl = off[m] + 16;
    const size_t lds = ldpc_grp_lds(tl, m, g.reg_variant);
    if (tl >= 65536 || lds > kLdpcGenericLdsMax) return;
    g.grp = 1;
    // two frames per workgroup, one after the other (ldpc_bp_grp_kernel FPG):
    // valid codewords (early stop) 0.777 -> 0.742 ms per 65 536 frames, the
    // harness frames (20 iterations) equal; PL_BP_FPG=1 restores one.  Only
    // the (DV, EPT, VPT) = (3, 6, 2) instance: the larger ones' two-frame
    // builds spill 24-41 more VGPRs than their one-frame builds
    g.fpg = opt.bp_fpg ? opt.bp_fpg : (dv == 3 && var.ept == 6 ? 2 : 1);
    g.tl = tl;
    g.lds_bytes = (int)lds;
    // sorted slot s goes to the thread slot (j = s / 4, wavefront w) in snake
    // order (w = s % 4 for even j, 3 - s % 4 for odd j), so the four
    // wavefronts -- one per SIMD -- get products of about equal total length
    grp_meta.assign((size_t)slots * 64, 0);
    for (int s = 0; s < slots; ++s) {
        const int j = s / 4, w = (j & 1) ? 3 - (s & 3) : (s & 3);
        for (int l = 0; l < 64; ++l) {
            const int e = 64 * s + l, q = 256 * j + 64 * w + l;
            if (e < E) grp_meta[q] = off[a.edge_chk[e]] | (a.pos(e) << 16) | (dslot[s] << 20);
            else grp_meta[q] = sink | (15 << 16) | (dslot[s] << 20);  // reads and stores the sink (position 15 skips no factor)
        }
    }
    // variables in thread-slot order (slot q = 256 j + tid): T' position and
    // check of each edge, variable index (-1: empty); the order chosen so
    // the variable pass's scattered LDS accesses conflict little
    std::vector<int32_t> tp((size_t)n * dv), vck((size_t)n * dv);
    for (int v = 0; v < n; ++v)
        for (int k = 0; k < dv; ++k) {
            const int e = a.var_edge[a.var_ptr[v] + k], c = a.edge_chk[e];
            tp[(size_t)v * dv + k] = off[c] + a.pos(e);
            vck[(size_t)v * dv + k] = c;
        }
    const int nslots = 256 * var.vpt;
    const std::vector<int> vmap = ldpc_var_slots(n, dv, tp, tl, nslots);
    var_tpos.assign((size_t)nslots * (2 * dv + 1), 0);
    for (int q = 0; q < nslots; ++q) {
        const int v = vmap[q];
        var_tpos[(size_t)2 * dv * nslots + q] = v;
        for (int k = 0; k < dv; ++k) {
            var_tpos[(size_t)q * dv + k] = v >= 0 ? tp[(size_t)v * dv + k] : 0;
            var_tpos[(size_t)dv * nslots + (size_t)q * dv + k] = v >= 0 ? vck[(size_t)v * dv + k] : 0;
        }
    }
    // + the pad positions (T' = 1.0 from the first write on), -1 filled to 256
    std::vector<char> real(sink, 0);
    for (int e = 0; e < E; ++e) real[off[a.edge_chk[e]] + a.pos(e)] = 1;
    const size_t pads_at = var_tpos.size();
    for (int q = 0; q < sink; ++q)
        if (!real[q]) var_tpos.push_back(q);
    g.npad = (int)((var_tpos.size() - pads_at + 255) / 256 * 256);
    var_tpos.resize(pads_at + g.npad, -1);
}

// ldpc_ms36_kernel's address words.  [n][8]: per variable its three edge words
// and meta addresses; then [m][4]: per check the LDS byte addresses 8v of its
// six variables, two per word
static std::vector<int32_t> build_ms36_words(const LdpcGeom& g, const Adjacency& a) {
    const int m = g.m, n = g.n;
    const uint32_t REC = ldpc_ms36_rec(n), MET = ldpc_ms36_meta(n);
    std::vector<int32_t> vw((size_t)n * 8 + (size_t)m * 4, 0);
    for (int v = 0; v < n; ++v)
        for (int k = 0; k < 3; ++k) {
            const int e = a.var_edge[a.var_ptr[v] + k], c = a.edge_chk[e];
            vw[(size_t)v * 8 + k] = (int32_t)((REC + 16u * (uint32_t)c) | (3u * (uint32_t)a.pos(e)));
            vw[(size_t)v * 8 + 3 + k] = (int32_t)(MET + 4u * (uint32_t)c);
        }
    for (int c = 0; c < m; ++c)
        for (int k = 0; k < 3; ++k) {
            const uint32_t v0 = (uint32_t)a.col_idx[a.row_ptr[c] + 2 * k], v1 = (uint32_t)a.col_idx[a.row_ptr[c] + 2 * k + 1];
            vw[(size_t)n * 8 + (size_t)c * 4 + k] = (int32_t)((8u * v0) | ((8u * v1) << 16));
        }
    return vw;
}

PlanStatus ldpc_plan_build(int m, int n, const int32_t* row_ptr, const int32_t* col_idx, int algo, int max_iter,
                           int early_stop, double norm, const LdpcPlanOptions& opt, LdpcHostPlan* out) {
    CsrInfo csr;
    PlanStatus st = csr_validate(m, n, row_ptr, col_idx, &csr);
    if (st.code) return st;
    if (algo != PL_LDPC_BP && algo != PL_LDPC_MS) return refuse(PL_EINVAL, "algo must be BP or MS");
    if (max_iter < 1) return refuse(PL_EINVAL, "max_iter must be >= 1");
    if (algo == PL_LDPC_MS && csr.deg1)
        return refuse(PL_EUNSUPPORTED, "min-sum on a degree-1 check (reference raises ValueError)");
    const int E = csr.E;
    const Adjacency a = build_adjacency(m, n, E, row_ptr, col_idx);
    if (a.maxdv > 128) return refuse(PL_EUNSUPPORTED, "variable degree > 128");
    if (E >= (1 << 20) || csr.maxdc >= (1 << 11)) return refuse(PL_EUNSUPPORTED, "code too large");

    LdpcGeom& g = out->geom;
    g = LdpcGeom{};
    g.m = m; g.n = n; g.E = E; g.max_iter = max_iter; g.early_stop = early_stop ? 1 : 0; g.algo = algo;
    g.maxdc = csr.maxdc; g.maxdv = a.maxdv; g.norm = norm;
    select_kernel(g, a, opt);
    std::vector<int32_t> grp_meta, var_tpos, ms_vw;
    build_grp_tables(g, a, opt, grp_meta, var_tpos);
    if (g.ms36) ms_vw = build_ms36_words(g, a);

    std::vector<int32_t>& all = out->tables;
    LdpcDevAt& at = out->at;
    all.clear();
    auto append = [&](const std::vector<int32_t>& v) {
        const size_t pos = all.size();
        all.insert(all.end(), v.begin(), v.end());
        return pos;
    };
    at.row_ptr = append(a.row_ptr);
    at.col_idx = append(a.col_idx);
    at.edge_chk = append(a.edge_chk);
    at.var_ptr = append(a.var_ptr);
    at.var_edge = append(a.var_edge);
    std::vector<int32_t> edge_meta(E), var_chk(E), var_cp(E);
    for (int e = 0; e < E; ++e) edge_meta[e] = a.row_ptr[a.edge_chk[e]] | (a.degree(a.edge_chk[e]) << 20);
    for (int k = 0; k < E; ++k) {
        const int e = a.var_edge[k], c = a.edge_chk[e];
        var_chk[k] = c;
        var_cp[k] = (c << 4) | (a.pos(e) & 15);
    }
    at.edge_meta = append(edge_meta);
    at.var_chk = append(var_chk);
    at.var_cp = append(var_cp);
    at.grp_meta = append(grp_meta);
    at.var_tpos = append(var_tpos);
    all.resize((all.size() + 3) & ~(size_t)3, 0);  // ms_vw: 16-byte aligned (uint4 loads)
    at.ms_vw = append(ms_vw);
    return {};
}

// ---- layered plans ----

void lms_geom(LmsGeom* g, bool force_global) {
    constexpr int kLdsMax = 160 * 1024;
    g->mw = g->maxdc <= 16 ? 1 : 1 + (g->maxdc + 31) / 32;
    g->off_mm = (int64_t)ldpc_align16((size_t)8 * g->n);
    g->off_meta = g->off_mm + (int64_t)16 * g->m;
    g->state_bytes = (int64_t)ldpc_align16((size_t)g->off_meta + (size_t)4 * g->m * g->mw);
    g->wave = g->max_layer <= 64 ? 1 : 0;
    const int vote = g->wave ? 0 : kLdpcVoteBytes;
    g->use_global = (force_global || g->state_bytes + vote > kLdsMax) ? 1 : 0;
    if (g->wave) {
        g->fpb = g->use_global ? 4 : (int)std::max<int64_t>(1, std::min<int64_t>(4, 65536 / g->state_bytes));
        g->threads = 64 * g->fpb;
    } else {
        g->fpb = 1;
        g->threads = std::min(1024, (g->max_layer + 63) / 64 * 64);
    }
    g->lds_bytes = (g->use_global ? 0 : (int)g->state_bytes * g->fpb) + vote;
}

PlanStatus lms_plan_build(int m, int n, const int32_t* row_ptr, const int32_t* col_idx, int n_layers,
                          const int32_t* layer_ptr, const int32_t* layer_rows, int max_iter, int early_stop,
                          double norm, const LdpcPlanOptions& opt, LmsHostPlan* out) {
    CsrInfo csr;
    PlanStatus st = csr_validate(m, n, row_ptr, col_idx, &csr);
    if (st.code) return st;
    if (max_iter < 0) return refuse(PL_EINVAL, "max_iter must be >= 0");
    if (n_layers < 0 || !layer_ptr || (m > 0 && !layer_rows) || layer_ptr[0] != 0 || layer_ptr[n_layers] != m)
        return refuse(PL_EINVAL, "layers must list every row exactly once");
    int max_layer = 0;
    std::vector<uint8_t> seen((size_t)m, 0);
    std::vector<int32_t> mark((size_t)n, -1);  // last layer that touched the column
    for (int l = 0; l < n_layers; ++l) {
        if (layer_ptr[l + 1] < layer_ptr[l] || layer_ptr[l + 1] > m) return refuse(PL_EINVAL, "layer_ptr not monotone");
        max_layer = std::max(max_layer, layer_ptr[l + 1] - layer_ptr[l]);
        for (int k = layer_ptr[l]; k < layer_ptr[l + 1]; ++k) {
            const int c = layer_rows[k];
            if (c < 0 || c >= m) return refuse(PL_EINVAL, "layer row index out of range");
            if (seen[c])
                return refuse(PL_EINVAL, "layers must list every row exactly once (row " + std::to_string(c) + " repeats)");
            seen[c] = 1;
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
                if (mark[col_idx[e]] == l)
                    return refuse(PL_EINVAL, "two rows of layer " + std::to_string(l) + " share column " +
                                                 std::to_string(col_idx[e]));
                mark[col_idx[e]] = l;
            }
        }
    }
    // layer_ptr[n_layers] == m entries, none repeated, all in range: every row is listed.
    // max_iter == 0 evaluates no check (MSDecoder raises only once an iteration runs)
    if (csr.deg1 && max_iter > 0)
        return refuse(PL_EUNSUPPORTED, "min-sum on a degree-1 check (reference raises ValueError)");
    if (csr.maxdc >= (1 << 11)) return refuse(PL_EUNSUPPORTED, "check degree >= 2048");
    LmsGeom& g = out->geom;
    g = LmsGeom{};
    g.m = m; g.n = n; g.E = csr.E; g.max_iter = max_iter; g.early_stop = early_stop ? 1 : 0; g.maxdc = csr.maxdc;
    g.n_layers = n_layers; g.max_layer = max_layer; g.norm = norm;
    lms_geom(&g, opt.lms_global);
    std::vector<int32_t>& all = out->tables;
    all.assign(row_ptr, row_ptr + m + 1);
    all.insert(all.end(), col_idx, col_idx + csr.E);
    all.insert(all.end(), layer_ptr, layer_ptr + n_layers + 1);
    all.insert(all.end(), layer_rows, layer_rows + m);
    return {};
}

// ---- quasi-cyclic layered plans ----

// The fixed-point plan's three parameters (qc_fixed_plan_build); null for the floating-point plans.
struct QcFixedParams { int norm16, llr_max, msg_max; };
constexpr double kQcBpClipMax = 1048576.0;  // 2^20

// The checks of a quasi-cyclic layered plan, in the order the header documents, then the layer stream.
static PlanStatus qc_check_and_stream(int mb, int nb, int z, const int32_t* shift, const int32_t* layer_order,
                                      int max_iter, const QcFixedParams* fx, int* maxdc_out,
                                      std::vector<int32_t>* tables, const double* bp_clip = nullptr) {
    if (mb < 1 || nb < 1 || z < 1 || !shift) return refuse(PL_EINVAL, "mb, nb and Z must be >= 1");
    if ((int64_t)nb * z > INT32_MAX || (int64_t)mb * z > INT32_MAX)
        return refuse(PL_EINVAL, "nb Z and mb Z must fit 32 bits");
    if (max_iter < 0) return refuse(PL_EINVAL, "max_iter must be >= 0");
    int maxdc = 0;
    bool deg1 = false;
    size_t blocks = 0;
    for (int i = 0; i < mb; ++i) {
        int d = 0;
        for (int j = 0; j < nb; ++j) {
            const int s = shift[(size_t)i * nb + j];
            if (s < -1 || s >= z)
                return refuse(PL_EINVAL, "shift of block (" + std::to_string(i) + ", " + std::to_string(j) +
                                             ") outside -1 .. Z-1");
            d += s >= 0;
        }
        maxdc = std::max(maxdc, d);
        deg1 |= d == 1;
        blocks += (size_t)d;
    }
    std::vector<int32_t> order((size_t)mb);
    if (layer_order) {
        std::vector<uint8_t> seen((size_t)mb, 0);
        for (int l = 0; l < mb; ++l) {
            const int i = layer_order[l];
            if (i < 0 || i >= mb || seen[i]) return refuse(PL_EINVAL, "layer_order must be a permutation of 0 .. mb-1");
            seen[i] = 1;
            order[l] = i;
        }
    } else {
        for (int l = 0; l < mb; ++l) order[l] = l;
    }
    if (fx) {
        const auto S = [](int v) { return std::to_string(v); };
        if (fx->norm16 < 1 || fx->norm16 > 16) return refuse(PL_EINVAL, "norm16 = " + S(fx->norm16) + " outside 1 .. 16");
        if (fx->llr_max < 1 || fx->llr_max > 127)
            return refuse(PL_EINVAL, "llr_max = " + S(fx->llr_max) + " outside 1 .. 127");
        if (fx->msg_max < 1 || fx->msg_max > 127)
            return refuse(PL_EINVAL, "msg_max = " + S(fx->msg_max) + " outside 1 .. 127");
    }
    // the sum-product plan's clip (qc_bp_plan_build): finite, in (0, 2^20]; a NaN fails the first comparison
    if (bp_clip && !(*bp_clip > 0.0 && *bp_clip <= kQcBpClipMax))
        return refuse(PL_EINVAL, "clip = " + std::to_string(*bp_clip) + " outside (0, 2^20]");
    // max_iter == 0 evaluates no check, as in the layered plan
    if (deg1 && max_iter > 0)
        return refuse(PL_EUNSUPPORTED, bp_clip ? "sum-product on a degree-1 check (the box-plus of no input)"
                                               : "min-sum on a degree-1 check (reference raises ValueError)");
    if (maxdc >= (1 << 11)) return refuse(PL_EUNSUPPORTED, "check degree >= 2048");
    if (z > kQcMaxZ) return refuse(PL_EUNSUPPORTED, "Z > 1024");

    std::vector<int32_t>& t = *tables;
    t.clear();
    t.reserve(2 * (size_t)mb + 2 * blocks);
    for (int l = 0; l < mb; ++l) {
        const int i = order[l];
        const size_t at = t.size();
        t.push_back(i);
        t.push_back(0);
        for (int j = 0; j < nb; ++j) {
            const int s = shift[(size_t)i * nb + j];
            if (s >= 0) { t.push_back(j); t.push_back(s); }
        }
        t[at + 1] = (int32_t)((t.size() - at - 2) / 2);
    }
    *maxdc_out = maxdc;
    return {};
}

// The shared part of a quasi-cyclic plan's geometry: the code, the instance (dcap), and from z and
// state_bytes the frames' lanes and the state's home: the 160 KB bound on a workgroup's LDS and, for
// z <= 64, the 64 KB a wavefront's frames may take before fewer than four wavefronts share a workgroup.
static void qc_map(QcMap& g, int mb, int nb, int z, int max_iter, int early_stop, int maxdc, int mw,
                   int64_t state_bytes, bool force_global) {
    constexpr int kLdsMax = 160 * 1024;
    g.mb = mb; g.nb = nb; g.z = z; g.m = mb * z; g.n = nb * z; g.max_iter = max_iter; g.early_stop = early_stop ? 1 : 0;
    g.maxdc = maxdc; g.mw = mw; g.state_bytes = state_bytes;
    g.dcap = maxdc <= 8 ? 8 : maxdc <= 16 ? 16 : maxdc <= kQcDcapMax ? 32 : 0;
    g.subwave = g.z <= 64 ? 1 : 0;
    if (g.subwave) {
        // fpw frames side by side in a wavefront's lanes; the LDS bound of lms_geom's WAVE case, per wavefront
        g.fpw = 64 / g.z;
        const int64_t wave_state = g.state_bytes * g.fpw;
        g.use_global = (force_global || wave_state > kLdsMax) ? 1 : 0;
        g.fpb = g.use_global ? 4 : (int)std::max<int64_t>(1, std::min<int64_t>(4, 65536 / wave_state));
        g.threads = 64 * g.fpb;
        g.lds_bytes = g.use_global ? 0 : (int)(wave_state * g.fpb);
    } else {
        g.fpw = 1;
        g.fpb = 1;
        g.use_global = (force_global || g.state_bytes + kLdpcVoteBytes > kLdsMax) ? 1 : 0;
        g.threads = (g.z + 63) / 64 * 64;
        g.lds_bytes = (g.use_global ? 0 : (int)g.state_bytes) + kLdpcVoteBytes;
    }
}

PlanStatus qc_plan_build(int mb, int nb, int z, const int32_t* shift, const int32_t* layer_order, int max_iter,
                         int early_stop, double norm, const LdpcPlanOptions& opt, QcHostPlan* out) {
    int maxdc = 0;
    const PlanStatus st = qc_check_and_stream(mb, nb, z, shift, layer_order, max_iter, nullptr, &maxdc, &out->tables);
    if (st.code) return st;

    LmsGeom lg{};  // the state layout is the layered kernel's
    lg.m = mb * z; lg.n = nb * z; lg.maxdc = maxdc; lg.max_layer = z;
    lms_geom(&lg, opt.lms_global);
    QcGeom& g = out->geom;
    g = QcGeom{};
    out->f32 = opt.qc_state_elem == 4;
    g.norm = norm; g.off_mm = lg.off_mm; g.off_meta = lg.off_meta;
    int64_t state_bytes = lg.state_bytes;
    if (out->f32) {  // the same arrays with 4-byte P and minima
        g.norm = (double)(float)norm;  // rounded once, here; the kernel's (float)g.norm is exact
        g.off_mm = (int64_t)ldpc_align16((size_t)4 * lg.n);
        g.off_meta = g.off_mm + (int64_t)8 * lg.m;
        state_bytes = (int64_t)ldpc_align16((size_t)g.off_meta + (size_t)4 * lg.m * lg.mw);
    }
    qc_map(g, mb, nb, z, max_iter, early_stop, maxdc, lg.mw, state_bytes, opt.lms_global);
    return {};
}

PlanStatus qc_fixed_plan_build(int mb, int nb, int z, const int32_t* shift, const int32_t* layer_order, int max_iter,
                               int early_stop, int norm16, int llr_max, int msg_max, const LdpcPlanOptions& opt,
                               QcFixedHostPlan* out) {
    const QcFixedParams fx{norm16, llr_max, msg_max};
    int maxdc = 0;
    const PlanStatus st = qc_check_and_stream(mb, nb, z, shift, layer_order, max_iter, &fx, &maxdc, &out->tables);
    if (st.code) return st;
    QcFixedGeom& g = out->geom;
    g = QcFixedGeom{};
    g.norm16 = norm16; g.llr_max = llr_max; g.msg_max = msg_max;
    const int mw = maxdc <= kQcFixedOneWord ? 1 : 1 + (maxdc + 31) / 32;
    g.off_p = (int64_t)4 * (mb * z) * mw;
    const int64_t state_bytes = (int64_t)ldpc_align16((size_t)g.off_p + (size_t)(nb * z));
    qc_map(g, mb, nb, z, max_iter, early_stop, maxdc, mw, state_bytes, opt.lms_global);
    return {};
}

PlanStatus qc_bp_plan_build(int mb, int nb, int z, const int32_t* shift, const int32_t* layer_order, int max_iter,
                            int early_stop, double clip, const LdpcPlanOptions& opt, QcBpHostPlan* out) {
    int maxdc = 0;
    const PlanStatus st = qc_check_and_stream(mb, nb, z, shift, layer_order, max_iter, nullptr, &maxdc, &out->tables,
                                              &clip);
    if (st.code) return st;
    QcBpGeom& g = out->geom;
    g = QcBpGeom{};
    g.clip = clip;
    const size_t blocks = (out->tables.size() - 2 * (size_t)mb) / 2;  // the stream is 2 words a layer and 2 a block
    g.off_r = (int64_t)ldpc_align16((size_t)8 * ((size_t)nb * z));
    const int64_t state_bytes = (int64_t)ldpc_align16((size_t)g.off_r + (size_t)8 * z * blocks);
    qc_map(g, mb, nb, z, max_iter, early_stop, maxdc, 0, state_bytes, opt.lms_global);
    g.dcap = 0;  // the rule keeps no input in registers: the two-pass instances only
    return {};
}

// ---- quasi-cyclic encoder plans ----

PlanStatus qc_encoder_plan_build(int mb, int nb, int z, const int32_t* shift, QcEncHostPlan* out) {
    if (mb < 1 || nb < 1 || z < 1 || !shift) return refuse(PL_EINVAL, "mb, nb and Z must be >= 1");
    const int kb = nb - mb;
    if (kb < 1) return refuse(PL_EINVAL, "kb = nb - mb must be >= 1 (no message block column)");
    if ((int64_t)nb * z > INT32_MAX) return refuse(PL_EINVAL, "nb Z must fit 32 bits");
    size_t blocks = 0;
    for (int i = 0; i < mb; ++i)
        for (int j = 0; j < nb; ++j) {
            const int s = shift[(size_t)i * nb + j];
            if (s < -1 || s >= z)
                return refuse(PL_EINVAL, "shift of block (" + std::to_string(i) + ", " + std::to_string(j) +
                                             ") outside -1 .. Z-1");
            blocks += s >= 0;
        }
    if (z > kQcMaxZ) return refuse(PL_EUNSUPPORTED, "Z > 1024");

    // the structure: P(i, t) is the block of row i in parity column kb + t
    auto P = [&](int i, int t) { return shift[(size_t)i * nb + kb + t]; };
    auto row = [](int i) { return "block row " + std::to_string(i); };
    auto pcol = [](int t) { return "parity column kb+" + std::to_string(t); };
    auto ext_ok = [&](int i) {
        if (P(i, i) < 0) return false;
        for (int t = i + 1; t < mb; ++t)
            if (P(i, t) >= 0) return false;
        return true;
    };
    int f = mb - 1;
    while (f >= 0 && ext_ok(f)) --f;
    const int g = f < 0 ? 0 : f + 2;  // the last row that is no extension row is core row g - 2
    int x = 0, a = 0, b = 0;
    if (g > mb)
        return refuse(PL_EUNSUPPORTED, row(f) + " is no extension row (a diagonal block and none to its right) and "
                                           "cannot be the last but one row of a core");
    if (g == 2) return refuse(PL_EUNSUPPORTED, "a core of g = 2 block rows: g must be 0 or >= 3");
    if (g > 0) {
        for (int i = 0; i < g; ++i)
            for (int t = g; t < mb; ++t)
                if (P(i, t) >= 0) return refuse(PL_EUNSUPPORTED, "core " + row(i) + " has a block in " + pcol(t));
        int cnt = 0;
        for (int i = 0; i < g; ++i) cnt += P(i, 0) >= 0;
        if (P(0, 0) < 0 || P(g - 1, 0) < 0 || cnt != 3)
            return refuse(PL_EUNSUPPORTED, pcol(0) + " must have exactly three blocks in the core, in rows 0, x and g-1 = " +
                                               std::to_string(g - 1) + " (it has " + std::to_string(cnt) + ")");
        for (int i = 1; i < g - 1; ++i)
            if (P(i, 0) >= 0) x = i;
        a = P(0, 0);
        b = P(x, 0);
        if (P(g - 1, 0) != a)
            return refuse(PL_EUNSUPPORTED, "the first and the last block of " + pcol(0) + " must have equal shifts (" +
                                               std::to_string(a) + ", " + std::to_string(P(g - 1, 0)) + ")");
        for (int t = 1; t < g; ++t)
            for (int i = 0; i < g; ++i) {
                const bool want = i == t - 1 || i == t;
                if ((P(i, t) >= 0) != want)
                    return refuse(PL_EUNSUPPORTED, pcol(t) + " must have exactly two blocks in the core, in rows " +
                                                       std::to_string(t - 1) + " and " + std::to_string(t));
                if (want && P(i, t) != 0)
                    return refuse(PL_EUNSUPPORTED, "the dual-diagonal block (" + std::to_string(i) + ", kb+" +
                                                       std::to_string(t) + ") must have shift 0");
            }
    }

    QcEncGeom& q = out->geom;
    q = QcEncGeom{};
    q.mb = mb; q.nb = nb; q.kb = kb; q.z = z; q.k = kb * z; q.n = nb * z; q.g = g;
    const int64_t frame = (int64_t)ldpc_align16((size_t)(nb + g) * (size_t)z);
    q.subwave = z <= 64 ? 1 : 0;
    q.fpw = q.subwave ? 64 / z : 1;
    const int64_t wave = frame * q.fpw;
    if (wave > kQcEncLdsMax)
        return refuse(PL_EUNSUPPORTED, "the codeword and the core sums of a workgroup, " + std::to_string(wave) +
                                           " bytes, exceed 160 KB of LDS");
    q.fpb = q.subwave ? (int)std::max<int64_t>(1, std::min<int64_t>(4, 65536 / wave)) : 1;
    q.threads = q.subwave ? 64 * q.fpb : (z + 63) / 64 * 64;
    q.frame_bytes = (int)frame;
    q.lds_bytes = (int)(wave * q.fpb);
    out->x = x; out->a = a; out->b = b;

    std::vector<int32_t>& t = out->tables;
    t.clear();
    t.reserve(4 + 3 * (size_t)mb + 2 * blocks);
    t.insert(t.end(), {g, x, a, b});
    for (int i = 0; i < g; ++i) {
        const size_t at = t.size();
        t.push_back(0);
        for (int j = 0; j < kb; ++j) {
            const int s = shift[(size_t)i * nb + j];
            if (s >= 0) { t.push_back(j); t.push_back(s); }
        }
        t[at] = (int32_t)((t.size() - at - 1) / 2);
    }
    // parity block columns written since the last synchronisation point: behind p_0's the chain p_1 .. p_{g-1}
    std::vector<uint8_t> dirty((size_t)mb, 0);
    for (int i = 1; i < g; ++i) dirty[i] = 1;
    out->n_sync = g > 0 ? 1 : 0;
    for (int i = g; i < mb; ++i) {
        const size_t at = t.size();
        t.push_back(P(i, i));
        t.push_back(0);
        t.push_back(0);
        bool sync = false;
        for (int j = 0; j < kb + i; ++j) {
            const int s = shift[(size_t)i * nb + j];
            if (s < 0) continue;
            t.push_back(j);
            t.push_back(s);
            sync |= j >= kb && dirty[j - kb];
        }
        t[at + 1] = sync ? 1 : 0;
        t[at + 2] = (int32_t)((t.size() - at - 3) / 2);
        if (sync) {
            std::fill(dirty.begin(), dirty.end(), 0);
            ++out->n_sync;
        }
        dirty[i] = 1;
    }
    return {};
}

// ---- rate matching (include/polarldpc.h, pl_rate_match) ----
PlanStatus rate_match_check(pl_rate_match* rm) {
    if (!rm) return refuse(PL_EINVAL, "rate match is NULL");
    const auto S = [](int64_t v) { return std::to_string(v); };
    if (rm->mb < 1 || rm->nb < 1 || rm->z < 1) return refuse(PL_EINVAL, "mb, nb and Z must be >= 1");
    const int64_t z = rm->z, kb = (int64_t)rm->nb - rm->mb;
    if (kb < 1) return refuse(PL_EINVAL, "kb = nb - mb must be >= 1 (no message block column)");
    const int64_t n = (int64_t)rm->nb * z, k = kb * z;
    if (n > INT32_MAX) return refuse(PL_EINVAL, "nb Z must fit 32 bits");
    if (rm->punctured < 0 || rm->punctured >= kb)
        return refuse(PL_EINVAL, "punctured = " + S(rm->punctured) + " outside 0 .. kb-1 = " + S(kb - 1));
    const int64_t P = (int64_t)rm->punctured * z, F = rm->fillers;
    if (F < 0 || F > k - P) return refuse(PL_EINVAL, "fillers = " + S(F) + " outside 0 .. k - P = " + S(k - P));
    const int64_t ncb = rm->ncb < 0 ? n - P : rm->ncb;
    if (ncb < k - P || ncb > n - P)
        return refuse(PL_EINVAL, "ncb = " + S(ncb) + " outside k - P = " + S(k - P) + " .. n - P = " + S(n - P));
    if (rm->start < 0 || rm->start >= ncb)
        return refuse(PL_EINVAL, "start = " + S(rm->start) + " outside 0 .. ncb-1 = " + S(ncb - 1));
    if (rm->E < 1) return refuse(PL_EINVAL, "E = " + S(rm->E) + " must be >= 1");
    const int64_t M = ncb - F;
    if (M < 1) return refuse(PL_EINVAL, "M = ncb - fillers = " + S(M) + " must be >= 1 (nothing to transmit)");
    const int64_t lo = k - P - F;  // buffer positions lo .. lo+F-1 are the fillers
    const int64_t start = rm->start, E = rm->E;
    const int64_t c0 = start < lo ? start : start >= lo + F ? start - F : lo % M;
    // compact indices c0 .. c0+E-1 mod M: the largest one, then its codeword position
    const int64_t cmax = c0 + E - 1 < M ? c0 + E - 1 : M - 1;
    rm->ncb = (int32_t)ncb;
    rm->n = (int32_t)n; rm->k = (int32_t)k; rm->P = (int32_t)P; rm->M = (int32_t)M; rm->c0 = (int32_t)c0;
    rm->hi = (int32_t)(P + (cmax < lo ? cmax : cmax + F));
    rm->max_reps = (int32_t)((E + M - 1) / M);
    return {};
}

}  // namespace pl

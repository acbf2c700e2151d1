// Host-side planning of the LDPC decoders: argument checks, kernel selection,
// LDS budgets and the device tables, as plain data.  No HIP here, neither in
// this header nor in ldpc_plan.cpp: the C-ABI (capi.cpp) uploads what the
// planner returns, and the planner is testable on a machine without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/polarldpc.h"  // pl_rate_match

namespace pl {

// ---- kernel arguments (field order and types are the kernels' ABI) ----
struct LdpcGeom {
    int m, n, E, max_iter, early_stop, algo, maxdc, maxdv;
    double norm;
    int threads;       // threads per workgroup (one frame per workgroup)
    int lds_bytes;     // 0 => messages live in the global workspace
    int use_global;
    int check_kernel;  // 1: ldpc_check_kernel (thread per check, state in LDS)
    int reg_variant;   // > 0: ldpc_reg_kernel instance (constant variable degree, LDS state)
    int compact;       // 1: ldpc_ms_compact_kernel (min-sum, compressed check state in LDS)
    int regular;       // every check has degree maxdc and every variable degree maxdv
    int grp;           // BP reg variant: ldpc_bp_grp_kernel (degree-grouped products, padded T'/C')
    int tl;            // grp: length of the padded T'/C' arrays (doubles)
    int npad;          // grp: pad positions listed after the variable slots (a multiple of 256, -1 filled)
    int ms36;          // > 0: ldpc_ms36_kernel<ms36> ((3,6)-regular min-sum, n = 1024 ms36)
    int fpg;           // grp: frames per workgroup (1 or 2)
};
struct LdpcDev {
    const int32_t* row_ptr;   // [m+1]
    const int32_t* col_idx;   // [E]   (check-major edge -> variable)
    const int32_t* edge_chk;  // [E]   edge -> check
    const int32_t* var_ptr;   // [n+1]
    const int32_t* var_edge;  // [E]   var-major list of check-major edge ids (ascending check)
    const int32_t* edge_meta; // [E]   first edge of the edge's check | check degree << 20
    const int32_t* var_chk;   // [E]   check of var_edge[k]
    const int32_t* var_cp;    // [E]   check << 4 | position in the check, of var_edge[k]
    // grp (ldpc_bp_grp_kernel): per edge slot (256 EPT of them) the T' position
    // of the edge's check | position in the check << 16 | its slot's D_s << 20;
    // per variable slot q (256 VPT of them): [q][DV] T' positions, [q][DV]
    // checks, then [q] the variable (-1: none); then npad pad positions
    const int32_t* grp_meta;  // [256 EPT]
    const int32_t* var_tpos;  // [256 VPT (2 DV + 1)]
    // ms36 (ldpc_ms36_kernel), 16-byte aligned: per variable [8] u32, its three
    // edge words (LDS rec address of the check | 3 * position) then the three
    // LDS meta addresses, in the reference's np.sum order (ascending check);
    // then per check [4] u32, the LDS addresses 8v of its six variables, two per word
    const uint32_t* ms_vw;    // [n][8] + [m][4]
};
struct LmsGeom {
    int m, n, E, max_iter, early_stop, maxdc;
    int n_layers, max_layer;  // layers and the checks of the largest one
    double norm;
    int mw;                   // meta words per check (1: every degree <= 16)
    int wave;                 // 1: one wavefront per frame (max_layer <= 64); 0: one workgroup per frame
    int use_global;           // state in the workspace instead of LDS
    int fpb;                  // frames per workgroup
    int threads, lds_bytes;
    int64_t state_bytes;      // per frame: P[n] f64, then at off_mm [m] double2, at off_meta [m][mw] u32
    int64_t off_mm, off_meta;
};
struct LmsDev {
    const int32_t* row_ptr;     // [m+1]  H as given (original row order)
    const int32_t* col_idx;     // [E]
    const int32_t* layer_ptr;   // [n_layers+1]
    const int32_t* layer_rows;  // [m]    rows layer by layer
};

// ---- (DV, EPT, VPT) instances of ldpc_reg_kernel / ldpc_bp_grp_kernel: E <=
// 256 EPT, n <= 256 VPT.  LdpcGeom::reg_variant is the index + 1; ldpc.hip builds
// its kernel-pointer table from this array.  E = DV n for a constant variable
// degree, so (3, 8, 2) and (3, 16, 4) could never be picked ahead of (3, 6, 2) /
// (3, 12, 4): not built
struct LdpcRegVariant { int dv, ept, vpt; };
constexpr LdpcRegVariant kLdpcRegVariants[] = {{3, 6, 2}, {3, 12, 4}, {4, 8, 2}, {4, 16, 4}};
constexpr int kLdpcRegVariantCount = (int)(sizeof(kLdpcRegVariants) / sizeof(kLdpcRegVariants[0]));
constexpr int ldpc_reg_variant(int dv, int E, int n) {  // 0: none fits
    for (int i = 0; i < kLdpcRegVariantCount; ++i)
        if (kLdpcRegVariants[i].dv == dv && E <= 256 * kLdpcRegVariants[i].ept && n <= 256 * kLdpcRegVariants[i].vpt)
            return i + 1;
    return 0;
}

// ---- LDS budgets, one formula per kernel (the kernels carve their dynamic LDS
// in this order; each names its function here) ----
constexpr size_t ldpc_align16(size_t b) { return (b + 15) & ~(size_t)15; }
constexpr int kLdpcVoteBytes = 128;  // wg_any's words [2][16] u32 (common.hpp), the last bytes of the LDS
// ldpc_decode_kernel: syndrome [2][m] u32 + decisions [n] u8, behind T[E], C[E] f64 unless those are global
constexpr size_t ldpc_small_lds(int m, int n) { return (size_t)8 * m + n; }
constexpr size_t ldpc_generic_lds(int E, int m, int n) { return (size_t)2 * (size_t)E * 8 + ldpc_small_lds(m, n); }
constexpr size_t kLdpcGenericLdsMax = 64 * 1024;  // above: T, C in the workspace, or a compact kernel
// ldpc_reg_kernel: the generic layout, the BP tanh lists (u16 [256 VPT DV]), the vote words
constexpr size_t ldpc_reg_list_bytes(int variant) {
    return (size_t)256 * kLdpcRegVariants[variant - 1].vpt * kLdpcRegVariants[variant - 1].dv * 2;
}
constexpr size_t ldpc_reg_lds(int E, int m, int n, int variant) {
    return ldpc_align16(ldpc_align16(ldpc_generic_lds(E, m, n)) + ldpc_reg_list_bytes(variant)) + kLdpcVoteBytes;
}
// ldpc_bp_grp_kernel: T'[tl], C'[tl] f64, syndrome [m rounded up to 4] u32, the tanh lists
constexpr size_t ldpc_grp_lds(int tl, int m, int variant) {
    return ldpc_align16(ldpc_align16((size_t)16 * tl + (size_t)4 * ((m + 3) & ~3)) + ldpc_reg_list_bytes(variant));
}
// ldpc_ms_compact_kernel: total [n] f64, per check (min1, min2) f64 + meta u32, the vote words
constexpr size_t ldpc_compact_lds(int m, int n) {
    return ldpc_align16(ldpc_align16((size_t)8 * n) + (size_t)20 * m) + kLdpcVoteBytes;
}
constexpr size_t kLdpcCompactLdsMax = 160 * 1024;
// ldpc_ms36_kernel<n / 1024> (static LDS): total [n] f64 at 0, check records [m] 16 B at
// ldpc_ms36_rec, meta [m] u32 at ldpc_ms36_meta, the vote words; 0: no instance for this n
constexpr uint32_t ldpc_ms36_rec(int n) { return 8u * (uint32_t)n; }
constexpr uint32_t ldpc_ms36_meta(int n) { return 16u * (uint32_t)n; }
constexpr int ldpc_ms36_lds(int n) { return (n == 2048 || n == 4096 || n == 8192) ? 18 * n + kLdpcVoteBytes : 0; }
// ldpc_check_kernel (diagnostic): C[E], T[E], tot[n] f64
constexpr size_t ldpc_check_lds(int E, int n) { return ldpc_align16((size_t)(2 * (size_t)E + n) * 8); }
// ldpc_decode_kernel<.., GLOBAL>: T[E], C[E] f64 per frame of the workspace
inline size_t ldpc_work_bytes_per_frame(const LdpcGeom& g) {
    return g.use_global ? (size_t)(2 * (size_t)g.E) * sizeof(double) : 0;
}
// what pl_plan_get_info reports in `reserved` (include/polarldpc.h)
inline int ldpc_kernel_code(const LdpcGeom& g) {
    return g.ms36 ? 8 : g.compact ? 5 : (g.check_kernel ? 3 : (g.grp ? 7 : (g.reg_variant ? 2 : 1)));
}
inline int lms_kernel_code(const LmsGeom& g) { return g.use_global ? 10 : 9; }

// ---- planner ----
struct PlanStatus {
    int code = 0;  // PL_OK or a PL_E* code of include/polarldpc.h
    std::string msg;
};

// H in CSR form: non-null pointers, row_ptr[0] == 0, E = row_ptr[m] >= 0 and
// every row_ptr[c+1] in [row_ptr[c], E] before any col_idx entry is read; then
// columns in [0, n), ascending within a row.
struct CsrInfo {
    int E = 0, maxdc = 0;
    bool deg1 = false;  // a row of degree 1 exists
};
PlanStatus csr_validate(int m, int n, const int32_t* row_ptr, const int32_t* col_idx, CsrInfo* info);

// The environment's planning switches, read once by capi.cpp (the planner calls no getenv).
enum LdpcKernelOverride {  // PL_LDPC_KERNEL
    kLdpcKernelDefault = 0,
    kLdpcKernelGeneric,  // ldpc_decode_kernel for every code
    kLdpcKernelReg,      // BP keeps ldpc_reg_kernel's per-lane products (no ldpc_bp_grp_kernel)
    kLdpcKernelCompact,  // (3,6) min-sum keeps ldpc_ms_compact_kernel (no ldpc_ms36_kernel)
    kLdpcKernelCheck,    // ldpc_check_kernel (capi.cpp passes it in the diagnostic build only)
};
struct LdpcPlanOptions {
    int kernel = kLdpcKernelDefault;
    int bp_fpg = 0;           // PL_BP_FPG: frames per workgroup of ldpc_bp_grp_kernel, 1 or 2; 0: the variant's default
    bool lms_global = false;  // PL_LMS_GLOBAL: layered state in the workspace
    int qc_state_elem = 8;    // qc_plan_build: bytes of a state element, 8 (fp64) or 4 (PL_LDPC_QC_F32)
};

// Element offsets of LdpcDev's members in LdpcHostPlan::tables.
struct LdpcDevAt {
    size_t row_ptr, col_idx, edge_chk, var_ptr, var_edge, edge_meta, var_chk, var_cp;
    size_t grp_meta, var_tpos;  // used when geom.grp
    size_t ms_vw;               // a multiple of 4 (uint4 loads); used when geom.ms36
};
struct LdpcHostPlan {
    LdpcGeom geom{};
    std::vector<int32_t> tables;  // one device buffer
    LdpcDevAt at{};
    LdpcDev dev(const int32_t* base) const {
        return {base + at.row_ptr, base + at.col_idx, base + at.edge_chk, base + at.var_ptr, base + at.var_edge,
                base + at.edge_meta, base + at.var_chk, base + at.var_cp,
                geom.grp ? base + at.grp_meta : nullptr, geom.grp ? base + at.var_tpos : nullptr,
                geom.ms36 ? reinterpret_cast<const uint32_t*>(base + at.ms_vw) : nullptr};
    }
};
// Flooding BP / min-sum plan (pl_ldpc_plan_create's arguments).
PlanStatus ldpc_plan_build(int m, int n, const int32_t* row_ptr, const int32_t* col_idx, int algo, int max_iter,
                           int early_stop, double norm, const LdpcPlanOptions& opt, LdpcHostPlan* out);

struct LmsHostPlan {
    LmsGeom geom{};
    std::vector<int32_t> tables;  // row_ptr, col_idx, layer_ptr, layer_rows as given
    LmsDev dev(const int32_t* base) const {
        const int32_t* col = base + (geom.m + 1);
        return {base, col, col + geom.E, col + geom.E + (geom.n_layers + 1)};
    }
};
// Mapping and state layout of ldpc_layered_kernel for the code described by
// the fields already set (m, n, maxdc, max_layer).
void lms_geom(LmsGeom* g, bool force_global);
// Layered min-sum plan (pl_ldpc_layered_plan_create's arguments).
PlanStatus lms_plan_build(int m, int n, const int32_t* row_ptr, const int32_t* col_idx, int n_layers,
                          const int32_t* layer_ptr, const int32_t* layer_rows, int max_iter, int early_stop,
                          double norm, const LdpcPlanOptions& opt, LmsHostPlan* out);

// ---- quasi-cyclic layered min-sum: the code and its mapping (ldpc_qc_frame.hpp) ----
// H is mb x nb blocks of z x z, each zero or a cyclically shifted identity; a
// block row is a layer.  What qc_frame_kernel reads whatever the arithmetic; the
// geometry of a decoder is this and its own state layout.
struct QcMap {
    int mb, nb, z, m, n, max_iter, early_stop, maxdc;
    int64_t state_bytes;  // per frame
    int mw;          // u32 words of a check's state next to its minima (QcGeom) or in all (QcFixedGeom)
    int dcap;        // inputs of a check kept in registers: 8, 16 or 32 (>= maxdc); 0: two-pass form
    int subwave;     // 1 (z <= 64): fpw frames share a wavefront; 0: one workgroup per frame
    int use_global;  // state in the workspace instead of LDS
    int fpw;         // frames per wavefront (64 / z; 1 when !subwave)
    int fpb;         // wavefronts per workgroup when subwave, else 1: a workgroup decodes fpw fpb frames
    int threads, lds_bytes;
};
constexpr int kQcMaxZ = 1024;
constexpr int kQcDcapMax = 32;  // largest register-resident instance of qc_frame_kernel

// ---- floating-point quasi-cyclic layered min-sum (ldpc_qc_layered.hip) ----
// State layout per frame: lms_geom's (mw meta words per check, as LmsGeom::mw); with f32 the same
// arrays in single precision: P[n] f32, at off_mm = align16(4 n) [m] float2, at
// off_meta = off_mm + 8 m the same [m][mw] u32, state_bytes = align16(off_meta + 4 m mw).
struct QcGeom : QcMap {
    double norm;  // a single-precision plan: (float)normalization, rounded by the planner (exact as a float)
    int64_t off_mm, off_meta;
};
inline int qc_kernel_code(const QcGeom& g, bool f32 = false) { return (g.use_global ? 12 : 11) + (f32 ? 2 : 0); }
struct QcHostPlan {
    QcGeom geom{};
    bool f32 = false;  // state and arithmetic in binary32: the float instances of qc_frame_kernel
    // per layer, in layer order: block row, its degree d, then d (block column, shift) pairs by
    // ascending block column -- a stream the kernel walks front to back, 2 + 2 d words a layer
    std::vector<int32_t> tables;
};
// Quasi-cyclic layered min-sum plan (pl_ldpc_qc_plan_create's arguments); shift [mb][nb]
// row-major, -1 a zero block; layer_order [mb] a permutation of the block rows, or null (0 .. mb-1).
PlanStatus qc_plan_build(int mb, int nb, int z, const int32_t* shift, const int32_t* layer_order, int max_iter,
                         int early_stop, double norm, const LdpcPlanOptions& opt, QcHostPlan* out);

// ---- int8 fixed-point quasi-cyclic layered min-sum (ldpc_qc_fixed.hip) ----
// The definition: include/polarldpc.h, pl_ldpc_qc_fixed_plan_create.  Mapping and layer stream are
// qc_plan_build's.  State layout per frame, all of it in LDS or all of it in the frame's workspace slice:
//   at 0      [m][mw] u32 per check.  s1 = min(msg_max, min1 norm16 >> 4) and s2 likewise of min2, the two
//             smallest |q| of the check; idx1 the position of min1 (the first one on a tie).
//             maxdc <= 14, mw = 1: s1 bits 0-6, s2 bits 7-13, idx1 bits 14-17, the negative flags bits
//               18-31 (position j at bit 18 + j); the parity of the negative inputs is their popcount
//             maxdc > 14, mw = 1 + ceil(maxdc / 32): word 0 = s1 bits 0-7, s2 bits 8-15, idx1 bits 16-26,
//               the parity bit 27; words 1 ..: the negative flags, position j at bit j % 32 of word 1 + j / 32
//   at off_p = 4 m mw   P[n] int8
//   state_bytes = align16(off_p + n): n + 4 m rounded up to 16 for degrees <= 14, n + 8 m up to 32.
struct QcFixedGeom : QcMap {       // mw: 1 (maxdc <= kQcFixedOneWord) or 1 + ceil(maxdc / 32)
    int norm16, llr_max, msg_max;  // the normalisation in sixteenths and the two saturation bounds
    int64_t off_p;
};
constexpr int kQcFixedOneWord = 14;  // 7 + 7 bits of minima, 4 of idx1 and 14 flags fill a word
inline int qc_fixed_kernel_code(const QcFixedGeom& g) { return g.use_global ? 16 : 15; }
struct QcFixedHostPlan {
    QcFixedGeom geom{};
    std::vector<int32_t> tables;  // QcHostPlan::tables: the same stream for the same base matrix
};
// pl_ldpc_qc_fixed_plan_create's arguments.  qc_plan_build's checks in its order, with norm16 in 1 .. 16,
// llr_max in 1 .. 127 and msg_max in 1 .. 127 (PL_EINVAL, in this order) behind the layer_order check
// and in front of the PL_EUNSUPPORTED ones.
PlanStatus qc_fixed_plan_build(int mb, int nb, int z, const int32_t* shift, const int32_t* layer_order, int max_iter,
                               int early_stop, int norm16, int llr_max, int msg_max, const LdpcPlanOptions& opt,
                               QcFixedHostPlan* out);

// ---- fp64 quasi-cyclic layered sum-product (ldpc_qc_bp.hip) ----
// The definition: include/polarldpc.h, pl_ldpc_qc_bp_plan_create.  Mapping and layer stream are
// qc_plan_build's.  State per frame, all of it in LDS or all of it in the frame's workspace slice:
//   at 0      P[n] f64
//   at off_r = align16(8 n)   R as [blocks][z] f64: edge j of a layer is slot (blocks of the earlier
//             layers of the stream) + j, its check r element slot z + r -- consecutive lanes,
//             consecutive doubles
//   state_bytes = align16(off_r + 8 z blocks)
struct QcBpGeom : QcMap {  // mw: 0 (no check words); dcap: 0 (the rule keeps no input in registers)
    double clip;           // the clamp of P on load and of every q
    int64_t off_r;
};
inline int qc_bp_kernel_code(const QcBpGeom& g) { return g.use_global ? 18 : 17; }
struct QcBpHostPlan {
    QcBpGeom geom{};
    std::vector<int32_t> tables;  // QcHostPlan::tables: the same stream for the same base matrix
};
// pl_ldpc_qc_bp_plan_create's arguments.  qc_plan_build's checks in its order, with clip finite and in
// (0, 2^20] (PL_EINVAL) behind the layer_order check and in front of the PL_EUNSUPPORTED ones.
PlanStatus qc_bp_plan_build(int mb, int nb, int z, const int32_t* shift, const int32_t* layer_order, int max_iter,
                            int early_stop, double clip, const LdpcPlanOptions& opt, QcBpHostPlan* out);

// ---- quasi-cyclic encoder from the base matrix (ldpc_qc_encode.hip) ----
// The supported structure and the encoding steps: include/polarldpc.h,
// pl_ldpc_qc_encoder_create.  kb = nb - mb message block columns, then mb parity
// block columns: a core of g block rows (g == 0 or g >= 3) and a lower-triangular
// extension.  Per frame the LDS holds the codeword, one byte per bit, and behind it
// the g vectors lambda_t: (nb + g) z bytes, rounded up to 16.
struct QcEncGeom {
    int mb, nb, kb, z, k, n;
    int g;            // core block rows
    int subwave;      // 1 (z <= 64): fpw frames share a wavefront; 0: one workgroup per frame
    int fpw;          // frames per wavefront (64 / z; 1 when !subwave)
    int fpb;          // wavefronts per workgroup when subwave, else 1: a workgroup encodes fpw fpb frames
    int threads;
    int frame_bytes;  // LDS bytes of a frame: align16((nb + g) z)
    int lds_bytes;    // fpw fpb frame_bytes
};
constexpr int kQcEncLdsMax = 160 * 1024;
struct QcEncHostPlan {
    QcEncGeom geom{};
    int x = 0, a = 0, b = 0;  // the core's middle row of parity column kb and its shifts (0 when g == 0)
    int n_sync = 0;           // synchronisation points the stream asks for: the one behind p_0 (g > 0)
                              // and one per extension row whose sync flag is set
    // One stream, walked front to back at wave-uniform addresses:
    //   g, x, a, b
    //   per core row t = 0 .. g-1:     d, then d (block column, shift) pairs -- its message blocks
    //                                  (block column < kb), ascending block column
    //   per extension row i = g .. mb-1: the diagonal shift d_i, the sync flag, d, then d (block column,
    //                                  shift) pairs -- its blocks left of the diagonal (block column <
    //                                  kb + i, message or parity), ascending block column
    // The sync flag is 1 iff the row reads a parity block column written since the last
    // synchronisation point; the kernel synchronises before such a row and nowhere else in the
    // extension.  4 + g + 3 (mb - g) + 2 (blocks in the stream) words.
    std::vector<int32_t> tables;
};
// Encoder plan for the base matrix shift [mb][nb] (row-major, -1 a zero block): pl_ldpc_qc_encoder_create's
// checks.  PL_EINVAL: mb, nb or z < 1, kb = nb - mb < 1, nb z beyond int32, a shift outside -1 .. z-1;
// PL_EUNSUPPORTED: z > kQcMaxZ, a parity part outside the structure (the message names the first rule
// violated), a workgroup's LDS above kQcEncLdsMax.
PlanStatus qc_encoder_plan_build(int mb, int nb, int z, const int32_t* shift, QcEncHostPlan* out);

// ---- rate matching of quasi-cyclic codes (ldpc_qc_ratematch.hip) ----
// The definition: include/polarldpc.h, pl_rate_match.  The struct is plain data and the kernels' argument
// (passed by value): no table, no device object.  rate_match_check validates the parameters in the
// header's order (PL_EINVAL, the message names the first condition violated) and fills n, k, P, M, c0,
// hi and max_reps; a negative ncb becomes n - P.
PlanStatus rate_match_check(pl_rate_match* rm);

// 64-bit FNV-1a over a table vector's bytes (the pl_debug_*_plan_probe digests)
uint64_t plan_tables_digest(const std::vector<int32_t>& tables);

}  // namespace pl

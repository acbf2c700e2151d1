// Layered sum-product (belief propagation) for quasi-cyclic LDPC codes on gfx950
// (MI355X), fp64.  The definition (the clamp, the box-plus and its order of
// operations, the forward / backward recursion of a check):
// include/polarldpc.h, pl_ldpc_qc_bp_plan_create.  Every operation is one IEEE
// binary64 operation (-ffp-contract=off), expm1 and log1p are glibc's bit for bit
// (libm_exact.hpp), so bits, iteration counts and posteriors equal a NumPy
// restatement exactly.
// The kernel, its mapping and its synchronisation: ldpc_qc_frame.hpp; this file
// is its sum-product rule.
// State per frame (ldpc_plan.hpp, QcBpGeom):
//   at 0      P[n] f64
//   at off_r  R as [blocks][z] f64: edge j of a layer is slot e0 + j, e0 the blocks
//             of the earlier layers of the stream; check r is element slot z + r
// The update keeps no array of a check's inputs: the first pass leaves q_j in
// P[v_j] (the checks of a layer share no variable) and the forward value F_j in
// R's slot j (R_j is dead once q_j exists); the second walks back with one
// running B.  So one instance serves every degree up to 2047, and DCAP is unused:
// only the DCAP = 0 instances are compiled.
#include "ldpc_qc_frame.hpp"
#include "libm_exact.hpp"

namespace pl {

PL_DEV double qb_clamp(double x, double clip) {
    if (x != x) return 0.0;
    return x > clip ? clip : (x < -clip ? -clip : x);
}

// log1p(expm1(-|t|) + 1.0): the correction term ln(1 + e^-|t|) of the box-plus
PL_DEV double qb_corr(double t) { return libm_log1p_pos(libm_expm1(-fabs(t)) + 1.0); }

PL_DEV double qb_boxplus(double a, double b) {
    const double aa = fabs(a), ab = fabs(b);
    const double m = ab < aa ? ab : aa;
    const double s = ((a < 0.0) != (b < 0.0)) ? -m : m;
    const double cp = qb_corr(a + b);
    const double cm = qb_corr(a - b);
    return s + (cp - cm);
}

struct QcBpRule {
    using Geom = QcBpGeom;
    using IO = double;
    using Elem = double;
    static constexpr bool kEdgeOffset = true;
    double* P;
    double* R;
    PL_DEV QcBpRule(const QcBpGeom& g, unsigned char* base)
        : P(reinterpret_cast<double*>(base)), R(reinterpret_cast<double*>(base + g.off_r)) {}
    static PL_DEV double load(const QcBpGeom& g, double x) { return qb_clamp(x, g.clip); }
    // One layered update of check r of a block row of degree d >= 2; pr: its d (block column, shift)
    // pairs; e0: the layer's first slot of R.  first: R holds nothing yet (R = +0.0).
    template <int DCAP>
    PL_DEV void update(const QcBpGeom& g, const int32_t* __restrict__ pr, int d, int r, int, bool first, int e0) const {
        const size_t z = (size_t)g.z;
        double* const Rc = R + (size_t)e0 * z + (size_t)r;  // slot j: Rc[j z]
        const double clip = g.clip;
        // forward: q_j into P[v_j], F_j into slot j (j <= d-2); slot d-1 keeps its R until the second pass
        double F = 0.0, q = 0.0;
        for (int j = 0; j < d; ++j) {
            const int v = qc_var(pr[2 * j], pr[2 * j + 1], r, g.z);
            const double p = P[v];
            q = qb_clamp(first ? p : p - Rc[(size_t)j * z], clip);
            P[v] = q;
            if (j < d - 1) {
                F = j == 0 ? q : qb_boxplus(F, q);
                Rc[(size_t)j * z] = F;
            }
        }
        // backward: R'_(d-1) = F_(d-2); B runs from q_(d-1) down; R'_j = boxplus(F_(j-1), B_(j+1)); R'_0 = B_1
        {
            const int v = qc_var(pr[2 * (d - 1)], pr[2 * (d - 1) + 1], r, g.z);
            P[v] = q + F;
            Rc[(size_t)(d - 1) * z] = F;
        }
        double B = q;
        for (int j = d - 2; j >= 1; --j) {
            const int v = qc_var(pr[2 * j], pr[2 * j + 1], r, g.z);
            const double qj = P[v];
            const double rn = qb_boxplus(Rc[(size_t)(j - 1) * z], B);
            B = qb_boxplus(qj, B);
            P[v] = qj + rn;
            Rc[(size_t)j * z] = rn;
        }
        {
            const int v = qc_var(pr[0], pr[1], r, g.z);
            P[v] = P[v] + B;
            Rc[0] = B;
        }
    }
};

// the rule ignores DCAP: one instance per (mapping, state home)
template <>
void* qc_frame_pick<QcBpRule>(const QcMap& g) { return qc_frame_pick_at<QcBpRule, 0>(g); }

hipError_t qc_prepare(const QcBpGeom& g) { return qc_frame_prepare<QcBpRule>(g); }

hipError_t qc_launch(const QcBpGeom& g, const int32_t* tab, const double* llr, int64_t ld, uint8_t* bits,
                     int32_t* iters, double* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s) {
    return qc_frame_launch<QcBpRule>(g, tab, llr, ld, bits, iters, post, ld_post, batch, work, s);
}

}  // namespace pl

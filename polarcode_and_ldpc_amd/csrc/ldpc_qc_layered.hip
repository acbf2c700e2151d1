// Layered normalised min-sum for quasi-cyclic LDPC codes on gfx950 (MI355X).
// H is mb x nb blocks of Z x Z, each zero or an identity shifted cyclically by
// s: H[i Z + r, j Z + (r + s) % Z] = 1.  Build-defined, as ldpc_layered.hip,
// and by definition equal to that decoder on the expanded H with the block rows
// as layers: the check state, its packing and the rule are ldpc_lms_check.hpp's
// text, the position of an input in its check is the rank of its block column
// among the row's non-zero blocks (its CSR position).
//
// What the structure buys over ldpc_layered_kernel: no row_ptr / col_idx /
// layer_rows, and the variable of check r is col Z + (r + s >= Z ? r + s - Z :
// r + s): consecutive lanes, consecutive P.  The kernel, its mapping and its
// synchronisation: ldpc_qc_frame.hpp; this file is its floating-point rule.
// State per frame as ldpc_layered.hip (P[n], double2 minima and mw meta words
// per check).
// Single precision (PL_LDPC_QC_F32): the same text instantiated with T = float
// -- P[n] float, float2 minima, the same meta words -- every operation one IEEE
// binary32 operation (no FMA contraction: -ffp-contract=off; no double in the
// arithmetic; subnormals kept: the default denormal mode), so the results equal
// a NumPy float32 restatement bit for bit.  The T = double instances are the
// code they were before T existed.
#include "ldpc_qc_frame.hpp"

namespace pl {

// One layered update of check r of a block row of degree d >= 2; pr: its d
// (block column, shift) pairs.  DCAP > 0 requires d <= DCAP <= 32, so the
// negative flags of a check are one word.  norm: the normalisation in the state
// type (the rule converts it once, at entry).
template <typename T, int DCAP>
PL_DEV void qc_check_update(const QcGeom& g, const int32_t* __restrict__ pr, int d, int r, T* P,
                            typename LmsNum<T>::Pair* mmp, uint32_t* mw, bool first, T norm) {
    using Num = LmsNum<T>;
    const bool small = g.mw == 1;
    LmsCheckT<T> old{};
    uint32_t w0 = 0;
    if (!first) {
        const typename Num::Pair mm = *mmp;
        old.min1 = mm.x; old.min2 = mm.y;
        w0 = mw[0];
        lms_unpack(w0, small, old);
    }
    LmsCheckT<T> nw{};
    nw.min1 = Num::inf(); nw.min2 = Num::inf();
    if constexpr (DCAP > 0) {
        const uint32_t negw = first ? 0u : (small ? (w0 >> 16) : mw[1]);
        T q[DCAP];
#pragma unroll
        for (int j = 0; j < DCAP; ++j) {
            q[j] = T(0);
            if (j < d) {
                const T p = P[qc_var(pr[2 * j], pr[2 * j + 1], r, g.z)];
                const T rr = first ? T(0) : lms_c2v(old, (negw >> j) & 1u, (uint32_t)j, norm);
                q[j] = p - rr;
                if (__builtin_isnan(q[j])) {
                    if (nw.ncnt == 0u) nw.nidx = (uint32_t)j;
                    nw.ncnt = nw.ncnt < 2u ? nw.ncnt + 1u : 2u;
                } else {
                    const T a = Num::abs(q[j]);
                    if (a < nw.min1) { nw.min2 = nw.min1; nw.min1 = a; nw.idx1 = (uint32_t)j; }
                    else if (a < nw.min2) nw.min2 = a;
                }
                if (q[j] == T(0)) nw.zcnt = nw.zcnt < 2u ? nw.zcnt + 1u : 2u;
                if (q[j] < T(0)) nw.par ^= 1u;
            }
        }
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < DCAP; ++j) {
            if (j < d) {
                const uint32_t nb = q[j] < T(0) ? 1u : 0u;
                P[qc_var(pr[2 * j], pr[2 * j + 1], r, g.z)] = q[j] + lms_c2v(nw, nb, (uint32_t)j, norm);
                acc |= nb << j;
            }
        }
        *mmp = Num::pair(nw.min1, nw.min2);
        if (small) {
            mw[0] = lms_pack(nw, true, acc);
        } else {
            mw[1] = acc;
            mw[0] = lms_pack(nw, false, 0u);
        }
    } else {
        uint32_t negw = small ? (w0 >> 16) : 0u;
        for (int j = 0; j < d; ++j) {
            if (!small && !first && (j & 31) == 0) negw = mw[1 + (j >> 5)];
            const T p = P[qc_var(pr[2 * j], pr[2 * j + 1], r, g.z)];
            const T rr = first ? T(0) : lms_c2v(old, (negw >> (j & 31)) & 1u, (uint32_t)j, norm);
            const T q = p - rr;
            if (__builtin_isnan(q)) {
                if (nw.ncnt == 0u) nw.nidx = (uint32_t)j;
                nw.ncnt = nw.ncnt < 2u ? nw.ncnt + 1u : 2u;
            } else {
                const T a = Num::abs(q);
                if (a < nw.min1) { nw.min2 = nw.min1; nw.min1 = a; nw.idx1 = (uint32_t)j; }
                else if (a < nw.min2) nw.min2 = a;
            }
            if (q == T(0)) nw.zcnt = nw.zcnt < 2u ? nw.zcnt + 1u : 2u;
            if (q < T(0)) nw.par ^= 1u;
        }
        uint32_t acc = 0;
        negw = small ? (w0 >> 16) : 0u;
        for (int j = 0; j < d; ++j) {
            if (!small && !first && (j & 31) == 0) negw = mw[1 + (j >> 5)];
            const int v = qc_var(pr[2 * j], pr[2 * j + 1], r, g.z);
            const T p = P[v];
            const T rr = first ? T(0) : lms_c2v(old, (negw >> (j & 31)) & 1u, (uint32_t)j, norm);
            const T q = p - rr;
            const uint32_t nb = q < T(0) ? 1u : 0u;
            P[v] = q + lms_c2v(nw, nb, (uint32_t)j, norm);
            acc |= nb << (j & 31);
            if (!small && ((j & 31) == 31 || j == d - 1)) { mw[1 + (j >> 5)] = acc; acc = 0; }
        }
        *mmp = Num::pair(nw.min1, nw.min2);
        mw[0] = lms_pack(nw, small, acc);
    }
}


// T: the state and arithmetic type; IO: the type of llr and post.  <double, double> is the fp64
// decoder; <float, float> and <float, double> are the binary32 decoder (PL_LDPC_QC_F32 plans), the second
// rounding each LLR to nearest even on load and widening the posteriors on store (exact).
template <typename T, typename IO_>
struct QcFloatRule {
    using Geom = QcGeom;
    using IO = IO_;
    using Elem = T;
    T* P;
    typename LmsNum<T>::Pair* MM;
    uint32_t* META;
    // a single-precision plan's g.norm already holds a float's value (qc_plan_build rounds it once), so this
    // one conversion is exact and no double is left in the float instances' iteration loop
    T norm;
    PL_DEV QcFloatRule(const QcGeom& g, unsigned char* base)
        : P(reinterpret_cast<T*>(base)), MM(reinterpret_cast<typename LmsNum<T>::Pair*>(base + g.off_mm)),
          META(reinterpret_cast<uint32_t*>(base + g.off_meta)), norm((T)g.norm) {}
    static PL_DEV T load(const QcGeom&, IO x) { return (T)x; }
    template <int DCAP>
    PL_DEV void update(const QcGeom& g, const int32_t* __restrict__ pr, int d, int r, int c, bool first) const {
        qc_check_update<T, DCAP>(g, pr, d, r, P, MM + c, META + (size_t)c * g.mw, first, norm);
    }
};

hipError_t qc_prepare(const QcGeom& g, bool f32) {
    if (!f32) return qc_frame_prepare<QcFloatRule<double, double>>(g);
    const hipError_t e = qc_frame_prepare<QcFloatRule<float, double>>(g);
    return e != hipSuccess ? e : qc_frame_prepare<QcFloatRule<float, float>>(g);
}

hipError_t qc_launch(const QcGeom& g, bool f32, const int32_t* tab, const double* llr, int64_t ld, uint8_t* bits,
                     int32_t* iters, double* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s) {
    return f32 ? qc_frame_launch<QcFloatRule<float, double>>(g, tab, llr, ld, bits, iters, post, ld_post, batch, work, s)
               : qc_frame_launch<QcFloatRule<double, double>>(g, tab, llr, ld, bits, iters, post, ld_post, batch, work,
                                                              s);
}
hipError_t qc_launch(const QcGeom& g, const int32_t* tab, const float* llr, int64_t ld, uint8_t* bits, int32_t* iters,
                     float* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s) {
    return qc_frame_launch<QcFloatRule<float, float>>(g, tab, llr, ld, bits, iters, post, ld_post, batch, work, s);
}

}  // namespace pl

// int8 fixed-point layered normalised min-sum for quasi-cyclic LDPC codes on
// gfx950 (MI355X), and the LLR quantiser in front of it.  The definition (the
// three saturation bounds, the integer rule, the quantiser's rounding):
// include/polarldpc.h, pl_ldpc_qc_fixed_plan_create and pl_llr_quantize.  All
// arithmetic is on 32-bit integers in registers, |values| <= 254; only the
// state is narrow.
// The kernel, its mapping and its synchronisation: ldpc_qc_frame.hpp; this file
// is its int8 rule.
// State per frame (ldpc_plan.hpp, QcFixedGeom):
//   at 0      [m][mw] u32 per check.  maxdc <= 14 (the DCAP 8 instances, and the DCAP
//             16 ones when the plan says so), mw = 1: the two minima already scaled
//             and clamped (bits 0-6, 7-13), idx1 (14-17), the negative flags
//             (18-31); the parity is their popcount.  Otherwise
//             mw = 1 + ceil(maxdc / 32): word 0 = the minima (bits 0-7, 8-15), idx1
//             (16-26), the parity of the negative inputs (27); words 1 .. = the
//             negative flags, 32 positions a word.
//             R[c][j] is rebuilt as +- the stored minimum: no multiply on the way in.
//   at off_p  P[n] int8
// The checks of a block row touch distinct variables, and LDS and global byte
// stores write their byte only, so neighbouring lanes may share a dword of P.
#include "ldpc_qc_frame.hpp"

namespace pl {

PL_DEV int qf_clamp(int x, int lim) { return x < -lim ? -lim : (x > lim ? lim : x); }

struct QfCheck {
    int m1, m2;  // the minima, scaled and clamped
    uint32_t idx1, par;
};
PL_DEV uint32_t qf_pack(const QfCheck& s) {
    return (uint32_t)s.m1 | ((uint32_t)s.m2 << 8) | (s.idx1 << 16) | (s.par << 27);
}
PL_DEV QfCheck qf_unpack(uint32_t w) {
    return {(int)(w & 255u), (int)((w >> 8) & 255u), (w >> 16) & 2047u, (w >> 27) & 1u};
}
// the one-word form of a check of degree <= 14: the flags ride along, the parity is their popcount
PL_DEV uint32_t qf_pack1(const QfCheck& s, uint32_t negs) {
    return (uint32_t)s.m1 | ((uint32_t)s.m2 << 7) | (s.idx1 << 14) | (negs << 18);
}
PL_DEV QfCheck qf_unpack1(uint32_t w) {
    return {(int)(w & 127u), (int)((w >> 7) & 127u), (w >> 14) & 15u, (uint32_t)__builtin_popcount(w >> 18) & 1u};
}
// R_cj from the state of check c; neg: input j was negative
PL_DEV int qf_c2v(const QfCheck& s, uint32_t neg, uint32_t j) {
    const int mag = (j == s.idx1) ? s.m2 : s.m1;
    return ((s.par ^ neg) & 1u) ? -mag : mag;
}
// the running minima of |q| over a check's inputs, the first position on a tie
struct QfMin {
    int min1 = 255, min2 = 255;
    uint32_t idx1 = 0, par = 0;
    PL_DEV void take(int q, uint32_t j) {
        const int a = q < 0 ? -q : q;
        if (a < min1) { min2 = min1; min1 = a; idx1 = j; }
        else if (a < min2) min2 = a;
        par ^= q < 0 ? 1u : 0u;
    }
    PL_DEV QfCheck scaled(const QcFixedGeom& g) const {
        const int s1 = (min1 * g.norm16) >> 4, s2 = (min2 * g.norm16) >> 4;
        return {s1 < g.msg_max ? s1 : g.msg_max, s2 < g.msg_max ? s2 : g.msg_max, idx1, par};
    }
};

// One layered update of check r of a block row of degree d >= 2; pr: its d (block
// column, shift) pairs; cw: the check's mw words.  DCAP > 0 requires d <= DCAP <= 32.
// first: the check words hold nothing yet (R = 0).
template <int DCAP>
PL_DEV void qf_check_update(const QcFixedGeom& g, const int32_t* __restrict__ pr, int d, int r, int8_t* P,
                            uint32_t* cw, bool first) {
    const uint32_t w0 = first ? 0u : cw[0];  // zero minima: R = 0
    // one word a check: every DCAP 8 plan, and the DCAP 16 plans of degree <= 14 (the same in every lane)
    const bool one = DCAP == 8 || (DCAP == 16 && g.mw == 1);
    const QfCheck old = one ? qf_unpack1(w0) : qf_unpack(w0);
    QfMin mn;
    if constexpr (DCAP > 0) {
        const uint32_t negw = one ? (w0 >> 18) : (first ? 0u : cw[1]);
        int q[DCAP];
#pragma unroll
        for (int j = 0; j < DCAP; ++j) {
            q[j] = 0;
            if (j < d) {
                const int p = P[qc_var(pr[2 * j], pr[2 * j + 1], r, g.z)];
                q[j] = qf_clamp(p - qf_c2v(old, (negw >> j) & 1u, (uint32_t)j), 127);
                mn.take(q[j], (uint32_t)j);
            }
        }
        const QfCheck nw = mn.scaled(g);
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < DCAP; ++j) {
            if (j < d) {
                const uint32_t nb = q[j] < 0 ? 1u : 0u;
                P[qc_var(pr[2 * j], pr[2 * j + 1], r, g.z)] = (int8_t)qf_clamp(q[j] + qf_c2v(nw, nb, (uint32_t)j), 127);
                acc |= nb << j;
            }
        }
        if (one) {
            cw[0] = qf_pack1(nw, acc);
        } else {
            cw[1] = acc;
            cw[0] = qf_pack(nw);
        }
    } else {
        uint32_t negw = 0;
        for (int j = 0; j < d; ++j) {
            if (!first && (j & 31) == 0) negw = cw[1 + (j >> 5)];
            const int p = P[qc_var(pr[2 * j], pr[2 * j + 1], r, g.z)];
            mn.take(qf_clamp(p - qf_c2v(old, (negw >> (j & 31)) & 1u, (uint32_t)j), 127), (uint32_t)j);
        }
        const QfCheck nw = mn.scaled(g);
        uint32_t acc = 0;
        negw = 0;
        for (int j = 0; j < d; ++j) {
            if (!first && (j & 31) == 0) negw = cw[1 + (j >> 5)];  // the old flags: this word is stored below, after its last use
            const int v = qc_var(pr[2 * j], pr[2 * j + 1], r, g.z);
            const int q = qf_clamp((int)P[v] - qf_c2v(old, (negw >> (j & 31)) & 1u, (uint32_t)j), 127);
            const uint32_t nb = q < 0 ? 1u : 0u;
            P[v] = (int8_t)qf_clamp(q + qf_c2v(nw, nb, (uint32_t)j), 127);
            acc |= nb << (j & 31);
            if ((j & 31) == 31 || j == d - 1) { cw[1 + (j >> 5)] = acc; acc = 0; }
        }
        cw[0] = qf_pack(nw);
    }
}

struct QcFixedRule {
    using Geom = QcFixedGeom;
    using IO = int8_t;
    using Elem = int8_t;
    uint32_t* CW;
    int8_t* P;
    PL_DEV QcFixedRule(const QcFixedGeom& g, unsigned char* base)
        : CW(reinterpret_cast<uint32_t*>(base)), P(reinterpret_cast<int8_t*>(base + g.off_p)) {}
    static PL_DEV int8_t load(const QcFixedGeom& g, int8_t x) { return (int8_t)qf_clamp((int)x, g.llr_max); }
    template <int DCAP>
    PL_DEV void update(const QcFixedGeom& g, const int32_t* __restrict__ pr, int d, int r, int c, bool first) const {
        qf_check_update<DCAP>(g, pr, d, r, P, CW + (size_t)c * g.mw, first);
    }
};

hipError_t qc_prepare(const QcFixedGeom& g) { return qc_frame_prepare<QcFixedRule>(g); }

hipError_t qc_launch(const QcFixedGeom& g, const int32_t* tab, const int8_t* llr, int64_t ld, uint8_t* bits,
                     int32_t* iters, int8_t* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s) {
    return qc_frame_launch<QcFixedRule>(g, tab, llr, ld, bits, iters, post, ld_post, batch, work, s);
}

// ---- the quantiser: L = clamp(rint((double)llr * scale), -llr_max, llr_max), NaN -> 0 ----
// Mapping as ldpc_qc_ratematch.hip's: a row's output is cut at its 16-byte boundaries, one thread a
// piece -- piece 0 the bytes in front of the row's first boundary, piece p >= 1 the 16 bytes behind
// boundary p - 1, the last one cut short at the row's end.  A whole piece is one 16-byte store, a cut one
// goes byte by byte, so any pointer and any pitch take the wide stores for all but a row's two ends.
constexpr unsigned kQzThreads = 256;
constexpr int64_t kQzMaxItems = ((int64_t)1 << 31) - kQzThreads;

template <typename TIN>
PL_DEV uint32_t qz_value(TIN v, double scale, double lim) {
    double x = rint((double)v * scale);  // half to even; +-inf stays, and is clamped
    x = x != x ? 0.0 : (x < -lim ? -lim : (x > lim ? lim : x));
    return (uint32_t)(int)x & 255u;
}

template <typename TIN>
__global__ void __launch_bounds__(kQzThreads)
llr_quantize_kernel(const TIN* __restrict__ llr, int64_t ldi, uint32_t W, uint32_t total, uint32_t n, double scale,
                    double lim, int8_t* __restrict__ out, int64_t ldo) {
    const uint32_t idx = blockIdx.x * kQzThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, p = idx - row * W;
    const TIN* src = llr + (int64_t)row * ldi;
    int8_t* dst = out + (int64_t)row * ldo;
    const uint32_t head = (uint32_t)(-(uintptr_t)dst) & 15u;
    uint32_t t0 = p == 0 ? 0 : head + (p - 1) * 16u;
    uint32_t t1 = p == 0 ? head : t0 + 16u;
    t1 = t1 < n ? t1 : n;
    if (t0 >= t1) return;
    if (t1 - t0 == 16u) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= qz_value(src[t0 + 4 * q + j], scale, lim) << (8 * j);
            w[q] = v;
        }
        *reinterpret_cast<uint4*>(dst + t0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint32_t t = t0; t < t1; ++t) dst[t] = (int8_t)qz_value(src[t], scale, lim);
    }
}

template <typename TIN>
static hipError_t qz_launch(const TIN* llr, int64_t ldi, int64_t batch, int n, double scale, int llr_max, int8_t* out,
                            int64_t ldo, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    const int64_t W = ((int64_t)n + 15) / 16 + 1;  // the head and ceil(n / 16) behind it cover every head
    const int64_t step = kQzMaxItems / W > 0 ? kQzMaxItems / W : 1;
    for (int64_t b0 = 0; b0 < batch; b0 += step) {
        const int64_t rows = batch - b0 < step ? batch - b0 : step;
        const uint32_t total = (uint32_t)(rows * W);
        hipLaunchKernelGGL((llr_quantize_kernel<TIN>), dim3((total + kQzThreads - 1) / kQzThreads), dim3(kQzThreads), 0,
                           s, llr + b0 * ldi, ldi, (uint32_t)W, total, (uint32_t)n, scale, (double)llr_max,
                           out + b0 * ldo, ldo);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t llr_quantize_launch(const void* llr, bool f32, int64_t ldi, int64_t batch, int n, double scale, int llr_max,
                               int8_t* out, int64_t ldo, hipStream_t s) {
    return f32 ? qz_launch((const float*)llr, ldi, batch, n, scale, llr_max, out, ldo, s)
               : qz_launch((const double*)llr, ldi, batch, n, scale, llr_max, out, ldo, s);
}

}  // namespace pl

// The compressed min-sum check state of the layered decoders and what both of
// them do with it: ldpc_layered.hip (any H, table-driven) and
// ldpc_qc_layered.hip (quasi-cyclic H, computed addresses).  One text, so the
// two kernels agree bit for bit by construction.
#pragma once
#include "common.hpp"

namespace pl {

// T: the type of the decoder's state and arithmetic, double or (the quasi-cyclic
// kernel's single-precision instances) float
template <typename T>
struct LmsCheckT {
    T min1, min2;
    uint32_t idx1, nidx, ncnt, zcnt, par;
};
using LmsCheck = LmsCheckT<double>;

// the constants and |x| of a state type, spelled in that type (no double in a float instance)
template <typename T> struct LmsNum;
template <> struct LmsNum<double> {
    using Pair = double2;
    static PL_DEV double inf() { return __builtin_inf(); }
    static PL_DEV double nan() { return __builtin_nan(""); }
    static PL_DEV double abs(double x) { return fabs(x); }
    static PL_DEV Pair pair(double a, double b) { return make_double2(a, b); }
};
template <> struct LmsNum<float> {
    using Pair = float2;
    static PL_DEV float inf() { return __builtin_inff(); }
    static PL_DEV float nan() { return __builtin_nanf(""); }
    static PL_DEV float abs(float x) { return fabsf(x); }
    static PL_DEV Pair pair(float a, float b) { return make_float2(a, b); }
};

// Meta word of a check.  mw == 1 (every degree <= 16): idx1 bits 0-3, nidx 4-7,
// NaN count 8-9 and zero count 10-11 (saturating at 2), parity 12, negative
// flags 16-31.  mw > 1: idx1 0-10, nidx 11-21, NaN count 22-23, zero count
// 24-25, parity 26; the flags follow in mw - 1 words of 32 positions.
template <typename T>
PL_DEV uint32_t lms_pack(const LmsCheckT<T>& s, bool small, uint32_t negs) {
    return small ? (s.idx1 | (s.nidx << 4) | (s.ncnt << 8) | (s.zcnt << 10) | (s.par << 12) | (negs << 16))
                 : (s.idx1 | (s.nidx << 11) | (s.ncnt << 22) | (s.zcnt << 24) | (s.par << 26));
}
template <typename T>
PL_DEV void lms_unpack(uint32_t w, bool small, LmsCheckT<T>& s) {
    if (small) {
        s.idx1 = w & 15u; s.nidx = (w >> 4) & 15u; s.ncnt = (w >> 8) & 3u; s.zcnt = (w >> 10) & 3u; s.par = (w >> 12) & 1u;
    } else {
        s.idx1 = w & 2047u; s.nidx = (w >> 11) & 2047u; s.ncnt = (w >> 22) & 3u; s.zcnt = (w >> 24) & 3u; s.par = (w >> 26) & 1u;
    }
}

// R_cj from the state of check c over all its inputs; `neg` = input j was
// negative.  The sign product over k != j is +-1 by the parity of negatives,
// +-0 if another input is zero (a single zero is the smallest input, idx1),
// NaN if another input is NaN; the min over k != j is min2 at idx1, else min1.
template <typename T>
PL_DEV T lms_c2v(const LmsCheckT<T>& s, uint32_t neg, uint32_t j, T norm) {
    const T mn = (j == s.idx1) ? s.min2 : s.min1;
    T sp = ((s.par ^ neg) & 1u) ? T(-1) : T(1);
    sp = (s.zcnt >= 2u || (s.zcnt == 1u && s.idx1 != j)) ? sp * T(0) : sp;
    const T nan = LmsNum<T>::nan();  // a value, not a call, in the conditional's arm: it stays a select
    sp = (s.ncnt >= 2u || (s.ncnt == 1u && s.nidx != j)) ? nan : sp;
    return (sp * mn) * norm;
}

template <bool WAVE>
PL_DEV void lms_sync() {
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

// OR of `pred` over the workgroup behind one barrier, words[parity][wavefront]
// double-buffered by the iteration parity, as ldpc.hip's wg_any -- but that one
// reads the words four at a time and so needs a multiple of four wavefronts;
// a layered workgroup has any number from 1 to 16, so this reads them singly.
PL_DEV bool lms_wg_any(bool pred, uint32_t* words, int parity) {
    const bool any_w = __ballot(pred) != 0;
    if (__lane_id() == 0) words[parity * 16 + (threadIdx.x >> 6)] = any_w ? 1u : 0u;
    __syncthreads();
    uint32_t any = 0;
    const int nw = (blockDim.x + 63) >> 6;
    for (int k = 0; k < nw; ++k) any |= words[parity * 16 + k];
    return any != 0u;
}

}  // namespace pl

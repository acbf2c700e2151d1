// The bit interleaver's parameter check and its index function, usable from host and device code: plain
// C++, no HIP.  The definition: include/polarldpc.h at pl_interleave_check.  The kernels
// (interleave.hip) and pl_interleave_index evaluate the same inline functions below.
#pragma once
#include <stdint.h>

#include <string>

#if defined(__HIPCC__)
#define PL_ILV_HD __host__ __device__ inline
#else
#define PL_ILV_HD inline
#endif

namespace pl {

struct IlvStatus {
    int code = 0;  // PL_OK or PL_EINVAL
    std::string msg;
};

constexpr int kIlvRect = 0, kIlvTri = 1;  // PL_ILV_RECT, PL_ILV_TRI
constexpr int64_t kIlvMaxE = (int64_t)1 << 30;
constexpr int kIlvMaxRows = 64;

// What the index function needs, derived once on the host and passed by value to the kernels.
// RECT: dim = C, Rf = E / C full rows, q = E % C cells of row Rf.
// TRI: dim = T, Rf = row(E) full rows, q = E - st(Rf) cells of row Rf, a = T - Rf.
struct IlvParams {
    uint32_t E, dim, Rf, q, a;
};

// floor(sqrt(x)), exact for x < 2^52: the double holds x exactly, and the correction steps mend the rounding
PL_ILV_HD uint64_t ilv_isqrt(uint64_t x) {
    uint64_t r = (uint64_t)__builtin_sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

// TRI: st(i) = i T - i (i - 1) / 2, the index of the first cell of row i (i <= T <= 46341: below 2^31)
PL_ILV_HD uint32_t ilv_tri_start(uint32_t T, uint32_t i) { return i * T - (i * (i - 1u)) / 2u; }

// TRI: the largest i <= T with st(i) <= x, for x <= T (T + 1) / 2
PL_ILV_HD uint32_t ilv_tri_row(uint32_t T, uint32_t x) {
    const uint64_t b = 2 * (uint64_t)T + 1, v = b * b - 8 * (uint64_t)x;
    const uint64_t r = ilv_isqrt(v);
    return (uint32_t)((b - (r + (r * r < v ? 1 : 0))) / 2);
}

// A position in the write order: cell j of row i, with the row's length; next() moves to the cell of k + 1.
template <int KIND>
struct IlvCursor {
    uint32_t i, j, len;
    PL_ILV_HD IlvCursor(const IlvParams& p, uint32_t k) {
        if (KIND == kIlvRect) {
            i = k / p.dim;
            j = k - i * p.dim;
            len = p.dim;
        } else {
            i = ilv_tri_row(p.dim, k);
            j = k - ilv_tri_start(p.dim, i);
            len = p.dim - i;
        }
    }
    // pos(k): the valid cells of the columns before j, plus the row.  Every product stays below 2^32
    // (TRI: at most Rf T <= 46341^2; RECT: at most E).
    PL_ILV_HD uint32_t pos(const IlvParams& p) const {
        const uint32_t mq = j < p.q ? j : p.q;
        if (KIND == kIlvRect) return j * p.Rf + mq + i;
        uint32_t P = mq + p.Rf * (j < p.a ? j : p.a);
        if (j > p.a) {
            const uint32_t d = j - p.a;
            P += d * p.Rf - (d * (d - 1u)) / 2u;
        }
        return P + i;
    }
    PL_ILV_HD void next() {
        if (++j == len) {
            j = 0;
            ++i;
            if (KIND == kIlvTri) --len;
        }
    }
};

// pos(k) of a checked (kind, E) with its params, 0 <= k < E
PL_ILV_HD uint32_t ilv_pos(int kind, const IlvParams& p, uint32_t k) {
    return kind == kIlvRect ? IlvCursor<kIlvRect>(p, k).pos(p) : IlvCursor<kIlvTri>(p, k).pos(p);
}

// The conditions in the header's order: kind, then 1 <= E <= 2^30, then rows (RECT 1 .. 64, TRI 0); the
// message names the first one violated.  On success *p (may be null) holds the derived values; p->dim is
// C or T.
IlvStatus ilv_check(int32_t kind, int32_t rows, int64_t E, IlvParams* p);

}  // namespace pl

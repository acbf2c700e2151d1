// The bit interleaver's parameter check (interleave_check.hpp): no HIP, no device call.
#include "interleave_check.hpp"

#include "../../include/polarldpc.h"

namespace pl {

static_assert(kIlvRect == PL_ILV_RECT && kIlvTri == PL_ILV_TRI, "the kinds of include/polarldpc.h");

IlvStatus ilv_check(int32_t kind, int32_t rows, int64_t E, IlvParams* p) {
    if (kind != PL_ILV_RECT && kind != PL_ILV_TRI)
        return {PL_EINVAL, "kind = " + std::to_string(kind) + " must be PL_ILV_RECT (0) or PL_ILV_TRI (1)"};
    if (E < 1 || E > kIlvMaxE) return {PL_EINVAL, "E = " + std::to_string(E) + " outside 1 .. 2^30"};
    if (kind == PL_ILV_RECT && (rows < 1 || rows > kIlvMaxRows))
        return {PL_EINVAL, "rows = " + std::to_string(rows) + " outside 1 .. 64 (PL_ILV_RECT)"};
    if (kind == PL_ILV_TRI && rows != 0)
        return {PL_EINVAL, "rows = " + std::to_string(rows) + " must be 0 (PL_ILV_TRI)"};
    IlvParams v;
    v.E = (uint32_t)E;
    if (kind == PL_ILV_RECT) {
        v.dim = (uint32_t)((E + rows - 1) / rows);
        v.Rf = v.E / v.dim;
        v.q = v.E % v.dim;
        v.a = 0;
    } else {
        v.dim = (uint32_t)((ilv_isqrt(8 * (uint64_t)E - 7) + 1) / 2);
        v.Rf = ilv_tri_row(v.dim, v.E);
        v.q = v.E - ilv_tri_start(v.dim, v.Rf);
        v.a = v.dim - v.Rf;
    }
    if (p) *p = v;
    return {};
}

}  // namespace pl

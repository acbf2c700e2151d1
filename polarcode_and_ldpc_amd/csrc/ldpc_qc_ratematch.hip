// Rate matching for quasi-cyclic LDPC codes on gfx950 (MI355X): bit selection on
// the transmit side, LLR recovery on the receive side.  The definition
// (parameters, the selection loop, the closed form both kernels compute, the
// recovery's sum order, fillers and accumulation): include/polarldpc.h,
// pl_rate_match.  No table: every index follows from the struct, which the
// kernels take by value.
// Mapping: a launch covers `rows` frames of W pieces each, one thread a piece,
// piece-major within a row so that consecutive lanes touch consecutive memory.
// A row's pieces are cut at the 16-byte boundaries of its output addresses: piece
// 0 is the `head` elements in front of the row's first boundary (none when the row
// starts on one), piece p >= 1 the 16 bytes behind boundary p - 1, the last one cut
// short at the row's end.  A whole piece goes out as one 16-byte store, a cut one
// element by element: any pointer and any pitch take the wide stores for all but
// the two ends of each row.  Loads are by element, since start misaligns them.
//   rate_match_kernel: a piece is up to 16 transmitted bytes, gathered one by one.
//   rate_recover_kernel: gather form; a piece is up to 2 doubles / 4 floats.  The
//     thread that owns a position sums its terms llr[r], llr[r + M], ... itself,
//     in ascending t: no atomics, and the order is the definition's.  ACC reads the
//     piece first and leaves every position that was not transmitted as it is.
// Launches stay below 2^31 work-items (row chunks), so piece indices are 32-bit.
#include "common.hpp"
#include "internal.hpp"

namespace pl {

constexpr unsigned kRmThreads = 256;
constexpr int64_t kRmMaxItems = ((int64_t)1 << 31) - kRmThreads;

// pieces of a row of len elements, EPT to 16 bytes: the head and ceil(len / EPT) behind it cover every head
static int64_t rm_pieces(int64_t len, int64_t ept) { return (len + ept - 1) / ept + 1; }

// elements [t0, t1) of piece p of a row of len elements at dst; t1 - t0 == EPT: whole, on a 16-byte boundary
template <typename T>
PL_DEV void rm_piece(const T* dst, uint32_t p, uint32_t len, uint32_t& t0, uint32_t& t1) {
    constexpr uint32_t EPT = 16 / sizeof(T);
    const uint32_t head = ((uint32_t)(-(uintptr_t)dst) & 15u) / (uint32_t)sizeof(T);
    t0 = p == 0 ? 0 : head + (p - 1) * EPT;
    t1 = p == 0 ? head : t0 + EPT;
    t1 = t1 < len ? t1 : len;
}

// codeword position - P of compact index c
PL_DEV uint32_t rm_buffer_pos(uint32_t c, uint32_t lo, uint32_t F) { return c < lo ? c : c + F; }

__global__ void __launch_bounds__(kRmThreads)
rate_match_kernel(pl_rate_match rm, const uint8_t* __restrict__ cw, int64_t ldc, uint32_t W, uint32_t total,
                  uint8_t* __restrict__ e, int64_t lde) {
    const uint32_t idx = blockIdx.x * kRmThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, p = idx - row * W;
    const uint8_t* src = cw + (int64_t)row * ldc + rm.P;
    uint8_t* dst = e + (int64_t)row * lde;
    uint32_t t0, t1;
    rm_piece(dst, p, (uint32_t)rm.E, t0, t1);
    if (t0 >= t1) return;
    const uint32_t M = (uint32_t)rm.M, F = (uint32_t)rm.fillers, lo = (uint32_t)(rm.k - rm.P - rm.fillers);
    uint32_t c = ((uint32_t)rm.c0 + t0) % M;
    if (t1 - t0 == 16u) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v |= (uint32_t)src[rm_buffer_pos(c, lo, F)] << (8 * j);
                c = c + 1 == M ? 0 : c + 1;
            }
            w[q] = v;
        }
        *reinterpret_cast<uint4*>(dst + t0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint32_t t = t0; t < t1; ++t) {
            dst[t] = src[rm_buffer_pos(c, lo, F)];
            c = c + 1 == M ? 0 : c + 1;
        }
    }
}

// the value of codeword position pos; old: what out holds there (ACC only)
template <typename TIN, typename TOUT, bool ACC>
PL_DEV TOUT rm_recover_value(const pl_rate_match& rm, const TIN* __restrict__ llr, uint32_t pos, TOUT fill, TOUT old) {
    const uint32_t P = (uint32_t)rm.P, F = (uint32_t)rm.fillers, lo = (uint32_t)(rm.k - rm.P - rm.fillers);
    const uint32_t M = (uint32_t)rm.M, c0 = (uint32_t)rm.c0, E = (uint32_t)rm.E;
    if (pos < P || pos >= P + (uint32_t)rm.ncb) return ACC ? old : (TOUT)0;  // punctured, or beyond the buffer
    const uint32_t b = pos - P;
    if (b >= lo && b < lo + F) return ACC ? old : fill;
    const uint32_t c = b < lo ? b : b - F;
    const uint32_t r = c >= c0 ? c - c0 : c + M - c0;
    if (r >= E) return ACC ? old : (TOUT)0;  // in the buffer, not reached by this transmission
    TOUT s = (TOUT)llr[r];
    for (uint32_t t = r + M; t < E; t += M) s = s + (TOUT)llr[t];  // t < E < 2^31 before M < 2^31 is added
    return ACC ? old + s : s;
}

template <typename TIN, typename TOUT, bool ACC>
__global__ void __launch_bounds__(kRmThreads)
rate_recover_kernel(pl_rate_match rm, const TIN* __restrict__ llr, int64_t ldl, uint32_t W, uint32_t total,
                    TOUT* __restrict__ out, int64_t ldo, uint32_t n_out, TOUT fill) {
    constexpr uint32_t EPT = 16 / sizeof(TOUT);  // elements of a whole piece
    const uint32_t idx = blockIdx.x * kRmThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, p = idx - row * W;
    const TIN* src = llr + (int64_t)row * ldl;
    TOUT* dst = out + (int64_t)row * ldo;
    uint32_t t0, t1;
    rm_piece(dst, p, n_out, t0, t1);
    if (t0 >= t1) return;
    if (t1 - t0 == EPT) {
        union { uint4 q; TOUT v[EPT]; } u;
        if (ACC) u.q = *reinterpret_cast<const uint4*>(dst + t0);
#pragma unroll
        for (uint32_t j = 0; j < EPT; ++j)
            u.v[j] = rm_recover_value<TIN, TOUT, ACC>(rm, src, t0 + j, fill, ACC ? u.v[j] : (TOUT)0);
        *reinterpret_cast<uint4*>(dst + t0) = u.q;
    } else {
        for (uint32_t pos = t0; pos < t1; ++pos)
            dst[pos] = rm_recover_value<TIN, TOUT, ACC>(rm, src, pos, fill, ACC ? dst[pos] : (TOUT)0);
    }
}

// rows of W pieces each, in launches below 2^31 work-items; fn(first row, work-items)
template <class Launch>
static hipError_t rm_chunks(int64_t batch, int64_t W, Launch fn) {
    const int64_t step = kRmMaxItems / W > 0 ? kRmMaxItems / W : 1;  // a single row: W < 2^27 + 2
    for (int64_t b0 = 0; b0 < batch; b0 += step) {
        const int64_t rows = batch - b0 < step ? batch - b0 : step;
        const hipError_t e = fn(b0, (uint32_t)(rows * W));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t rate_match_launch(const pl_rate_match& rm, const uint8_t* cw, int64_t ldc, int64_t batch, uint8_t* e,
                             int64_t lde, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    const int64_t W = rm_pieces(rm.E, 16);
    return rm_chunks(batch, W, [&](int64_t b0, uint32_t total) {
        hipLaunchKernelGGL(rate_match_kernel, dim3((total + kRmThreads - 1) / kRmThreads), dim3(kRmThreads), 0, s, rm,
                           cw + b0 * ldc, ldc, (uint32_t)W, total, e + b0 * lde, lde);
        return hipGetLastError();
    });
}

template <typename TIN, typename TOUT>
static hipError_t rm_recover(const pl_rate_match& rm, const TIN* llr, int64_t ldl, int64_t batch, TOUT* out,
                             int64_t ldo, int n_out, double filler, bool acc, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    const int64_t W = rm_pieces(n_out, 16 / sizeof(TOUT));
    const TOUT fill = (TOUT)filler;
    return rm_chunks(batch, W, [&](int64_t b0, uint32_t total) {
        const dim3 grid((total + kRmThreads - 1) / kRmThreads), block(kRmThreads);
        const TIN* src = llr + b0 * ldl;
        TOUT* dst = out + b0 * ldo;
        if (acc)
            hipLaunchKernelGGL((rate_recover_kernel<TIN, TOUT, true>), grid, block, 0, s, rm, src, ldl, (uint32_t)W,
                               total, dst, ldo, (uint32_t)n_out, fill);
        else
            hipLaunchKernelGGL((rate_recover_kernel<TIN, TOUT, false>), grid, block, 0, s, rm, src, ldl, (uint32_t)W,
                               total, dst, ldo, (uint32_t)n_out, fill);
        return hipGetLastError();
    });
}

hipError_t rate_recover_launch(const pl_rate_match& rm, const void* llr, int64_t ldl, bool llr_f32, int64_t batch,
                               void* out, int64_t ldo, bool out_f32, int n_out, double filler, bool acc,
                               hipStream_t s) {
    if (llr_f32)
        return out_f32 ? rm_recover(rm, (const float*)llr, ldl, batch, (float*)out, ldo, n_out, filler, acc, s)
                       : rm_recover(rm, (const float*)llr, ldl, batch, (double*)out, ldo, n_out, filler, acc, s);
    return out_f32 ? rm_recover(rm, (const double*)llr, ldl, batch, (float*)out, ldo, n_out, filler, acc, s)
                   : rm_recover(rm, (const double*)llr, ldl, batch, (double*)out, ldo, n_out, filler, acc, s);
}

}  // namespace pl

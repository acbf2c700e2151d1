// The bit interleaver between rate matching and the QAM modem on gfx950 (MI355X): f[pos(k)] = e[k] for
// bits, e[k] = f[pos(k)] for LLRs.  The definition: include/polarldpc.h at pl_interleave_check; pos(k) is
// interleave_check.hpp's IlvCursor, the same code pl_interleave_index runs on the host: closed form, no
// table.  Elements are moved as unsigned integers of their size (1, 4, 8 bytes), so every bit pattern
// survives.  Both sides of a row are cut at the 16-byte boundaries of their addresses into pieces, as
// qam_demap_kernel cuts its output: a whole piece is one 16-byte access, the cut ones at a row's two ends
// go element by element, whatever the pointer and the pitch.
//   ilv_lds_kernel<U, KIND, DEINT>: frames of at most kIlvLdsBytes.  A workgroup holds F = 1024 / tpr
//     frames, tpr threads a frame (a power of two, at least a frame's pieces up to 1024).  The image of
//     f[0:E) lies in LDS at the 16-byte phase of f's address.  Interleave: the pieces of e are loaded
//     whole and scattered into the image element by element, then the image goes out in whole pieces.
//     Deinterleave: f comes in in whole pieces, then each piece of e is gathered from the image and
//     stored whole.  Global memory sees contiguous 16-byte accesses only; the permutation happens in LDS.
//   ilv_direct_kernel<U, KIND, DEINT>: longer frames, one thread a piece of e: the same piece, gathered
//     from or scattered to global memory (a stride of about `rows`, or up to T, elements between lanes).
// A thread takes pos of its piece's first element from the closed form (one division, or one square root)
// and steps the cursor from there.  Launches stay below 2^31 work-items (row chunks).  No scratch.
#include "common.hpp"
#include "interleave_check.hpp"
#include "internal.hpp"

namespace pl {

constexpr unsigned kIlvLdsThreads = 1024, kIlvDirectThreads = 256;
constexpr int64_t kIlvMaxItems = ((int64_t)1 << 31) - kIlvLdsThreads;

template <typename U>
union IlvVec {
    uint4 u;
    U t[16 / sizeof(U)];
};

// piece pc of a row whose first element lies `lead` elements behind a 16-byte boundary: elements [lo, hi)
template <uint32_t EPT>
struct IlvPiece {
    uint32_t lo, hi;
    PL_DEV IlvPiece(uint32_t pc, uint32_t lead, uint32_t E) {
        const int32_t b = (int32_t)(pc * EPT) - (int32_t)lead;  // pc EPT <= E + 2 EPT
        lo = b < 0 ? 0u : (uint32_t)b;
        hi = (uint32_t)(b + (int32_t)EPT) < E ? (uint32_t)(b + (int32_t)EPT) : E;
    }
    PL_DEV bool empty() const { return lo >= hi; }
    PL_DEV bool whole() const { return hi - lo == EPT; }
};

template <typename U>
PL_DEV uint32_t ilv_lead(const U* p) {
    return (uint32_t)((uintptr_t)p & 15u) / (uint32_t)sizeof(U);
}

// Piece w of the e side against a linear f (global memory or the LDS image): DEINT e[k] = f[pos(k)], else
// f[pos(k)] = e[k].  e and f are row pointers.
template <typename U, int KIND, bool DEINT, typename F>
PL_DEV void ilv_piece(const IlvParams& p, const IlvPiece<16 / sizeof(U)>& w, U* e, F* f) {
    constexpr uint32_t EPT = 16 / sizeof(U);
    IlvCursor<KIND> cur(p, w.lo);
    if (w.whole()) {
        IlvVec<U> v;
        if (!DEINT) v.u = *reinterpret_cast<const uint4*>(e + w.lo);
#pragma unroll
        for (uint32_t j = 0; j < EPT; ++j) {
            if (DEINT) v.t[j] = f[cur.pos(p)];
            else const_cast<U*>(f)[cur.pos(p)] = v.t[j];
            cur.next();
        }
        if (DEINT) *reinterpret_cast<uint4*>(e + w.lo) = v.u;
    } else {
        for (uint32_t x = w.lo; x < w.hi; ++x) {
            if (DEINT) e[x] = f[cur.pos(p)];
            else const_cast<U*>(f)[cur.pos(p)] = e[x];
            cur.next();
        }
    }
}

template <typename U, int KIND, bool DEINT>
__global__ void __launch_bounds__(kIlvLdsThreads)
ilv_lds_kernel(IlvParams p, const U* __restrict__ src, int64_t lds, U* __restrict__ dst, int64_t ldd, uint32_t batch,
               uint32_t tshift, uint32_t pitch) {
    constexpr uint32_t EPT = 16 / sizeof(U);
    extern __shared__ uint4 ilv_smem[];
    const uint32_t tpr = 1u << tshift, fr = threadIdx.x >> tshift, lane = threadIdx.x & (tpr - 1u);
    const uint32_t row = blockIdx.x * (kIlvLdsThreads >> tshift) + fr;
    const bool live = row < batch;
    const U* s = src + (int64_t)row * lds;
    U* d = dst + (int64_t)row * ldd;
    const uint32_t ls = ilv_lead(s), ldl = ilv_lead(d);
    // img[x] = f[x], at f's phase within 16 bytes: a whole piece of f is a whole 16-byte LDS access
    U* img = reinterpret_cast<U*>(ilv_smem) + fr * pitch + (DEINT ? ls : ldl);
    if (live) {
        const uint32_t np = (ls + p.E + EPT - 1u) / EPT;
        for (uint32_t pc = lane; pc < np; pc += tpr) {
            const IlvPiece<EPT> w(pc, ls, p.E);
            if (DEINT) {
                if (w.whole()) {
                    *reinterpret_cast<uint4*>(img + w.lo) = *reinterpret_cast<const uint4*>(s + w.lo);
                } else {
                    for (uint32_t x = w.lo; x < w.hi; ++x) img[x] = s[x];
                }
            } else {
                ilv_piece<U, KIND, false>(p, w, const_cast<U*>(s), img);
            }
        }
    }
    __syncthreads();
    if (live) {
        const uint32_t np = (ldl + p.E + EPT - 1u) / EPT;
        for (uint32_t pc = lane; pc < np; pc += tpr) {
            const IlvPiece<EPT> w(pc, ldl, p.E);
            if (DEINT) {
                ilv_piece<U, KIND, true>(p, w, d, img);
            } else {
                if (w.whole()) {
                    *reinterpret_cast<uint4*>(d + w.lo) = *reinterpret_cast<const uint4*>(img + w.lo);
                } else {
                    for (uint32_t x = w.lo; x < w.hi; ++x) d[x] = img[x];
                }
            }
        }
    }
}

template <typename U, int KIND, bool DEINT>
__global__ void __launch_bounds__(kIlvDirectThreads)
ilv_direct_kernel(IlvParams p, const U* __restrict__ src, int64_t lds, U* __restrict__ dst, int64_t ldd, uint32_t W,
                  uint32_t total) {
    constexpr uint32_t EPT = 16 / sizeof(U);
    const uint32_t idx = blockIdx.x * kIlvDirectThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, pc = idx - row * W;
    const U* s = src + (int64_t)row * lds;
    U* d = dst + (int64_t)row * ldd;
    const IlvPiece<EPT> w(pc, ilv_lead(DEINT ? d : s), p.E);
    if (w.empty()) return;
    if (DEINT) ilv_piece<U, KIND, true>(p, w, d, s);
    else ilv_piece<U, KIND, false>(p, w, const_cast<U*>(s), d);
}

// rows in launches below 2^31 work-items; fn(first row, rows)
template <class Launch>
static hipError_t ilv_chunks(int64_t batch, int64_t step, Launch fn) {
    for (int64_t b0 = 0; b0 < batch; b0 += step) {
        const hipError_t e = fn(b0, batch - b0 < step ? batch - b0 : step);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename U, int KIND, bool DEINT>
static hipError_t ilv_run(const IlvParams& p, const U* src, int64_t lds, U* dst, int64_t ldd, int64_t batch,
                          hipStream_t st) {
    constexpr int64_t EPT = 16 / sizeof(U);
    const int64_t W = (p.E + 2 * EPT - 2) / EPT;  // the pieces of a row at the worst phase
    if ((int64_t)p.E * (int64_t)sizeof(U) <= kIlvLdsBytes) {
        uint32_t tshift = 0;
        while (tshift < 10 && ((int64_t)1 << tshift) < W) ++tshift;
        const int64_t F = kIlvLdsThreads >> tshift;
        const uint32_t pitch = (uint32_t)(W * EPT);  // >= (EPT - 1) + E, a multiple of 16 bytes
        const size_t bytes = (size_t)F * pitch * sizeof(U);
        const auto kern = ilv_lds_kernel<U, KIND, DEINT>;
        if (bytes > 65536) {
            const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)bytes);
            if (e != hipSuccess) return e;
        }
        return ilv_chunks(batch, kIlvMaxItems / kIlvLdsThreads * F, [&](int64_t b0, int64_t rows) {
            hipLaunchKernelGGL(kern, dim3((unsigned)((rows + F - 1) / F)), dim3(kIlvLdsThreads), bytes, st, p,
                               src + b0 * lds, lds, dst + b0 * ldd, ldd, (uint32_t)rows, tshift, pitch);
            return hipGetLastError();
        });
    }
    return ilv_chunks(batch, kIlvMaxItems / W, [&](int64_t b0, int64_t rows) {  // W <= 2^30 / 2 + 1
        const uint32_t total = (uint32_t)(rows * W);
        hipLaunchKernelGGL((ilv_direct_kernel<U, KIND, DEINT>),
                           dim3((total + kIlvDirectThreads - 1) / kIlvDirectThreads), dim3(kIlvDirectThreads), 0, st, p,
                           src + b0 * lds, lds, dst + b0 * ldd, ldd, (uint32_t)W, total);
        return hipGetLastError();
    });
}

template <typename U, bool DEINT>
static hipError_t ilv_kind(int kind, const IlvParams& p, const void* src, int64_t lds, void* dst, int64_t ldd,
                           int64_t batch, hipStream_t st) {
    return kind == kIlvRect ? ilv_run<U, kIlvRect, DEINT>(p, (const U*)src, lds, (U*)dst, ldd, batch, st)
                            : ilv_run<U, kIlvTri, DEINT>(p, (const U*)src, lds, (U*)dst, ldd, batch, st);
}

hipError_t bit_interleave_launch(int kind, const IlvParams& p, const uint8_t* e, int64_t lde, int64_t batch, uint8_t* f,
                                 int64_t ldf, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    return ilv_kind<uint8_t, false>(kind, p, e, lde, f, ldf, batch, s);
}

hipError_t llr_deinterleave_launch(int kind, const IlvParams& p, const void* f, int64_t ldf, int64_t batch, void* e,
                                   int64_t lde, bool f32, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    return f32 ? ilv_kind<uint32_t, true>(kind, p, f, ldf, e, lde, batch, s)
               : ilv_kind<uint64_t, true>(kind, p, f, ldf, e, lde, batch, s);
}

}  // namespace pl

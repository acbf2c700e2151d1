// Rate matching for polar codes on gfx950 (MI355X): bit selection on the transmit
// side, LLR recovery on the receive side.  The definition (parameters, the
// interleaved sequence y[m] = x[J(m)], the selection, the recovery's sum order,
// known_llr and accumulation): include/polarldpc.h, pl_polar_rm.  No table: every
// index follows from the parameters, which the kernels take by value.
// Mapping (ldpc_qc_ratematch.hip's piece scheme, restated): a launch covers `rows`
// frames of W pieces each, one thread a piece, piece-major within a row so that
// consecutive lanes touch consecutive memory.  A row's pieces are cut at the
// 16-byte boundaries of its output addresses: piece 0 is the `head` elements in
// front of the row's first boundary (none when the row starts on one), piece
// p >= 1 the 16 bytes behind boundary p - 1, the last one cut short at the row's
// end.  A whole piece goes out as one 16-byte store, a cut one element by element.
// Recover loads by element: the selection's offset N - E misaligns the source run.
//   polar_rate_match_kernel: a piece is up to 16 transmitted bytes.  A whole piece that
//     lies inside one sub-block is a contiguous run of the codeword: one index
//     computation, then four dword loads where the run's address allows, else 16
//     byte loads at constant offsets.  A piece that straddles sub-blocks (always so
//     for S < 16) gathers byte by byte.
//   polar_rate_recover_kernel<TIN, ACC>: gather form; a piece is up to 2 doubles.  The
//     thread that owns a position sums its terms llr[m], llr[m + N], ... itself, in
//     ascending t: no atomics, and the order is the definition's.  ACC reads the
//     piece first and leaves every position that was not transmitted as it is.
// perm / inv travel as four 64-bit words each and a byte comes out by two selects and
// a shift: a by-value array indexed per lane would live in scratch.  S and N are
// powers of two, so / and mod are a shift and a mask.
// Launches stay below 2^31 work-items (row chunks), so piece indices are 32-bit.
#include "common.hpp"
#include "internal.hpp"

namespace pl {

constexpr unsigned kPrmThreads = 256;
constexpr int64_t kPrmMaxItems = ((int64_t)1 << 31) - kPrmThreads;

// what the kernels need of a checked pl_polar_rm
struct PrmArgs {
    uint32_t N, E, U, lgS;  // S = 1 << lgS
    uint32_t shorten, pad;  // used when E < N
    uint64_t perm[4], inv[4];
};

static PrmArgs prm_args(const pl_polar_rm& rm) {
    PrmArgs a{};
    a.N = (uint32_t)rm.N;
    a.E = (uint32_t)rm.E;
    a.U = (uint32_t)rm.U;
    while ((1u << a.lgS) < (uint32_t)rm.S) ++a.lgS;
    a.shorten = rm.mode == PL_PRM_SHORTEN;
    for (int i = 0; i < 32; ++i) {
        a.perm[i >> 3] |= (uint64_t)rm.perm[i] << (8 * (i & 7));
        a.inv[i >> 3] |= (uint64_t)rm.inv[i] << (8 * (i & 7));
    }
    return a;
}

// pieces of a row of len elements, EPT to 16 bytes: the head and ceil(len / EPT) behind it cover every head
static int64_t prm_pieces(int64_t len, int64_t ept) { return (len + ept - 1) / ept + 1; }

// elements [t0, t1) of piece p of a row of len elements at dst; t1 - t0 == EPT: whole, on a 16-byte boundary
template <typename T>
PL_DEV void prm_piece(const T* dst, uint32_t p, uint32_t len, uint32_t& t0, uint32_t& t1) {
    constexpr uint32_t EPT = 16 / sizeof(T);
    const uint32_t head = ((uint32_t)(-(uintptr_t)dst) & 15u) / (uint32_t)sizeof(T);
    t0 = p == 0 ? 0 : head + (p - 1) * EPT;
    t1 = p == 0 ? head : t0 + EPT;
    t1 = t1 < len ? t1 : len;
}

// byte i < 32 of four packed words
PL_DEV uint32_t prm_byte(const uint64_t (&w)[4], uint32_t i) {
    const uint64_t lo = (i & 8u) ? w[1] : w[0], hi = (i & 8u) ? w[3] : w[2];
    return (uint32_t)(((i & 16u) ? hi : lo) >> (8u * (i & 7u))) & 0xFFu;
}

// index v with its sub-block number sent through the packed permutation w
PL_DEV uint32_t prm_map(const uint64_t (&w)[4], uint32_t v, uint32_t lgS) {
    return (prm_byte(w, v >> lgS) << lgS) | (v & ((1u << lgS) - 1u));
}

// interleaved index of transmitted bit t, and its codeword position
PL_DEV uint32_t prm_index(const PrmArgs& a, uint32_t t) {
    return a.E >= a.N ? (t & (a.N - 1u)) : a.shorten ? t : t + a.U;
}
PL_DEV uint32_t prm_source(const PrmArgs& a, uint32_t t) { return prm_map(a.perm, prm_index(a, t), a.lgS); }

__global__ void __launch_bounds__(kPrmThreads)
polar_rate_match_kernel(PrmArgs a, const uint8_t* __restrict__ cw, int64_t ldc, uint32_t W, uint32_t total,
                        uint8_t* __restrict__ e, int64_t lde) {
    const uint32_t idx = blockIdx.x * kPrmThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, p = idx - row * W;
    const uint8_t* src = cw + (int64_t)row * ldc;
    uint8_t* dst = e + (int64_t)row * lde;
    uint32_t t0, t1;
    prm_piece(dst, p, a.E, t0, t1);
    if (t0 >= t1) return;
    if (t1 - t0 == 16u) {
        uint32_t w[4];
        const uint32_t m0 = prm_index(a, t0), S = 1u << a.lgS;
        if ((m0 & (S - 1u)) + 16u <= S) {  // inside one sub-block: 16 contiguous source bytes, one index computation
            const uint8_t* run = src + prm_map(a.perm, m0, a.lgS);
            if (((uintptr_t)run & 3u) == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = reinterpret_cast<const uint32_t*>(run)[q];
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    w[q] = (uint32_t)run[4 * q] | (uint32_t)run[4 * q + 1] << 8 | (uint32_t)run[4 * q + 2] << 16 |
                           (uint32_t)run[4 * q + 3] << 24;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t v = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) v |= (uint32_t)src[prm_source(a, t0 + 4 * q + j)] << (8 * j);
                w[q] = v;
            }
        }
        *reinterpret_cast<uint4*>(dst + t0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint32_t t = t0; t < t1; ++t) dst[t] = src[prm_source(a, t)];
    }
}

// the value of decoder input i; old: what out holds there (ACC only)
template <typename TIN, bool ACC>
PL_DEV double prm_recover_value(const PrmArgs& a, const TIN* __restrict__ llr, uint32_t i, double known, double old) {
    const uint32_t m = prm_map(a.inv, i, a.lgS);
    double s;
    if (a.E >= a.N) {
        s = (double)llr[m];
        for (uint32_t t = m + a.N; t < a.E; t += a.N) s = s + (double)llr[t];  // t < E <= 2^30 before N <= 2^15 is added
    } else if (a.shorten) {
        if (m >= a.E) return ACC ? old : known;
        s = (double)llr[m];
    } else {
        if (m < a.U) return ACC ? old : 0.0;
        s = (double)llr[m - a.U];
    }
    return ACC ? old + s : s;
}

template <typename TIN, bool ACC>
__global__ void __launch_bounds__(kPrmThreads)
polar_rate_recover_kernel(PrmArgs a, const TIN* __restrict__ llr, int64_t ldl, uint32_t W, uint32_t total,
                          double* __restrict__ out, int64_t ldo, double known) {
    const uint32_t idx = blockIdx.x * kPrmThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, p = idx - row * W;
    const TIN* src = llr + (int64_t)row * ldl;
    double* dst = out + (int64_t)row * ldo;
    uint32_t t0, t1;
    prm_piece(dst, p, a.N, t0, t1);
    if (t0 >= t1) return;
    if (t1 - t0 == 2u) {
        union { uint4 q; double v[2]; } u;
        if (ACC) u.q = *reinterpret_cast<const uint4*>(dst + t0);
#pragma unroll
        for (uint32_t j = 0; j < 2; ++j)
            u.v[j] = prm_recover_value<TIN, ACC>(a, src, t0 + j, known, ACC ? u.v[j] : 0.0);
        *reinterpret_cast<uint4*>(dst + t0) = u.q;
    } else {
        for (uint32_t i = t0; i < t1; ++i) dst[i] = prm_recover_value<TIN, ACC>(a, src, i, known, ACC ? dst[i] : 0.0);
    }
}

// rows of W pieces each, in launches below 2^31 work-items; fn(first row, work-items)
template <class Launch>
static hipError_t prm_chunks(int64_t batch, int64_t W, Launch fn) {
    const int64_t step = kPrmMaxItems / W > 0 ? kPrmMaxItems / W : 1;  // a single row: W <= 2^26 + 1
    for (int64_t b0 = 0; b0 < batch; b0 += step) {
        const int64_t rows = batch - b0 < step ? batch - b0 : step;
        const hipError_t e = fn(b0, (uint32_t)(rows * W));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t polar_rate_match_launch(const pl_polar_rm& rm, const uint8_t* cw, int64_t ldc, int64_t batch, uint8_t* e,
                                   int64_t lde, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    const PrmArgs a = prm_args(rm);
    const int64_t W = prm_pieces(rm.E, 16);
    return prm_chunks(batch, W, [&](int64_t b0, uint32_t total) {
        hipLaunchKernelGGL(polar_rate_match_kernel, dim3((total + kPrmThreads - 1) / kPrmThreads), dim3(kPrmThreads), 0,
                           s, a, cw + b0 * ldc, ldc, (uint32_t)W, total, e + b0 * lde, lde);
        return hipGetLastError();
    });
}

template <typename TIN>
static hipError_t prm_recover(const pl_polar_rm& rm, const TIN* llr, int64_t ldl, int64_t batch, double* out,
                              int64_t ldo, double known, bool acc, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    const PrmArgs a = prm_args(rm);
    const int64_t W = prm_pieces(rm.N, 2);
    return prm_chunks(batch, W, [&](int64_t b0, uint32_t total) {
        const dim3 grid((total + kPrmThreads - 1) / kPrmThreads), block(kPrmThreads);
        const TIN* src = llr + b0 * ldl;
        double* dst = out + b0 * ldo;
        if (acc)
            hipLaunchKernelGGL((polar_rate_recover_kernel<TIN, true>), grid, block, 0, s, a, src, ldl, (uint32_t)W, total,
                               dst, ldo, known);
        else
            hipLaunchKernelGGL((polar_rate_recover_kernel<TIN, false>), grid, block, 0, s, a, src, ldl, (uint32_t)W,
                               total, dst, ldo, known);
        return hipGetLastError();
    });
}

hipError_t polar_rate_recover_launch(const pl_polar_rm& rm, const void* llr, int64_t ldl, bool llr_f32, int64_t batch,
                                     double* out, int64_t ldo, double known, bool acc, hipStream_t s) {
    return llr_f32 ? prm_recover(rm, (const float*)llr, ldl, batch, out, ldo, known, acc, s)
                   : prm_recover(rm, (const double*)llr, ldl, batch, out, ldo, known, acc, s);
}

}  // namespace pl

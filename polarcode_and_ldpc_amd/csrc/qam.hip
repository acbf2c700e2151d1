// Gray-mapped square QAM on gfx950 (MI355X): modulator, complex AWGN, max-log soft demapper.
// The definition (bit to axis, the Gray axis mapping, the scale, the symbol layout, the noise stream and
// the demapper's operation order): include/polarldpc.h at pl_qam_check.  H = m / 2 bits per axis is a
// template parameter, so every loop over bits and levels unrolls and every value stays in a register.
// Mapping of the two transmit kernels: one thread a symbol, symbol-major within a row: a thread reads its
// m codeword bytes (zeros behind E) and writes I and Q, as one 16-byte store where the address allows.
//   qam_tx_kernel<H, NOISE>: NOISE adds sigma z of the symbol's Box-Muller pair (common.hpp normal_pair,
//     salt kQamSalt, counter s): one Philox call, one log, one sqrt and one sincospi per symbol.
// The demapper is output-driven, as the rate matchers are (polar_ratematch.hip's piece scheme):
//   qam_demap_kernel<H, T>: one thread a group of G symbols, V = G m LLRs; G = 2 for float with m = 2, 6
//     and 1 otherwise, so that V sizeof(T) is a multiple of 16 bytes and every group of a row meets the
//     16-byte boundaries of the output at the same offset `head`.  Per axis the 2^H squared distances are
//     computed once and each of the H bits takes its two minima over them (the level sets are compile-time
//     masks).  A whole group goes out as `head` single elements, 16-byte stores, and the rest as single
//     elements; the group cut by the row's end goes out element by element.
// Block Rayleigh fading (the definition: include/polarldpc.h at pl_qam_fading_check) rides on both mappings:
//   qam_rayleigh_kernel<H>: qam_tx_kernel's thread a symbol, with the coefficient of the symbol's fading block
//     (a second Box-Muller pair, salt SALT_FADE, counter q = s / Lc) recomputed by every thread of the block
//     and written by the block's first symbol.
//   qam_demap_csi_kernel<H, T>: qam_demap_kernel's groups and stores; per symbol one more 16-byte load (the
//     coefficient), five products, two divisions, and the erased symbol (|h|^2 == 0.0 -> +0.0).
// The exact log-MAP demapper (the definition: include/polarldpc.h at pl_qam_demap_logmap) rides on the demappers:
//   qam_demap_logmap_kernel<H, T, CSI>: their groups, loads and stores; per axis value the minima of max-log, then
//     h 2^h expm1 and 2 h log1p as glibc computes them (libm_exact.hpp), levels and axis values in rolled loops.
// Launches stay below 2^31 work-items (row chunks), so work-item indices are 32-bit.
#include "common.hpp"
#include "internal.hpp"
#include "libm_exact.hpp"
#include "qam_check.hpp"

namespace pl {

constexpr unsigned kQamThreads = 256;
constexpr int64_t kQamMaxItems = ((int64_t)1 << 31) - kQamThreads;
constexpr uint32_t kQamSalt = 0x9A3A9A3Au;

// integer level of the H axis bits b[0], b[1], ...: c_p = c_(p-1) ^ b_p, idx = sum c_p 2^(H-1-p), a = 2^H - 1 - 2 idx
template <int H>
PL_DEV int qam_level(const uint32_t (&b)[H]) {
    uint32_t c = 0, idx = 0;
#pragma unroll
    for (int p = 0; p < H; ++p) {
        c ^= b[p];
        idx = (idx << 1) | c;
    }
    return ((1 << H) - 1) - 2 * (int)idx;
}

template <int H, bool NOISE>
__global__ void __launch_bounds__(kQamThreads)
qam_tx_kernel(const uint8_t* __restrict__ e, int64_t lde, uint32_t E, uint32_t S, uint32_t total, double scale,
              double sigma, uint64_t seed, uint64_t f0, double* __restrict__ out, int64_t ldo) {
    constexpr uint32_t M = 2 * H;
    const uint32_t idx = blockIdx.x * kQamThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / S, s = idx - row * S;
    uint32_t bi[H] = {}, bq[H] = {};
    if (e) {
        const uint8_t* src = e + (int64_t)row * lde;
        const uint32_t t0 = s * M;  // < E <= 2^30
#pragma unroll
        for (int p = 0; p < H; ++p) {
            bi[p] = t0 + 2 * p < E ? src[t0 + 2 * p] & 1u : 0u;
            bq[p] = t0 + 2 * p + 1 < E ? src[t0 + 2 * p + 1] & 1u : 0u;
        }
    }
    double vi = (double)qam_level<H>(bi) * scale, vq = (double)qam_level<H>(bq) * scale;
    if (NOISE) {
        double z0, z1;
        normal_pair(seed, kQamSalt, s, f0 + row, z0, z1);
        vi = vi + sigma * z0;
        vq = vq + sigma * z1;
    }
    double* o = out + (int64_t)row * ldo + 2 * (int64_t)s;
    if (((uintptr_t)o & 15u) == 0) {
        *reinterpret_cast<double2*>(o) = make_double2(vi, vq);
    } else {
        o[0] = vi;
        o[1] = vq;
    }
}

// the H LLRs of one axis value r: llr[p] = (min d over levels with bit p = 1  -  min d over levels with bit p = 0) w
template <int H>
PL_DEV void qam_axis_llr(double r, double scale, double w, double (&llr)[H]) {
    constexpr int L = 1 << H;
    double d[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
        const double t = r - (double)((L - 1) - 2 * i) * scale;
        d[i] = t * t;
    }
#pragma unroll
    for (int p = 0; p < H; ++p) {
        // bit p of level index i: c_p ^ c_(p-1) = bit H-1-p of i ^ (i >> 1); index 0 has every bit 0 and
        // index 2^(H-1-p) has bit p = 1.  Every d is NaN or none is, so the order of the minima is free.
        double d0 = d[0], d1 = d[1 << (H - 1 - p)];
#pragma unroll
        for (int i = 1; i < L; ++i) {
            if (((i ^ (i >> 1)) >> (H - 1 - p)) & 1) {
                if (i != (1 << (H - 1 - p))) d1 = __builtin_fmin(d1, d[i]);
            } else {
                d0 = __builtin_fmin(d0, d[i]);
            }
        }
        llr[p] = (d1 - d0) * w;
    }
}

// v[0:V) to o[0:V), V sizeof(T) a multiple of 16 and o + HEAD on a 16-byte boundary
template <int HEAD, int V, typename T>
PL_DEV void qam_store_group(T* o, const T (&v)[V]) {
    constexpr int EPT = 16 / sizeof(T);
#pragma unroll
    for (int j = 0; j < HEAD; ++j) o[j] = v[j];
#pragma unroll
    for (int q = HEAD; q + EPT <= V; q += EPT) {
        union { uint4 u; T t[EPT]; } x;
#pragma unroll
        for (int j = 0; j < EPT; ++j) x.t[j] = v[q + j];
        *reinterpret_cast<uint4*>(o + q) = x.u;
    }
    if (HEAD > 0) {
#pragma unroll
        for (int j = V - (EPT - HEAD); j < V; ++j) o[j] = v[j];
    }
}

template <int H, typename T>
__global__ void __launch_bounds__(kQamThreads)
qam_demap_kernel(const double* __restrict__ y, int64_t ldy, uint32_t E, uint32_t S, uint32_t W, uint32_t total,
                 double scale, double w, T* __restrict__ llr, int64_t ldl) {
    constexpr uint32_t M = 2 * H;
    constexpr uint32_t G = (sizeof(T) == 4 && (H & 1)) ? 2 : 1;
    constexpr uint32_t V = G * M;
    constexpr uint32_t EPT = 16 / sizeof(T);
    static_assert(V % EPT == 0, "a group is whole 16-byte pieces");
    const uint32_t idx = blockIdx.x * kQamThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, g = idx - row * W;
    const double* src = y + (int64_t)row * ldy;
    T v[V];
#pragma unroll
    for (uint32_t k = 0; k < G; ++k) {
        const uint32_t s = g * G + k;
        double ri = 0.0, rq = 0.0;
        if (s < S) {
            const double* ps = src + 2 * (int64_t)s;
            if (((uintptr_t)ps & 15u) == 0) {
                const double2 pr = *reinterpret_cast<const double2*>(ps);
                ri = pr.x;
                rq = pr.y;
            } else {
                ri = ps[0];
                rq = ps[1];
            }
        }
        double li[H], lq[H];
        qam_axis_llr<H>(ri, scale, w, li);
        qam_axis_llr<H>(rq, scale, w, lq);
#pragma unroll
        for (int p = 0; p < H; ++p) {
            v[k * M + 2 * p] = (T)li[p];
            v[k * M + 2 * p + 1] = (T)lq[p];
        }
    }
    const uint32_t t0 = g * V;  // < E: W = ceil(E / V)
    T* o = llr + (int64_t)row * ldl + t0;
    if (E - t0 >= V) {
        const uint32_t head = ((uint32_t)(-(uintptr_t)o) & 15u) / (uint32_t)sizeof(T);
        if (head == 0) {
            qam_store_group<0, V, T>(o, v);
        } else if constexpr (EPT == 2) {
            qam_store_group<1, V, T>(o, v);
        } else {
            if (head == 1) qam_store_group<1, V, T>(o, v);
            else if (head == 2) qam_store_group<2, V, T>(o, v);
            else qam_store_group<3, V, T>(o, v);
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < V; ++j)
            if (j < E - t0) o[j] = v[j];
    }
}

// ---- block Rayleigh fading; the definition: include/polarldpc.h at pl_qam_fading_check ----
// The pieces of the two kernels above that the fading kernels share with them, as functions (the kernels above keep
// their own text: their code is not to change).
// the clean symbol s of row `row`: its m codeword bytes (zeros behind E, and all zeros without e) -> (vi, vq)
template <int H>
PL_DEV void qam_symbol(const uint8_t* __restrict__ e, int64_t lde, uint32_t E, uint32_t row, uint32_t s, double scale,
                       double& vi, double& vq) {
    constexpr uint32_t M = 2 * H;
    uint32_t bi[H] = {}, bq[H] = {};
    if (e) {
        const uint8_t* src = e + (int64_t)row * lde;
        const uint32_t t0 = s * M;  // < E <= 2^30
#pragma unroll
        for (int p = 0; p < H; ++p) {
            bi[p] = t0 + 2 * p < E ? src[t0 + 2 * p] & 1u : 0u;
            bq[p] = t0 + 2 * p + 1 < E ? src[t0 + 2 * p + 1] & 1u : 0u;
        }
    }
    vi = (double)qam_level<H>(bi) * scale;
    vq = (double)qam_level<H>(bq) * scale;
}

// two doubles at o / from p, 16 bytes at once where the address allows
PL_DEV void qam_store2(double* o, double a, double b) {
    if (((uintptr_t)o & 15u) == 0) {
        *reinterpret_cast<double2*>(o) = make_double2(a, b);
    } else {
        o[0] = a;
        o[1] = b;
    }
}

PL_DEV void qam_load2(const double* p, double& a, double& b) {
    if (((uintptr_t)p & 15u) == 0) {
        const double2 pr = *reinterpret_cast<const double2*>(p);
        a = pr.x;
        b = pr.y;
    } else {
        a = p[0];
        b = p[1];
    }
}

// a group of a row with `left` elements to the row's end: whole (left >= V) from the 16-byte boundary `head`
// elements on, the one cut by the row's end element by element
template <int V, typename T>
PL_DEV void qam_store_cut(T* o, const T (&v)[V], uint32_t left) {
    constexpr uint32_t EPT = 16 / sizeof(T);
    if (left >= (uint32_t)V) {
        const uint32_t head = ((uint32_t)(-(uintptr_t)o) & 15u) / (uint32_t)sizeof(T);
        if (head == 0) {
            qam_store_group<0, V, T>(o, v);
        } else if constexpr (EPT == 2) {
            qam_store_group<1, V, T>(o, v);
        } else {
            if (head == 1) qam_store_group<1, V, T>(o, v);
            else if (head == 2) qam_store_group<2, V, T>(o, v);
            else qam_store_group<3, V, T>(o, v);
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if ((uint32_t)j < left) o[j] = v[j];
    }
}

constexpr double kFadeC = 0x1.6a09e667f3bcdp-1;  // the double nearest 1 / sqrt(2)

// the coefficient of fading block q of frame f: (seed, f, q) only
PL_DEV void qam_fade_coeff(uint64_t seed, uint32_t q, uint64_t f, double& hr, double& hi) {
    double g0, g1;
    normal_pair(seed, SALT_FADE, q, f, g0, g1);
    hr = g0 * kFadeC;
    hi = g1 * kFadeC;
}

// qam_tx_kernel's mapping, one thread a symbol.  Every thread computes its block's coefficient itself (a wave runs
// the Box-Muller path as soon as one lane needs it); the block's first symbol writes it.
template <int H>
__global__ void __launch_bounds__(kQamThreads)
qam_rayleigh_kernel(const uint8_t* __restrict__ e, int64_t lde, uint32_t E, uint32_t S, uint32_t Lc, uint32_t total,
                    double scale, double sigma, uint64_t seed, uint64_t f0, double* __restrict__ out, int64_t ldo,
                    double* __restrict__ h, int64_t ldh) {
    const uint32_t idx = blockIdx.x * kQamThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / S, s = idx - row * S, q = s / Lc;
    double xi, xq, hr, hi, z0, z1;
    qam_symbol<H>(e, lde, E, row, s, scale, xi, xq);
    qam_fade_coeff(seed, q, f0 + row, hr, hi);
    normal_pair(seed, kQamSalt, s, f0 + row, z0, z1);
    const double yi = (hr * xi - hi * xq) + sigma * z0;
    const double yq = (hr * xq + hi * xi) + sigma * z1;
    qam_store2(out + (int64_t)row * ldo + 2 * (int64_t)s, yi, yq);
    if (s == q * Lc) qam_store2(h + (int64_t)row * ldh + 2 * (int64_t)q, hr, hi);
}

// qam_demap_kernel with the channel state: per symbol the coefficient of its block, the matched filter u = conj(h) y,
// r = u / |h|^2 and the weight w |h|^2; a symbol with |h|^2 == 0.0 is erased, every LLR +0.0.
template <int H, typename T>
__global__ void __launch_bounds__(kQamThreads)
qam_demap_csi_kernel(const double* __restrict__ y, int64_t ldy, const double* __restrict__ h, int64_t ldh, uint32_t E,
                     uint32_t S, uint32_t Lc, uint32_t W, uint32_t total, double scale, double w, T* __restrict__ llr,
                     int64_t ldl) {
    constexpr uint32_t M = 2 * H;
    constexpr uint32_t G = (sizeof(T) == 4 && (H & 1)) ? 2 : 1;
    constexpr uint32_t V = G * M;
    static_assert(V % (16 / sizeof(T)) == 0, "a group is whole 16-byte pieces");
    const uint32_t idx = blockIdx.x * kQamThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, g = idx - row * W;
    const double* src = y + (int64_t)row * ldy;
    const double* hsrc = h + (int64_t)row * ldh;
    T v[V];
#pragma unroll
    for (uint32_t k = 0; k < G; ++k) {
        const uint32_t s = g * G + k;
        double yi = 0.0, yq = 0.0, hr = 1.0, hi = 0.0;  // a symbol behind S: its LLRs are not stored
        if (s < S) {
            qam_load2(src + 2 * (int64_t)s, yi, yq);
            qam_load2(hsrc + 2 * (int64_t)(s / Lc), hr, hi);
        }
        const double g2 = hr * hr + hi * hi;
        const double ui = hr * yi + hi * yq;
        const double uq = hr * yq - hi * yi;
        const double wg = w * g2;
        double li[H], lq[H];
        qam_axis_llr<H>(ui / g2, scale, wg, li);
        qam_axis_llr<H>(uq / g2, scale, wg, lq);
        const bool erased = g2 == 0.0;
#pragma unroll
        for (int p = 0; p < H; ++p) {
            v[k * M + 2 * p] = erased ? (T)0.0 : (T)li[p];
            v[k * M + 2 * p + 1] = erased ? (T)0.0 : (T)lq[p];
        }
    }
    const uint32_t t0 = g * V;  // < E: W = ceil(E / V)
    qam_store_cut<V, T>(llr + (int64_t)row * ldl + t0, v, E - t0);
}

// ---- the exact log-MAP demapper; the definition: include/polarldpc.h at pl_qam_demap_logmap ----
// glibc's expm1 and log1p (libm_exact.hpp, whose functions stay as they are) on the arguments the definition can
// produce: q = (D_v - d_a) W is <= 0, -inf or NaN (D_v is the minimum and W >= 0 or NaN), T_v - 1.0 is in [0, 7] or NaN.
PL_DEV double qam_expm1(double x) {
    if (x != x) return x + x;  // NaN
    if (x == -__builtin_inf()) return -1.0;
    return libm_expm1(x);
}

PL_DEV double qam_log1p(double x) {
    if (x != x) return x + x;  // NaN
    return libm_log1p_pos(x);
}

// glibc's expm1 returns its constant (tiny - 1.0 = -1.0) from the first double whose high word is 0x4043687A on, the
// 56 ln 2 of its comment; e is then +0.0 and T_v + 0.0 is T_v bit for bit (T_v is never -0.0: it starts at +0.0 and
// only terms >= +0.0 are added).  A NaN q fails the comparison and takes the whole path.
constexpr double kQamSkip = -0x1.3687ap+5;

// the H minima pairs of one axis value, qam_axis_llr's d0 and d1
template <int H>
PL_DEV void qam_axis_minima(double r, double scale, double (&D0)[H], double (&D1)[H]) {
    constexpr int L = 1 << H;
    double d[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
        const double t = r - (double)((L - 1) - 2 * i) * scale;
        d[i] = t * t;
    }
#pragma unroll
    for (int p = 0; p < H; ++p) {
        double d0 = d[0], d1 = d[1 << (H - 1 - p)];
#pragma unroll
        for (int i = 1; i < L; ++i) {
            if (((i ^ (i >> 1)) >> (H - 1 - p)) & 1) {
                if (i != (1 << (H - 1 - p))) d1 = __builtin_fmin(d1, d[i]);
            } else {
                d0 = __builtin_fmin(d0, d[i]);
            }
        }
        D0[p] = d0;
        D1[p] = d1;
    }
}

// the H LLRs of one axis value r at weight W.  The levels run in a rolled loop in ascending index, so that the
// kernel holds H copies of expm1 and not H 2^H: level i's distance is computed again (the same two operations give
// the same double) and goes to T_0 or T_1 of each bit by the bit the level carries there.  The sums sit in 2 H
// registers whatever the level count.
template <int H>
PL_DEV void qam_axis_llr_logmap(double r, double scale, double W, double (&llr)[H]) {
    constexpr int L = 1 << H;
    double D0[H], D1[H], T0[H], T1[H];
    qam_axis_minima<H>(r, scale, D0, D1);
#pragma unroll
    for (int p = 0; p < H; ++p) T0[p] = T1[p] = 0.0;
#pragma unroll 1
    for (int i = 0; i < L; ++i) {
        const double t = r - (double)((L - 1) - 2 * i) * scale;
        const double d = t * t;
        const int gray = i ^ (i >> 1);
#pragma unroll
        for (int p = 0; p < H; ++p) {
            const bool one = (gray >> (H - 1 - p)) & 1;
            const double q = ((one ? D1[p] : D0[p]) - d) * W;
            if (!(q <= kQamSkip)) {
                const double e = qam_expm1(q) + 1.0;
                const double s0 = T0[p] + e, s1 = T1[p] + e;
                T0[p] = one ? T0[p] : s0;
                T1[p] = one ? s1 : T1[p];
            }
        }
    }
#pragma unroll
    for (int p = 0; p < H; ++p) {
        const double c0 = qam_log1p(T0[p] - 1.0), c1 = qam_log1p(T1[p] - 1.0);
        llr[p] = ((D1[p] - D0[p]) * W) + (c0 - c1);
    }
}

// qam_demap_kernel's and qam_demap_csi_kernel's groups, loads and stores (CSI: with the channel state) around the
// log-MAP arithmetic.  The 2 G axis values of a group go through one copy of that arithmetic, in a rolled loop
// whose counter is uniform over the wave: the selects in front of it and behind it compare that counter with
// constants, and v stays in registers.
template <int H, typename T, bool CSI>
__global__ void __launch_bounds__(kQamThreads)
qam_demap_logmap_kernel(const double* __restrict__ y, int64_t ldy, const double* __restrict__ h, int64_t ldh, uint32_t E,
                        uint32_t S, uint32_t Lc, uint32_t W, uint32_t total, double scale, double w,
                        T* __restrict__ llr, int64_t ldl) {
    constexpr uint32_t M = 2 * H;
    constexpr uint32_t G = (sizeof(T) == 4 && (H & 1)) ? 2 : 1;
    constexpr uint32_t V = G * M;
    static_assert(V % (16 / sizeof(T)) == 0, "a group is whole 16-byte pieces");
    const uint32_t idx = blockIdx.x * kQamThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / W, g = idx - row * W;
    const double* src = y + (int64_t)row * ldy;
    double r[2 * G], wt[G];
    bool erased[G];
#pragma unroll
    for (uint32_t k = 0; k < G; ++k) {
        const uint32_t s = g * G + k;
        double yi = 0.0, yq = 0.0, hr = 1.0, hi = 0.0;  // a symbol behind S: its LLRs are not stored
        if (s < S) {
            qam_load2(src + 2 * (int64_t)s, yi, yq);
            if (CSI) qam_load2(h + (int64_t)row * ldh + 2 * (int64_t)(s / Lc), hr, hi);
        }
        if (CSI) {
            const double g2 = hr * hr + hi * hi;
            const double ui = hr * yi + hi * yq;
            const double uq = hr * yq - hi * yi;
            r[2 * k] = ui / g2;
            r[2 * k + 1] = uq / g2;
            wt[k] = w * g2;
            erased[k] = g2 == 0.0;
        } else {
            r[2 * k] = yi;
            r[2 * k + 1] = yq;
            wt[k] = w;
            erased[k] = false;
        }
    }
    T v[V];
#pragma unroll 1
    for (uint32_t a = 0; a < 2 * G; ++a) {
        double ra = r[0], wa = wt[0];
        bool er = erased[0];
#pragma unroll
        for (uint32_t j = 1; j < 2 * G; ++j) {
            if (a == j) {
                ra = r[j];
                wa = wt[j / 2];
                er = erased[j / 2];
            }
        }
        double l[H];
        qam_axis_llr_logmap<H>(ra, scale, wa, l);
#pragma unroll
        for (uint32_t j = 0; j < 2 * G; ++j) {
            if (a == j) {
#pragma unroll
                for (int p = 0; p < H; ++p) v[(j / 2) * M + 2 * p + (j & 1)] = er ? (T)0.0 : (T)l[p];
            }
        }
    }
    const uint32_t t0 = g * V;  // < E: W = ceil(E / V)
    qam_store_cut<V, T>(llr + (int64_t)row * ldl + t0, v, E - t0);
}

// rows of W work-items each, in launches below 2^31 work-items; fn(first row, work-items)
template <class Launch>
static hipError_t qam_chunks(int64_t batch, int64_t W, Launch fn) {
    const int64_t step = kQamMaxItems / W;  // W <= 2^29: at least 3 rows
    for (int64_t b0 = 0; b0 < batch; b0 += step) {
        const int64_t rows = batch - b0 < step ? batch - b0 : step;
        const hipError_t e = fn(b0, (uint32_t)(rows * W));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int H, bool NOISE>
static hipError_t qam_tx(const uint8_t* e, int64_t lde, int64_t E, int64_t S, int64_t batch, double scale,
                         double sigma, uint64_t seed, int64_t off, double* out, int64_t ldo, hipStream_t st) {
    return qam_chunks(batch, S, [&](int64_t b0, uint32_t total) {
        hipLaunchKernelGGL((qam_tx_kernel<H, NOISE>), dim3((total + kQamThreads - 1) / kQamThreads), dim3(kQamThreads),
                           0, st, e ? e + b0 * lde : e, lde, (uint32_t)E, (uint32_t)S, total, scale, sigma, seed,
                           (uint64_t)(off + b0), out + b0 * ldo, ldo);
        return hipGetLastError();
    });
}

template <bool NOISE>
static hipError_t qam_tx_m(int m, const uint8_t* e, int64_t lde, int64_t E, int64_t S, int64_t batch, double scale,
                           double sigma, uint64_t seed, int64_t off, double* out, int64_t ldo, hipStream_t st) {
    switch (m) {
        case 2: return qam_tx<1, NOISE>(e, lde, E, S, batch, scale, sigma, seed, off, out, ldo, st);
        case 4: return qam_tx<2, NOISE>(e, lde, E, S, batch, scale, sigma, seed, off, out, ldo, st);
        case 6: return qam_tx<3, NOISE>(e, lde, E, S, batch, scale, sigma, seed, off, out, ldo, st);
        default: return qam_tx<4, NOISE>(e, lde, E, S, batch, scale, sigma, seed, off, out, ldo, st);
    }
}

hipError_t qam_modulate_launch(int m, int64_t E, int64_t S, double scale, const uint8_t* e, int64_t lde, int64_t batch,
                               double* x, int64_t ldx, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    return qam_tx_m<false>(m, e, lde, E, S, batch, scale, 0.0, 0, 0, x, ldx, s);
}

hipError_t qam_awgn_launch(int m, int64_t E, int64_t S, double scale, const uint8_t* e, int64_t lde, int64_t batch,
                           double sigma, uint64_t seed, int64_t off, double* y, int64_t ldy, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    return qam_tx_m<true>(m, e, lde, E, S, batch, scale, sigma, seed, off, y, ldy, s);
}

template <int H, typename T>
static hipError_t qam_demap(int64_t E, int64_t S, double scale, const double* y, int64_t ldy, int64_t batch, double w,
                            T* llr, int64_t ldl, hipStream_t st) {
    constexpr int64_t V = ((sizeof(T) == 4 && (H & 1)) ? 2 : 1) * 2 * H;
    const int64_t W = (E + V - 1) / V;
    return qam_chunks(batch, W, [&](int64_t b0, uint32_t total) {
        hipLaunchKernelGGL((qam_demap_kernel<H, T>), dim3((total + kQamThreads - 1) / kQamThreads), dim3(kQamThreads), 0,
                           st, y + b0 * ldy, ldy, (uint32_t)E, (uint32_t)S, (uint32_t)W, total, scale, w,
                           llr + b0 * ldl, ldl);
        return hipGetLastError();
    });
}

template <typename T>
static hipError_t qam_demap_m(int m, int64_t E, int64_t S, double scale, const double* y, int64_t ldy, int64_t batch,
                              double w, T* llr, int64_t ldl, hipStream_t st) {
    switch (m) {
        case 2: return qam_demap<1, T>(E, S, scale, y, ldy, batch, w, llr, ldl, st);
        case 4: return qam_demap<2, T>(E, S, scale, y, ldy, batch, w, llr, ldl, st);
        case 6: return qam_demap<3, T>(E, S, scale, y, ldy, batch, w, llr, ldl, st);
        default: return qam_demap<4, T>(E, S, scale, y, ldy, batch, w, llr, ldl, st);
    }
}

hipError_t qam_demap_launch(int m, int64_t E, int64_t S, double scale, const double* y, int64_t ldy, int64_t batch,
                            double w, void* llr, int64_t ldl, bool llr_f32, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    return llr_f32 ? qam_demap_m(m, E, S, scale, y, ldy, batch, w, (float*)llr, ldl, s)
                   : qam_demap_m(m, E, S, scale, y, ldy, batch, w, (double*)llr, ldl, s);
}

template <int H>
static hipError_t qam_rayleigh(const uint8_t* e, int64_t lde, int64_t E, int64_t S, int64_t Lc, int64_t batch,
                               double scale, double sigma, uint64_t seed, int64_t off, double* y, int64_t ldy, double* h,
                               int64_t ldh, hipStream_t st) {
    return qam_chunks(batch, S, [&](int64_t b0, uint32_t total) {
        hipLaunchKernelGGL((qam_rayleigh_kernel<H>), dim3((total + kQamThreads - 1) / kQamThreads), dim3(kQamThreads), 0,
                           st, e ? e + b0 * lde : e, lde, (uint32_t)E, (uint32_t)S, (uint32_t)Lc, total, scale, sigma,
                           seed, (uint64_t)(off + b0), y + b0 * ldy, ldy, h + b0 * ldh, ldh);
        return hipGetLastError();
    });
}

hipError_t qam_rayleigh_launch(int m, int64_t E, int64_t S, int64_t Lc, double scale, const uint8_t* e, int64_t lde,
                               int64_t batch, double sigma, uint64_t seed, int64_t off, double* y, int64_t ldy,
                               double* h, int64_t ldh, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    switch (m) {
        case 2: return qam_rayleigh<1>(e, lde, E, S, Lc, batch, scale, sigma, seed, off, y, ldy, h, ldh, s);
        case 4: return qam_rayleigh<2>(e, lde, E, S, Lc, batch, scale, sigma, seed, off, y, ldy, h, ldh, s);
        case 6: return qam_rayleigh<3>(e, lde, E, S, Lc, batch, scale, sigma, seed, off, y, ldy, h, ldh, s);
        default: return qam_rayleigh<4>(e, lde, E, S, Lc, batch, scale, sigma, seed, off, y, ldy, h, ldh, s);
    }
}

template <int H, typename T>
static hipError_t qam_demap_csi(int64_t E, int64_t S, int64_t Lc, double scale, const double* y, int64_t ldy,
                                const double* h, int64_t ldh, int64_t batch, double w, T* llr, int64_t ldl,
                                hipStream_t st) {
    constexpr int64_t V = ((sizeof(T) == 4 && (H & 1)) ? 2 : 1) * 2 * H;
    const int64_t W = (E + V - 1) / V;
    return qam_chunks(batch, W, [&](int64_t b0, uint32_t total) {
        hipLaunchKernelGGL((qam_demap_csi_kernel<H, T>), dim3((total + kQamThreads - 1) / kQamThreads),
                           dim3(kQamThreads), 0, st, y + b0 * ldy, ldy, h + b0 * ldh, ldh, (uint32_t)E, (uint32_t)S,
                           (uint32_t)Lc, (uint32_t)W, total, scale, w, llr + b0 * ldl, ldl);
        return hipGetLastError();
    });
}

template <typename T>
static hipError_t qam_demap_csi_m(int m, int64_t E, int64_t S, int64_t Lc, double scale, const double* y, int64_t ldy,
                                  const double* h, int64_t ldh, int64_t batch, double w, T* llr, int64_t ldl,
                                  hipStream_t st) {
    switch (m) {
        case 2: return qam_demap_csi<1, T>(E, S, Lc, scale, y, ldy, h, ldh, batch, w, llr, ldl, st);
        case 4: return qam_demap_csi<2, T>(E, S, Lc, scale, y, ldy, h, ldh, batch, w, llr, ldl, st);
        case 6: return qam_demap_csi<3, T>(E, S, Lc, scale, y, ldy, h, ldh, batch, w, llr, ldl, st);
        default: return qam_demap_csi<4, T>(E, S, Lc, scale, y, ldy, h, ldh, batch, w, llr, ldl, st);
    }
}

hipError_t qam_demap_csi_launch(int m, int64_t E, int64_t S, int64_t Lc, double scale, const double* y, int64_t ldy,
                                const double* h, int64_t ldh, int64_t batch, double w, void* llr, int64_t ldl,
                                bool llr_f32, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    return llr_f32 ? qam_demap_csi_m(m, E, S, Lc, scale, y, ldy, h, ldh, batch, w, (float*)llr, ldl, s)
                   : qam_demap_csi_m(m, E, S, Lc, scale, y, ldy, h, ldh, batch, w, (double*)llr, ldl, s);
}

template <int H, typename T, bool CSI>
static hipError_t qam_demap_logmap(int64_t E, int64_t S, int64_t Lc, double scale, const double* y, int64_t ldy,
                                   const double* h, int64_t ldh, int64_t batch, double w, T* llr, int64_t ldl,
                                   hipStream_t st) {
    constexpr int64_t V = ((sizeof(T) == 4 && (H & 1)) ? 2 : 1) * 2 * H;
    const int64_t W = (E + V - 1) / V;
    return qam_chunks(batch, W, [&](int64_t b0, uint32_t total) {
        hipLaunchKernelGGL((qam_demap_logmap_kernel<H, T, CSI>), dim3((total + kQamThreads - 1) / kQamThreads),
                           dim3(kQamThreads), 0, st, y + b0 * ldy, ldy, CSI ? h + b0 * ldh : h, ldh, (uint32_t)E,
                           (uint32_t)S, (uint32_t)Lc, (uint32_t)W, total, scale, w, llr + b0 * ldl, ldl);
        return hipGetLastError();
    });
}

template <typename T, bool CSI>
static hipError_t qam_demap_logmap_m(int m, int64_t E, int64_t S, int64_t Lc, double scale, const double* y,
                                     int64_t ldy, const double* h, int64_t ldh, int64_t batch, double w, T* llr,
                                     int64_t ldl, hipStream_t st) {
    switch (m) {
        case 2: return qam_demap_logmap<1, T, CSI>(E, S, Lc, scale, y, ldy, h, ldh, batch, w, llr, ldl, st);
        case 4: return qam_demap_logmap<2, T, CSI>(E, S, Lc, scale, y, ldy, h, ldh, batch, w, llr, ldl, st);
        case 6: return qam_demap_logmap<3, T, CSI>(E, S, Lc, scale, y, ldy, h, ldh, batch, w, llr, ldl, st);
        default: return qam_demap_logmap<4, T, CSI>(E, S, Lc, scale, y, ldy, h, ldh, batch, w, llr, ldl, st);
    }
}

hipError_t qam_demap_logmap_launch(int m, int64_t E, int64_t S, int64_t Lc, double scale, const double* y, int64_t ldy,
                                   const double* h, int64_t ldh, int64_t batch, double w, void* llr, int64_t ldl,
                                   bool llr_f32, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    if (h)
        return llr_f32 ? qam_demap_logmap_m<float, true>(m, E, S, Lc, scale, y, ldy, h, ldh, batch, w, (float*)llr, ldl, s)
                       : qam_demap_logmap_m<double, true>(m, E, S, Lc, scale, y, ldy, h, ldh, batch, w, (double*)llr, ldl, s);
    return llr_f32 ? qam_demap_logmap_m<float, false>(m, E, S, 1, scale, y, ldy, h, 0, batch, w, (float*)llr, ldl, s)
                   : qam_demap_logmap_m<double, false>(m, E, S, 1, scale, y, ldy, h, 0, batch, w, (double*)llr, ldl, s);
}

}  // namespace pl
